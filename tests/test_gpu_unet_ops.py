"""The U-Net kernels of csrc/unet_ops.hip (2 x 2 average pool, 2 x 2 stride-2 up-convolution, 1 x 1 convolution, their input and
weight gradients) against float64 torch on the CPU, element by element, through the raw entry points.

References: `F.avg_pool2d`, `F.conv_transpose2d`, `F.conv2d` and their autograd on float64 copies of the operands.

Bounds, per element, EVERY element compared:
* products (forward, input gradient, weight and bias gradient): |err| <= 1e-6 * S + ulp(ref), the form and constants of
  tests/test_gpu_conv_ops.py (derivation there): S is the same operation on the absolute values of the operands, in float64.
* pool forward: |err| <= 2^-24 (|a| + |b| + |c| + |d|): three fp32 additions, each within 2^-24 relative of a partial sum
  that is at most the sum of the absolute values; the multiplication by 0.25 is exact.
* pool backward: bit-equal to 0.25 * dy at all four positions.
64 sentinel floats behind every buffer (scratch included) must come back bit for bit; the kernels that ran are read from
lib.kernel_accounting(); every launch is repeated on the same operands and must be bit-identical (no atomics: the weight
gradient folds its per-workgroup partial sums in a fixed order); a second weight-gradient launch into the same buffers must
exactly double them (it accumulates, and x + x is exact).
"""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_ops import Out, bits, check, cl

pytestmark = pytest.mark.gpu

POOL_SHAPES = [(1, 2, 2, 1), (3, 4, 8, 5), (1, 6, 10, 8), (1, 34, 46, 13), (2, 16, 16, 64)]
# (B, H, W, Cin, Cout): H, W the up-convolution's INPUT grid; the 1 x 1 convolution runs on npix = B H W.  The last shape has
# 12 pixel tiles for fewer weight-gradient splits (1 x 1: 17 x 3 blocks, S = 11; up-convolution: 17 x 9 blocks, S = 4), so a
# workgroup walks more than one tile and prefetches tile t + S; in every other shape S is the tile count
GEMM_SHAPES = [(1, 1, 1, 1, 1), (3, 2, 4, 5, 3), (1, 3, 5, 16, 8), (1, 4, 8, 13, 57), (2, 8, 16, 64, 32), (1, 5, 7, 57, 1),
               (1, 8, 8, 264, 132), (1, 4, 4, 528, 264), (1, 16, 48, 264, 132)]


def sentinels(outs):
    for k, o in outs.items():
        assert o.sentinels_intact(), f"{k}: the floats behind the buffer were written"


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "B{}_{}x{}_c{}".format(*s))
def test_avgpool2x2(cuda, shape):
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    B, H, W, C = shape
    gen = torch.Generator().manual_seed(300 + C)
    x = torch.randn(B, C, H, W, generator=gen)
    dy = torch.randn(B, C, H // 2, W // 2, generator=gen)
    xg, dyg = cl(x).to(cuda), cl(dy).to(cuda)
    runs = []
    with L.kernel_accounting() as acc:
        for rep in range(2):
            y, dx = Out((B, H // 2, W // 2, C), cuda, gen), Out((B, H, W, C), cuda, gen)
            L.check(lib.dlwp_avgpool2x2_fwd(L.ptr(xg), L.ptr(y.t), B, H, W, C, L.stream()))
            L.check(lib.dlwp_avgpool2x2_bwd(L.ptr(dyg), L.ptr(dx.t), B, H, W, C, L.stream()))
            torch.cuda.synchronize()
            sentinels({"y": y, "dx": dx})
            runs.append((y, dx))
    assert {r["name"]: r["calls"] for r in acc.rows} == {"avgpool2x2_fwd": 2, "avgpool2x2_bwd": 2}, acc.rows
    (y, dx), (y2, dx2) = runs
    assert torch.equal(bits(y.t), bits(y2.t)) and torch.equal(bits(dx.t), bits(dx2.t))
    ref = F.avg_pool2d(x.double(), 2, 2)
    bound = 2.0 ** -24 * 4.0 * F.avg_pool2d(x.double().abs(), 2, 2)
    err = (y.t.permute(0, 3, 1, 2).double().cpu() - ref).abs()
    print(f"  pool {shape}: max |err| {err.max():.3e}, worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    expect = (0.25 * cl(dy)).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(bits(dx.t.cpu()), bits(expect))


def gemm_reference(op, x, w, b, gy):
    """float64 forward + autograd of the layer and the same graph on absolute values (S)"""
    def run(x_, w_, b_, g_):
        x_, w_, b_ = x_.requires_grad_(True), w_.requires_grad_(True), b_.requires_grad_(True)
        y = op(x_, w_, b_)
        y.backward(g_)
        return y.detach(), x_.grad, w_.grad, b_.grad
    d = lambda t: t.detach().double().clone()      # noqa: E731
    return run(d(x), d(w), d(b), d(gy)), run(d(x).abs(), d(w).abs(), d(b).abs(), d(gy).abs())


@pytest.mark.parametrize("up", [True, False], ids=["upconv2x2", "conv1x1"])
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=lambda s: "B{}_{}x{}_c{}_n{}".format(*s))
def test_pixel_gemm_forward_and_gradients(cuda, shape, up):
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    B, H, W, Cin, Cout = shape
    gen = torch.Generator().manual_seed(500 + Cin + 2 * Cout + int(up))
    x = torch.randn(B, Cin, H, W, generator=gen)
    b = torch.randn(Cout, generator=gen)
    if up:
        w = torch.randn(Cin, Cout, 2, 2, generator=gen) / Cin ** 0.5
        gy = torch.randn(B, Cout, 2 * H, 2 * W, generator=gen)
        op = lambda x_, w_, b_: F.conv_transpose2d(x_, w_, b_, stride=2)      # noqa: E731
    else:
        w = torch.randn(Cout, Cin, 1, 1, generator=gen) / Cin ** 0.5
        gy = torch.randn(B, Cout, H, W, generator=gen)
        op = F.conv2d
    (y_ref, gx_ref, gw_ref, gb_ref), (S_y, S_gx, S_gw, S_gb) = gemm_reference(op, x, w, b, gy)
    xg, wg, bg, gyg = cl(x).to(cuda), w.to(cuda), b.to(cuda), cl(gy).to(cuda)
    npix = B * H * W
    n_ws = lib.dlwp_upconv2x2_wgrad_ws_floats(B, H, W, Cin, Cout) if up else lib.dlwp_conv1x1_wgrad_ws_floats(npix, Cin, Cout)
    assert n_ws > 0

    def wgrad(o):
        if up:
            L.check(lib.dlwp_upconv2x2_wgrad(L.ptr(xg), L.ptr(gyg), L.ptr(o["ws"].t), L.ptr(o["gw"].t), L.ptr(o["gb"].t), B, H, W, Cin, Cout,
                                             L.stream()))
        else:
            L.check(lib.dlwp_conv1x1_wgrad(L.ptr(xg), L.ptr(gyg), L.ptr(o["ws"].t), L.ptr(o["gw"].t), L.ptr(o["gb"].t), npix, Cin, Cout,
                                           L.stream()))

    def launch():
        o = {"y": Out(tuple(gyg.shape), cuda, gen), "gx": Out(tuple(xg.shape), cuda, gen), "ws": Out((n_ws,), cuda, gen),
             "gw": Out(tuple(w.shape), cuda, gen, zero=True), "gb": Out((Cout,), cuda, gen, zero=True)}
        s = L.stream()
        if up:
            L.check(lib.dlwp_upconv2x2_fwd(L.ptr(xg), L.ptr(wg), L.ptr(bg), L.ptr(o["y"].t), B, H, W, Cin, Cout, s))
            L.check(lib.dlwp_upconv2x2_dgrad(L.ptr(gyg), L.ptr(wg), L.ptr(o["gx"].t), B, H, W, Cin, Cout, s))
        else:
            L.check(lib.dlwp_conv1x1_fwd(L.ptr(xg), L.ptr(wg), L.ptr(bg), L.ptr(o["y"].t), npix, Cin, Cout, s))
            L.check(lib.dlwp_conv1x1_dgrad(L.ptr(gyg), L.ptr(wg), L.ptr(o["gx"].t), npix, Cin, Cout, s))
        wgrad(o)
        torch.cuda.synchronize()
        sentinels(o)
        return o

    with L.kernel_accounting() as acc:
        o = launch()
    rows = {r["name"]: r["calls"] for r in acc.rows}
    expect = {"pixel_wgrad": 1, "pixel_wgrad_fold": 1}
    expect.update({"upconv2x2_fwd": 1, "upconv2x2_dgrad": 1} if up else {"conv1x1": 2})
    assert rows == expect, (rows, expect)
    print(shape, "upconv2x2" if up else "conv1x1")
    check("y", o["y"].t.permute(0, 3, 1, 2), y_ref, S_y)
    check("gx", o["gx"].t.permute(0, 3, 1, 2), gx_ref, S_gx)
    check("gw", o["gw"].t, gw_ref, S_gw)
    check("gb", o["gb"].t, gb_ref, S_gb)
    # ---- the same launches again: bit-identical
    o2 = launch()
    for k in ("y", "gx", "gw", "gb"):
        assert torch.equal(bits(o[k].t), bits(o2[k].t)), f"{k}: two launches on the same operands differ"
    # ---- accumulation: a second weight-gradient launch into the same buffers doubles them
    wgrad(o)
    torch.cuda.synchronize()
    sentinels(o)
    assert torch.equal(bits(o["gw"].t), bits(2 * o2["gw"].t)) and torch.equal(bits(o["gb"].t), bits(2 * o2["gb"].t))
    # ---- no bias: NULL bias forward, NULL gb in the weight gradient
    y0 = Out(tuple(gyg.shape), cuda, gen)
    gw0, ws0 = Out(tuple(w.shape), cuda, gen, zero=True), Out((n_ws,), cuda, gen)
    if up:
        L.check(lib.dlwp_upconv2x2_fwd(L.ptr(xg), L.ptr(wg), None, L.ptr(y0.t), B, H, W, Cin, Cout, L.stream()))
        L.check(lib.dlwp_upconv2x2_wgrad(L.ptr(xg), L.ptr(gyg), L.ptr(ws0.t), L.ptr(gw0.t), None, B, H, W, Cin, Cout, L.stream()))
    else:
        L.check(lib.dlwp_conv1x1_fwd(L.ptr(xg), L.ptr(wg), None, L.ptr(y0.t), npix, Cin, Cout, L.stream()))
        L.check(lib.dlwp_conv1x1_wgrad(L.ptr(xg), L.ptr(gyg), L.ptr(ws0.t), L.ptr(gw0.t), None, npix, Cin, Cout, L.stream()))
    torch.cuda.synchronize()
    sentinels({"y0": y0, "gw0": gw0, "ws0": ws0})
    check("y without bias", y0.t.permute(0, 3, 1, 2), y_ref - b.double().view(1, -1, 1, 1), S_y - b.double().abs().view(1, -1, 1, 1))
    assert torch.equal(bits(gw0.t), bits(o2["gw"].t))


def test_autograd_ops_and_layers_match_torch(cuda):
    """conv_ops.avg_pool2x2 / upconv2x2 / conv1x1 through autograd, and the channels-first `forward` of UpConv2x2 / Conv1x1
    loaded from the torch layers' state_dict, against the torch layers in float64 (rel_gap bars of the model tests)."""
    from dlwp_benchmark_amd import conv_ops
    from unet_ref import rel_gap
    gen = torch.Generator().manual_seed(9)
    torch.manual_seed(9)
    x = torch.randn(2, 7, 6, 10, generator=gen)
    ref_up, ref_out = torch.nn.ConvTranspose2d(7, 5, 2, stride=2), torch.nn.Conv2d(5, 3, 1)
    up, out = conv_ops.UpConv2x2(7, 5), conv_ops.Conv1x1(5, 3)
    up.load_state_dict(ref_up.state_dict(), strict=True)
    out.load_state_dict(ref_out.state_dict(), strict=True)
    up, out = up.to(cuda), out.to(cuda)
    ref_up, ref_out = ref_up.double(), ref_out.double()
    xr = x.double().requires_grad_(True)
    yr = ref_out(F.avg_pool2d(ref_up(xr), 2, 2))
    yr.square().sum().backward()
    xg = x.to(cuda).requires_grad_(True)
    y = out(conv_ops.avg_pool2x2(up(xg).permute(0, 2, 3, 1)).permute(0, 3, 1, 2))
    y.square().sum().backward()
    torch.cuda.synchronize()
    assert rel_gap(y.detach().cpu(), yr.detach()) <= 1e-4
    assert rel_gap(xg.grad.cpu(), xr.grad) <= 5e-4
    for mine, ref in ((up, ref_up), (out, ref_out)):
        assert rel_gap(mine.weight.grad.cpu(), ref.weight.grad) <= 5e-4 and rel_gap(mine.bias.grad.cpu(), ref.bias.grad) <= 5e-4
    with torch.no_grad():
        y_eval = out(conv_ops.avg_pool2x2(up(xg).permute(0, 2, 3, 1)).permute(0, 3, 1, 2))
    assert not y_eval.requires_grad and torch.equal(bits(y_eval), bits(y))
