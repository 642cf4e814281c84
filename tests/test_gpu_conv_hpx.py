"""The 3 x 3 convolution kernels with HEALPix padding (csrc/conv3x3.hip MODE_HPX / MODE_HPX_DGRAD and the fold kernel) against
float64 torch on the CPU, element by element, through `conv_ops.conv3x3` and `conv_ops.convlstm_cell` with autograd.

Reference: `F.conv2d` (and its autograd) on float64 copies of the operands behind tests/hpx_ref.py `hpx_pad1`, which
tests/test_hpx_ref.py pins to the reference's own padded output.

Bound: the per-element bound of tests/test_gpu_conv_ops.py, UNCHANGED -- |err| <= 1e-6 * S + ulp(result) [+ 4.8e-7 behind tanh /
sigmoid] [+ carried error], every element compared, `check`, `cell_bounds` and the helpers imported from there.  S is the same
graph on absolute values: the padding weights (1, 0.5) are non-negative, so autograd through `hpx_pad1` of |x| gives it, for the
input gradient too.  What the mode adds to the arithmetic: a mean-of-two cell is one addition and an exact halving before the
product (1 rounding of an operand, 6e-8 relative, inside its |a| |b| term), and the input gradient's fold adds at most four ring
cells to the interior value, 4 roundings of at most 6e-8 * S each; with the documented 3.5e-7 * S of the MFMA chain this stays
under 1e-6 * S.

Every case runs twice through autograd and once more through the raw entry points with sentinel floats behind every output: all
three must agree bit for bit (no atomics anywhere; the fold adds in the table's fixed order), and the sentinels must be intact.

Shapes: face 2 and 4 (the whole face and both mean-of-two corners inside one tile; one and two spheres), face 8 (the published
mesh, half a tile wide), face 24 (3 x 2 tiles, ragged in width: an interior tile edge stays in the face while a face edge leaves
it); channel forms (5, 0, 13) -- the 16-column path -- and (16, 1, 57) -- two inputs, the 64-column path; the cell at face 8
with 57 + 57 -> 228 channels, with and without h_prev / c_prev.
"""
import pytest
import torch
import torch.nn.functional as F

from hpx_ref import hpx_pad1
from test_gpu_conv_ops import FN_ULP, Out, bits, cell_bounds, check, cl, ulp32

pytestmark = pytest.mark.gpu

HPX = "healpix"
ACTC = {None: 0, "tanh": 1, "relu": 2}
# (spheres, face size, C1, C2, Cout, act)
CASES = [
    (1, 2, 5, 0, 13, "tanh"),
    (2, 2, 16, 1, 57, None),
    (1, 4, 16, 1, 57, "relu"),
    (2, 4, 5, 0, 13, None),
    (1, 8, 5, 0, 13, "relu"),
    (2, 8, 16, 1, 57, "tanh"),
    (1, 24, 5, 0, 13, None),
    (1, 24, 16, 1, 57, "relu"),
]


def reference(x, w, b, gy, act):
    """test_gpu_conv_ops.reference with the HEALPix padding: float64 forward + autograd, the same graph on absolute values (S)
    and with the carried dz error as the upstream gradient (E)"""
    xd, wd, bd = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv2d(hpx_pad1(xd), wd, bd)
    y = torch.tanh(pre) if act == "tanh" else (torch.relu(pre) if act == "relu" else pre)
    y.backward(gy.double())
    xa, wa = x.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True)
    S_y = F.conv2d(hpx_pad1(xa), wa, b.double().abs())
    e_y = 1e-6 * S_y.detach() + ulp32(pre.detach())
    g = gy.double()
    if act == "tanh":
        dz = g * (1 - y.detach() ** 2)
        e_y = e_y + FN_ULP
        dz_err = g.abs() * (2 * y.detach().abs() * e_y + e_y ** 2) + 3 * ulp32(dz)
    elif act == "relu":
        dz = g * (pre.detach() > 0)
        dz_err = g.abs() * (pre.detach().abs() <= e_y)
    else:
        dz, dz_err = g, torch.zeros_like(g)
    S_y.backward(dz.abs(), retain_graph=True)
    S = {"y": S_y.detach(), "gx": xa.grad.clone(), "gw": wa.grad.clone(), "gb": dz.abs().sum(dim=(0, 2, 3))}
    xa.grad, wa.grad = None, None
    S_y.backward(dz_err)
    E = {"gx": xa.grad, "gw": wa.grad, "gb": dz_err.sum(dim=(0, 2, 3))}
    return y.detach(), xd.grad, wd.grad, bd.grad, S, E


def run_raw(dev, gen, x1, x2, w, b, gy_cl, act):
    """pack, forward, (activation backward,) HEALPix input gradient, weight gradient through the raw entry points, every output
    with sentinel floats behind it"""
    from dlwp_benchmark_amd import conv_ops, lib as L
    lib = L.load()
    B, n, _, C1 = x1.shape
    C2 = x2.shape[-1] if x2 is not None else 0
    Cout, a = w.shape[0], ACTC[act]
    img_f = Out((lib.dlwp_conv3x3_image_floats(C1 + C2, Cout, 0),), dev, gen)
    img_b = Out((lib.dlwp_conv3x3_image_floats(C1 + C2, Cout, 2),), dev, gen)
    y, g1 = Out((B, n, n, Cout), dev, gen), Out((B, n, n, C1), dev, gen)
    g2 = Out((B, n, n, C2), dev, gen) if C2 else None
    dz = Out((B, n, n, Cout), dev, gen) if a else None
    gw, gb = Out(tuple(w.shape), dev, gen, zero=True), Out((Cout,), dev, gen, zero=True)
    ws = Out((lib.dlwp_conv3x3_wgrad_ws_floats(B, n, n, C1 + C2, Cout),), dev, gen)
    G = Out((lib.dlwp_conv3x3_hpx_dgrad_ws_floats(B, n, C1 + C2),), dev, gen)
    table = torch.from_numpy(conv_ops.hpx_fold_table(n)).to(dev)
    s = L.stream()
    L.check(lib.dlwp_conv3x3_pack(L.ptr(w), L.ptr(img_f.t), C1 + C2, Cout, 0, s))
    L.check(lib.dlwp_conv3x3_pack(L.ptr(w), L.ptr(img_b.t), C1 + C2, Cout, 2, s))
    L.check(lib.dlwp_conv3x3_fwd(L.ptr(x1), L.ptr(x2), L.ptr(img_f.t), L.ptr(b), L.ptr(y.t), None, B, n, n, C1, C2, Cout, 0, 2, 2, a, s))
    d = gy_cl
    if a:
        L.check(lib.dlwp_conv3x3_act_bwd(L.ptr(y.t), L.ptr(gy_cl), L.ptr(dz.t), gy_cl.numel(), a, s))
        d = dz.t
    L.check(lib.dlwp_conv3x3_hpx_dgrad(L.ptr(d), L.ptr(img_b.t), table.data_ptr(), L.ptr(G.t), L.ptr(g1.t), L.ptr(g2.t) if g2 else None,
                                       B, n, Cout, C1, C2, s))
    L.check(lib.dlwp_conv3x3_wgrad(L.ptr(x1), L.ptr(x2), L.ptr(d), L.ptr(ws.t), L.ptr(gw.t), L.ptr(gb.t), B, n, n, C1, C2, Cout, 2, 2, s))
    torch.cuda.synchronize()
    outs = {"y": y, "g1": g1, "g2": g2, "gw": gw, "gb": gb, "img_f": img_f, "img_b": img_b, "ws": ws, "dz": dz, "G": G}
    for k, o in outs.items():
        assert o is None or o.sentinels_intact(), f"{k}: the floats behind the buffer were written"
    return {k: outs[k].t if outs[k] is not None else None for k in ("y", "g1", "g2", "gw", "gb")}


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: "s{}_f{}_c{}+{}_n{}_{}".format(*CASES[i]))
def test_conv3x3_healpix_forward_and_gradients(cuda, case):
    from dlwp_benchmark_amd import conv_ops, lib as L
    spheres, n, C1, C2, Cout, act = CASES[case]
    B = 12 * spheres
    gen = torch.Generator().manual_seed(3000 + case)
    x = torch.randn(B, C1 + C2, n, n, generator=gen)
    w = torch.randn(Cout, C1 + C2, 3, 3, generator=gen) / (3.0 * (C1 + C2) ** 0.5)
    b = torch.randn(Cout, generator=gen)
    gy = torch.randn(B, Cout, n, n, generator=gen)
    y_ref, gx_ref, gw_ref, gb_ref, S, E = reference(x, w, b, gy, act)
    xcl = cl(x)
    results = []
    for rep in range(2):
        x1 = xcl[..., :C1].contiguous().to(cuda).requires_grad_(True)
        x2 = xcl[..., C1:].contiguous().to(cuda).requires_grad_(True) if C2 else None
        wg, bg = w.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
        with L.kernel_accounting() as acc:
            y = conv_ops.conv3x3(x1, wg, bg, HPX, act, x2=x2)
            y.backward(cl(gy).to(cuda))
            torch.cuda.synchronize()
        results.append(dict(y=y.detach(), g1=x1.grad, g2=x2.grad if C2 else None, gw=wg.grad, gb=bg.grad))
    # ---- which kernels ran
    rows = {r["name"]: r["calls"] for r in acc.rows}
    expect = {"conv3x3_pack": 2, "conv3x3_hpx_n16" if Cout <= 16 else "conv3x3_hpx_n64": 1,
              "conv3x3_hpx_dgrad_n16" if C1 + C2 <= 16 else "conv3x3_hpx_dgrad_n64": 1, "conv3x3_hpx_fold": 1,
              "conv3x3_hpx_wgrad": 1, "conv3x3_wgrad_fold": 1}
    if act:
        expect["conv3x3_act_bwd"] = 1
    assert rows == expect, (rows, expect)
    # ---- repeated launches and the raw entry points (with sentinels): bit-identical
    raw = run_raw(cuda, gen, xcl[..., :C1].contiguous().to(cuda), xcl[..., C1:].contiguous().to(cuda) if C2 else None, w.to(cuda),
                  b.to(cuda), cl(gy).to(cuda), act)
    o = results[0]
    for k, v in o.items():
        if v is not None:
            assert torch.equal(bits(v), bits(results[1][k])), f"{k}: two runs on the same operands differ"
            assert torch.equal(bits(v), bits(raw[k])), f"{k}: autograd and the raw entry points differ"
    # ---- values
    print(CASES[case])
    check("y", o["y"].permute(0, 3, 1, 2), y_ref, S["y"], fn=FN_ULP if act == "tanh" else 0.0)
    gx = gx_ref.permute(0, 2, 3, 1)
    Sx, Ex = S["gx"].permute(0, 2, 3, 1), E["gx"].permute(0, 2, 3, 1)
    check("gx1", o["g1"], gx[..., :C1], Sx[..., :C1], Ex[..., :C1])
    if C2:
        check("gx2", o["g2"], gx[..., C1:], Sx[..., C1:], Ex[..., C1:])
    check("gw", o["gw"], gw_ref, S["gw"], E["gw"])
    check("gb", o["gb"], gb_ref, S["gb"], E["gb"])


def cell_reference(x, hp, cp, w, b, gh, gc):
    """test_gpu_conv_ops.cell_reference with the HEALPix padding"""
    d = lambda t: t.double().requires_grad_(True)      # noqa: E731
    xd, hd, cd, wd, bd = d(x), d(hp), d(cp), d(w), d(b)
    hid = cp.shape[1]
    z = F.conv2d(hpx_pad1(torch.cat([xd, hd], 1)), wd, bd)
    z.retain_grad()
    zi, ii, ff, oo = torch.split(z, hid, dim=1)
    c = torch.sigmoid(ff) * cd + torch.sigmoid(ii) * torch.tanh(zi)
    h = torch.sigmoid(oo) * torch.tanh(c)
    torch.autograd.backward([h, c], [gh.double(), gc.double()])
    xin_a = torch.cat([x, hp], 1).double().abs().requires_grad_(True)
    wa = w.double().abs().requires_grad_(True)
    S_z = F.conv2d(hpx_pad1(xin_a), wa, b.double().abs())
    ref = dict(h=h.detach(), c=c.detach(), gx=xd.grad, ghp=hd.grad, gcp=cd.grad, gw=wd.grad, gb=bd.grad, dz=z.grad, z=z.detach())
    return ref, S_z, xin_a, wa


@pytest.mark.parametrize("with_state", [True, False], ids=["carried_state", "zero_state"])
def test_healpix_cell_matches_the_unfused_definition(cuda, with_state):
    """the published cell width at the published mesh: 57 + 57 -> 4 x 57 channels on 12 faces of 8 x 8"""
    from dlwp_benchmark_amd import conv_ops, lib as L
    hid, B, n = 57, 12, 8
    gen = torch.Generator().manual_seed(4057 + with_state)
    r = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    x, hp, cp = r(B, hid, n, n), torch.tanh(r(B, hid, n, n)), r(B, hid, n, n)
    if not with_state:
        hp, cp = torch.zeros_like(hp), torch.zeros_like(cp)
    w, b = r(4 * hid, 2 * hid, 3, 3) / (2.0 * hid ** 0.5), r(4 * hid)
    gh, gc = r(B, hid, n, n), r(B, hid, n, n)
    ref, S_z, xin_a, wa = cell_reference(x, hp, cp, w, b, gh, gc)
    e_c, e_h, e_gcp, S, E = cell_bounds(ref, S_z, xin_a, wa, cp, gh, gc, hid)
    results = []
    for rep in range(2):
        g = lambda t: t.to(cuda).requires_grad_(True)      # noqa: E731
        X, Wg, Bg = g(cl(x)), g(w), g(b)
        Hp, Cp = (g(cl(hp)), g(cl(cp))) if with_state else (None, None)
        with L.kernel_accounting() as acc:
            h, c = conv_ops.convlstm_cell(X, Hp, Cp, Wg, Bg, HPX)
            torch.autograd.backward([h, c], [cl(gh).to(cuda), cl(gc).to(cuda)])
            torch.cuda.synchronize()
        rows = {r_["name"]: r_["calls"] for r_ in acc.rows}
        assert rows == {"conv3x3_pack": 2, "convlstm_cell_hpx_fwd": 1, "convlstm_gate_bwd": 1, "conv3x3_hpx_dgrad_n64": 1,
                        "conv3x3_hpx_fold": 1, "conv3x3_hpx_wgrad": 1, "conv3x3_wgrad_fold": 1}, rows
        results.append(dict(h=h, c=c, gx=X.grad, ghp=Hp.grad if with_state else None, gcp=Cp.grad if with_state else None, gw=Wg.grad,
                            gb=Bg.grad))
    o = results[0]
    for k, v in o.items():
        assert v is None or torch.equal(bits(v), bits(results[1][k])), f"{k}: two runs on the same operands differ"
    zero = torch.zeros(())
    cf = lambda t: t.permute(0, 3, 1, 2)      # noqa: E731
    check("c", cf(o["c"]), ref["c"], zero, e_c)
    check("h", cf(o["h"]), ref["h"], zero, e_h)
    check("dx", cf(o["gx"]), ref["gx"], S["gin"][:, :hid], E["gin"][:, :hid])
    if with_state:
        check("dc_prev", cf(o["gcp"]), ref["gcp"], zero, e_gcp)
        check("dh_prev", cf(o["ghp"]), ref["ghp"], S["gin"][:, hid:], E["gin"][:, hid:])
    else:
        assert float(o["gw"][:, hid:].abs().max()) == 0.0      # zero state: the recurrent half of the weight gets no gradient
    check("dW", o["gw"], ref["gw"], S["gw"], E["gw"])
    check("db", o["gb"], ref["gb"], S["gb"], E["gb"])


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("face", [0, 4, 9], ids=["north_face", "equatorial_face", "south_face"])
def test_one_hot_output_gradient_gives_the_exact_input_gradient_pattern(cuda, n, face):
    """A one-hot dz at the top-left and at the bottom-right corner pixel of a pole face and of an equatorial face with
    integer-valued weights: every product and sum is exact in fp32, so the input gradient must EQUAL the float64 one -- the
    rotated neighbours, the neighbour read on two sides and the 0.5 entries of the mean-of-two corners included.  A rotation or
    corner mistake fails here by whole weights, not by rounding."""
    from dlwp_benchmark_amd import conv_ops
    w = torch.arange(1.0, 19.0).reshape(1, 2, 3, 3)                 # 2 input channels, 1 output channel, weights 1 .. 18
    for (y, x) in ((0, 0), (n - 1, n - 1)):
        gy = torch.zeros(12, 1, n, n)
        gy[face, 0, y, x] = 1.0
        xd = torch.zeros(12, 2, n, n, dtype=torch.float64, requires_grad=True)
        F.conv2d(hpx_pad1(xd), w.double()).backward(gy.double())
        assert 0.5 in (xd.grad % 1.0) or face != 4                 # the equatorial corners do reach a mean-of-two cell
        xg = torch.zeros(12, n, n, 2, device=cuda, requires_grad=True)
        conv_ops.conv3x3(xg, w.to(cuda), None, HPX).backward(cl(gy).to(cuda))
        got = xg.grad.permute(0, 3, 1, 2).double().cpu()
        assert torch.equal(got, xd.grad), (face, (y, x), (got - xd.grad).abs().max())
