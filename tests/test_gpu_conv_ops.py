"""The 3 x 3 convolution kernels (csrc/conv3x3.hip) against float64 torch on the CPU, element by element.

Reference: `F.conv2d` (and its autograd) on float64 copies of the operands, after an explicit one-pixel padding per axis.

Bound, per element, EVERY element compared:  |err| <= 1e-6 * S + ulp(result) [+ 4.8e-7 behind tanh / sigmoid] [+ carried error]
* S = sum |a| |b| over that element's products: the same convolution (or its autograd) of the absolute values, in float64.
  1e-6: a plain sequential fp32 multiply-add chain stays below 3.3e-7 * S for zero-mean operands at every K from 9 to 12 288
  and the fp32 MFMA chain is documented at 3.5e-7 * S at K = 4096; three times that.  Operands are zero-mean (randn).
* ulp(result): one fp32 spacing at the reference value (the final rounding).
* 4.8e-7 (4 ulp at 1.0): the evaluation of tanh / the logistic function itself, the order the device math library documents.
* carried error: a gradient is a product with dz = gy * act'(y), and the kernel forms dz from ITS OWN y.  With e_y the forward
  bound of that element, |delta dz| <= |gy| (2 |y| e_y + e_y^2) for tanh and |gy| where |pre-activation| <= e_y for relu
  (the mask may legitimately differ there), plus three ulp of dz for tanh (the roundings of y^2, 1 - y^2 and the product); this is pushed through the same products (sum |delta dz| |b|).
  For the cell the analogous first-order propagation is written out at `cell_bounds`.
Sentinel floats after every output buffer must come back bit for bit; the kernels that ran are read from
lib.kernel_accounting(); every launch is repeated on the same operands and must be bit-identical (the weight gradient folds its
per-workgroup partial sums in a fixed order: no atomics).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from convlstm_ref import pad1

pytestmark = pytest.mark.gpu

SENT = 64
FN_ULP = 4.8e-7
Z, C_ = "zeros", "circular"
PADC = {Z: 0, C_: 1}
ACTC = {None: 0, "tanh": 1, "relu": 2}

# (B, H, W, C1, C2, Cout, pad_h, pad_w, act): every channel count of {1, 4, 5, 13, 16, 57, 114, 162, 228, 324} as input and as
# output width, every grid of {8x8, 16x24, 32x64, 64x64, 33x47}, B in {1, 3}, the four padding pairs, the three activations,
# one and two input tensors, both column-tile paths (n16: <= 16 output columns, n64 otherwise) for forward and input gradient
CASES = [
    (1, 8, 8, 1, 0, 5, C_, C_, None),
    (3, 8, 8, 5, 0, 1, Z, Z, "tanh"),
    (1, 16, 24, 4, 0, 13, Z, C_, "relu"),
    (3, 16, 24, 13, 13, 4, C_, Z, None),
    (1, 33, 47, 16, 0, 16, C_, C_, "tanh"),
    (3, 33, 47, 5, 4, 57, Z, C_, None),
    (1, 32, 64, 57, 57, 228, C_, C_, None),
    (1, 64, 64, 114, 0, 57, Z, Z, "relu"),
    (3, 32, 64, 57, 0, 114, C_, Z, "tanh"),
    (1, 32, 64, 162, 162, 162, Z, C_, None),
    (1, 16, 24, 324, 0, 324, C_, C_, "tanh"),
    (1, 64, 64, 228, 0, 16, Z, C_, None),
    (3, 64, 64, 16, 1, 162, C_, C_, "relu"),
    (1, 33, 47, 1, 0, 1, C_, Z, None),
]


def ulp32(ref):
    return torch.from_numpy(np.spacing(np.abs(ref.float().numpy()))).double()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def check(what, got, ref, S, extra=None, fn=0.0):
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = 1e-6 * S + ulp32(ref) + fn + (extra if extra is not None else 0.0)
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), what
    print(f"  {what}: max |err| {err.max():.3e}, worst err / bound {float((err / bound).max()):.3f} over {err.numel()} elements")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound, worst ratio {float((err / bound).max()):.3f}"
    return bound


class Out:
    """an output buffer with SENT sentinel floats behind it"""

    def __init__(self, shape, dev, gen, zero=False):
        n = int(np.prod(shape))
        self.flat = torch.randn(n + SENT, generator=gen).to(dev)
        if zero:
            self.flat[:n] = 0
        self.before = self.flat[n:].clone()
        self.t, self.n = self.flat[:n].view(shape), n

    def sentinels_intact(self):
        return torch.equal(bits(self.flat[self.n:]), bits(self.before))


def cl(t):
    """channels-first float64 CPU -> channels-last fp32 (CPU)"""
    return t.detach().permute(0, 2, 3, 1).float().contiguous()


def reference(x, w, b, gy, pads, act):
    """float64 forward + autograd of act(conv(pad(x), w) + b), the same graph on absolute values (S) and with the carried
    dz error as the upstream gradient (E)."""
    xd, wd, bd = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv2d(pad1(xd, pads), wd, bd)
    y = torch.tanh(pre) if act == "tanh" else (torch.relu(pre) if act == "relu" else pre)
    y.backward(gy.double())
    xa, wa = x.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True)
    S_y = F.conv2d(pad1(xa, pads), wa, b.double().abs())
    e_y = 1e-6 * S_y.detach() + ulp32(pre.detach())                       # forward bound of the pre-activation
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


def run_kernels(dev, gen, x1, x2, w, b, gy_cl, pads, act):
    """pack, forward, (activation backward,) input gradient, weight gradient through the raw entry points"""
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    B, H, W_, C1 = x1.shape
    C2 = x2.shape[-1] if x2 is not None else 0
    Cout = w.shape[0]
    ph, pw, a = PADC[pads[0]], PADC[pads[1]], ACTC[act]
    img_f = Out((lib.dlwp_conv3x3_image_floats(C1 + C2, Cout, 0),), dev, gen)
    img_b = Out((lib.dlwp_conv3x3_image_floats(C1 + C2, Cout, 2),), dev, gen)
    y = Out((B, H, W_, Cout), dev, gen)
    g1 = Out((B, H, W_, C1), dev, gen)
    g2 = Out((B, H, W_, C2), dev, gen) if C2 else None
    dz = Out((B, H, W_, Cout), dev, gen) if a else None
    gw, gb = Out(tuple(w.shape), dev, gen, zero=True), Out((Cout,), dev, gen, zero=True)
    ws = Out((lib.dlwp_conv3x3_wgrad_ws_floats(B, H, W_, C1 + C2, Cout),), dev, gen)
    s = L.stream()
    L.check(lib.dlwp_conv3x3_pack(L.ptr(w), L.ptr(img_f.t), C1 + C2, Cout, 0, s))
    L.check(lib.dlwp_conv3x3_pack(L.ptr(w), L.ptr(img_b.t), C1 + C2, Cout, 2, s))
    L.check(lib.dlwp_conv3x3_fwd(L.ptr(x1), L.ptr(x2), L.ptr(img_f.t), L.ptr(b), L.ptr(y.t), None, B, H, W_, C1, C2, Cout, 0, ph, pw, a, s))
    d = gy_cl
    if a:
        L.check(lib.dlwp_conv3x3_act_bwd(L.ptr(y.t), L.ptr(gy_cl), L.ptr(dz.t), gy_cl.numel(), a, s))
        d = dz.t
    L.check(lib.dlwp_conv3x3_fwd(L.ptr(d), None, L.ptr(img_b.t), None, L.ptr(g1.t), L.ptr(g2.t) if g2 else None, B, H, W_, Cout, 0, C1, C2,
                                 ph, pw, 0, s))
    L.check(lib.dlwp_conv3x3_wgrad(L.ptr(x1), L.ptr(x2), L.ptr(d), L.ptr(ws.t), L.ptr(gw.t), L.ptr(gb.t), B, H, W_, C1, C2, Cout, ph, pw, s))
    torch.cuda.synchronize()
    outs = {"y": y, "g1": g1, "g2": g2, "gw": gw, "gb": gb, "img_f": img_f, "img_b": img_b, "ws": ws, "dz": dz}
    for k, o in outs.items():
        assert o is None or o.sentinels_intact(), f"{k}: the floats behind the buffer were written"
    return outs


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: "B{}_{}x{}_c{}+{}_n{}_{}_{}_{}".format(*CASES[i]))
def test_conv3x3_forward_and_gradients(cuda, case):
    from dlwp_benchmark_amd import lib as L
    B, H, W_, C1, C2, Cout, ph, pw, act = CASES[case]
    pads = (ph, pw)
    gen = torch.Generator().manual_seed(1000 + case)
    x = torch.randn(B, C1 + C2, H, W_, generator=gen)
    w = torch.randn(Cout, C1 + C2, 3, 3, generator=gen) / (3.0 * (C1 + C2) ** 0.5)
    b = torch.randn(Cout, generator=gen)
    gy = torch.randn(B, Cout, H, W_, generator=gen)
    y_ref, gx_ref, gw_ref, gb_ref, S, E = reference(x, w, b, gy, pads, act)
    xcl = cl(x)
    x1 = xcl[..., :C1].contiguous().to(cuda)
    x2 = xcl[..., C1:].contiguous().to(cuda) if C2 else None
    wg, bg, gy_cl = w.to(cuda), b.to(cuda), cl(gy).to(cuda)
    with L.kernel_accounting() as acc:
        o = run_kernels(cuda, gen, x1, x2, wg, bg, gy_cl, pads, act)
    # ---- which kernels ran
    rows = {r["name"]: r["calls"] for r in acc.rows}
    fwd_name = "conv3x3_n16" if Cout <= 16 else "conv3x3_n64"
    bwd_name = "conv3x3_n16" if C1 + C2 <= 16 else "conv3x3_n64"
    expect = {"conv3x3_pack": 2, "conv3x3_wgrad": 1, "conv3x3_wgrad_fold": 1}
    expect[fwd_name] = expect.get(fwd_name, 0) + 1
    expect[bwd_name] = expect.get(bwd_name, 0) + 1
    if act:
        expect["conv3x3_act_bwd"] = 1
    assert rows == expect, (rows, expect)
    # ---- values
    print(CASES[case])
    fn = FN_ULP if act == "tanh" else 0.0
    check("y", o["y"].t.permute(0, 3, 1, 2), y_ref, S["y"], fn=fn)
    gx = gx_ref.permute(0, 2, 3, 1)
    Sx, Ex = S["gx"].permute(0, 2, 3, 1), E["gx"].permute(0, 2, 3, 1)
    check("gx1", o["g1"].t, gx[..., :C1], Sx[..., :C1], Ex[..., :C1])
    if C2:
        check("gx2", o["g2"].t, gx[..., C1:], Sx[..., C1:], Ex[..., C1:])
    check("gw", o["gw"].t, gw_ref, S["gw"], E["gw"])
    check("gb", o["gb"].t, gb_ref, S["gb"], E["gb"])
    # ---- the same launches again: bit-identical
    o2 = run_kernels(cuda, gen, x1, x2, wg, bg, gy_cl, pads, act)
    for k in ("y", "g1", "g2", "gw", "gb"):
        if o[k] is not None:
            assert torch.equal(bits(o[k].t), bits(o2[k].t)), f"{k}: two launches on the same operands differ"
    # ---- accumulation: a second weight-gradient launch into the same buffers doubles them (x + x is exact)
    lib = L.load()
    d = o["dz"].t if act else gy_cl
    L.check(lib.dlwp_conv3x3_wgrad(L.ptr(x1), L.ptr(x2), L.ptr(d), L.ptr(o["ws"].t), L.ptr(o["gw"].t), L.ptr(o["gb"].t), B, H, W_, C1, C2,
                                   Cout, PADC[ph], PADC[pw], L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(o["gw"].t), bits(2 * o2["gw"].t)) and torch.equal(bits(o["gb"].t), bits(2 * o2["gb"].t))


def cell_reference(x, hp, cp, w, b, gh, gc, pads):
    """the UNFUSED definition in float64 (conv -> split -> activations -> update) with its autograd, S and carried-error terms"""
    d = lambda t: t.double().requires_grad_(True)      # noqa: E731
    xd, hd, cd, wd, bd = d(x), d(hp), d(cp), d(w), d(b)
    hid = cp.shape[1]
    z = F.conv2d(pad1(torch.cat([xd, hd], 1), pads), wd, bd)
    z.retain_grad()
    zi, ii, ff, oo = torch.split(z, hid, dim=1)
    c = torch.sigmoid(ff) * cd + torch.sigmoid(ii) * torch.tanh(zi)
    h = torch.sigmoid(oo) * torch.tanh(c)
    torch.autograd.backward([h, c], [gh.double(), gc.double()])
    xin_a = torch.cat([x, hp], 1).double().abs().requires_grad_(True)
    wa = w.double().abs().requires_grad_(True)
    S_z = F.conv2d(pad1(xin_a, pads), wa, b.double().abs())
    ref = dict(h=h.detach(), c=c.detach(), gx=xd.grad, ghp=hd.grad, gcp=cd.grad, gw=wd.grad, gb=bd.grad, dz=z.grad, z=z.detach())
    return ref, S_z, xin_a, wa


def cell_bounds(ref, S_z, xin_a, wa, cp, gh, gc, hid):
    """First-order propagation of the pre-activation bound e_z = 1e-6 S_z + ulp(z) through the cell.
    Gates: tanh and the logistic function are 1-Lipschitz, so |delta gate| <= e_z + 4.8e-7 =: e_q; delta := the largest e_q of
    the four gates of a hidden channel.  c = f c_prev + i g with |i|, |g| <= 1: |delta c| <= |c_prev| delta + 2 delta + 2 ulp(c).
    h = o tanh(c): |delta h| <= delta + |delta c| + 4.8e-7 + ulp(h).
    Backward (gate kernel): dc = gc + gh o (1 - tc^2), tc = tanh(c) with |delta tc| <= |delta c| + 4.8e-7 =: e_t; every dz_q is dc
    or gh times a polynomial P_q of the stored gates with |P_q| <= m := max(1, |c_prev|) and a gradient 1-norm <= 3 m, and
    |delta dc| <= 3 |gh| e_t.  Hence |delta dz_q| <= 3 m (|dc| + |gh|) e_t + 4 ulp(dz_q) (e_t >= delta), and
    |delta dc_prev| = |delta (dc f)| <= (|dc| + 3 |gh|) e_t + ulp.  These carried errors go through the products like dz itself."""
    z = ref["z"]
    e_q = 1e-6 * S_z.detach() + ulp32(z) + FN_ULP
    delta = torch.stack(torch.split(e_q, hid, dim=1)).max(dim=0).values
    cpd, ghd, gcd = cp.double(), gh.double(), gc.double()
    e_c = cpd.abs() * delta + 2 * delta + 2 * ulp32(ref["c"])
    e_h = delta + e_c + FN_ULP + ulp32(ref["h"])
    e_t = e_c + FN_ULP
    oo = torch.sigmoid(torch.split(z, hid, dim=1)[3])
    tc = torch.tanh(ref["c"])
    dc = gcd + ghd * oo * (1 - tc ** 2)
    m = cpd.abs().clamp_min(1.0)
    dz_err = (3 * m * (dc.abs() + ghd.abs()) * e_t).repeat(1, 4, 1, 1) + 4 * ulp32(ref["dz"])
    e_gcp = (dc.abs() + 3 * ghd.abs()) * e_t
    S_z.backward(ref["dz"].abs(), retain_graph=True)
    S = {"gin": xin_a.grad.clone(), "gw": wa.grad.clone(), "gb": ref["dz"].abs().sum(dim=(0, 2, 3))}
    xin_a.grad, wa.grad = None, None
    S_z.backward(dz_err)
    E = {"gin": xin_a.grad, "gw": wa.grad, "gb": dz_err.sum(dim=(0, 2, 3))}
    return e_c, e_h, e_gcp, S, E


@pytest.mark.parametrize("hid,B,H,W_,pads", [(5, 1, 8, 8, (C_, C_)), (16, 3, 16, 24, (Z, C_)), (57, 1, 33, 47, (C_, C_))])
def test_fused_cell_matches_the_unfused_definition(cuda, hid, B, H, W_, pads):
    from dlwp_benchmark_amd import conv_ops, lib as L
    gen = torch.Generator().manual_seed(77 + hid)
    r = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    x, hp, cp = r(B, hid, H, W_), torch.tanh(r(B, hid, H, W_)), r(B, hid, H, W_)
    w, b = r(4 * hid, 2 * hid, 3, 3) / (2.0 * hid ** 0.5), r(4 * hid)
    gh, gc = r(B, hid, H, W_), r(B, hid, H, W_)
    ref, S_z, xin_a, wa = cell_reference(x, hp, cp, w, b, gh, gc, pads)
    e_c, e_h, e_gcp, S, E = cell_bounds(ref, S_z, xin_a, wa, cp, gh, gc, hid)
    results = []
    for rep in range(2):
        g = lambda t: t.to(cuda).requires_grad_(True)      # noqa: E731
        X, Hp, Cp, Wg, Bg = g(cl(x)), g(cl(hp)), g(cl(cp)), g(w), g(b)
        with L.kernel_accounting() as acc:
            h, c = conv_ops.convlstm_cell(X, Hp, Cp, Wg, Bg, pads)
            torch.autograd.backward([h, c], [cl(gh).to(cuda), cl(gc).to(cuda)])
            torch.cuda.synchronize()
        rows = {r_["name"]: r_["calls"] for r_ in acc.rows}
        assert rows == {"conv3x3_pack": 2, "convlstm_cell_fwd": 1, "convlstm_gate_bwd": 1, "conv3x3_n64" if 2 * hid > 16 else "conv3x3_n16": 1,
                        "conv3x3_wgrad": 1, "conv3x3_wgrad_fold": 1}, rows
        results.append(dict(h=h, c=c, gx=X.grad, ghp=Hp.grad, gcp=Cp.grad, gw=Wg.grad, gb=Bg.grad))
    o = results[0]
    for k in o:
        assert torch.equal(bits(o[k]), bits(results[1][k])), f"{k}: two runs on the same operands differ"
    zero = torch.zeros(())
    cf = lambda t: t.permute(0, 3, 1, 2)      # noqa: E731
    check("c", cf(o["c"]), ref["c"], zero, e_c)
    check("h", cf(o["h"]), ref["h"], zero, e_h)
    check("dc_prev", cf(o["gcp"]), ref["gcp"], zero, e_gcp)
    check("dx", cf(o["gx"]), ref["gx"], S["gin"][:, :hid], E["gin"][:, :hid])
    check("dh_prev", cf(o["ghp"]), ref["ghp"], S["gin"][:, hid:], E["gin"][:, hid:])
    check("dW", o["gw"], ref["gw"], S["gw"], E["gw"])
    check("db", o["gb"], ref["gb"], S["gb"], E["gb"])


def test_zero_state_cell_equals_explicit_zero_states(cuda):
    """h_prev = c_prev = None (the first step of a rollout) skips the recurrent half of the product: same h, c bit for bit"""
    from dlwp_benchmark_amd import conv_ops
    gen = torch.Generator().manual_seed(5)
    hid = 13
    x = torch.randn(2, 16, 24, hid, generator=gen).to(cuda)
    w = (torch.randn(4 * hid, 2 * hid, 3, 3, generator=gen) * 0.2).to(cuda)
    b = torch.randn(4 * hid, generator=gen).to(cuda)
    zeros = torch.zeros_like(x)
    with torch.no_grad():
        h0, c0 = conv_ops.convlstm_cell(x, None, None, w, b, "circular")
        h1, c1 = conv_ops.convlstm_cell(x, zeros, zeros, w, b, "circular")
    assert torch.equal(bits(h0), bits(h1)) and torch.equal(bits(c0), bits(c1))


@pytest.mark.parametrize("hid,B,H,W_,pads", [(5, 1, 8, 8, (C_, C_)), (16, 3, 16, 24, (Z, C_)), (57, 1, 33, 47, (C_, C_))])
def test_cell_backward_kernels_on_their_own_inputs(cuda, hid, B, H, W_, pads):
    """The chained bound of the test above is a worst-case sum and therefore loose for the backward pass; here every backward
    kernel of the cell is held to float64 ON THE INPUTS IT ACTUALLY READ (the gates and c the forward kernel stored, the dz the
    gate kernel wrote), through the raw entry points with sentinels behind every buffer:
    * stored gates: 1e-6 S_z + ulp + 4.8e-7 against the unfused float64 gates;
    * gate backward: dz and dc_prev are sums of products of at most eight fp32 operations on factors bounded by 1 and
      m = max(1, |c_prev|), with tanh(c) evaluated to 4.8e-7: |err| <= (|dc_in| + |dh|) m (2 * 4.8e-7 + 16 * 2^-24);
    * input and weight gradient from that dz: the convolution bound 1e-6 S + ulp."""
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    gen = torch.Generator().manual_seed(177 + hid)
    r = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    x, hp, cp = r(B, hid, H, W_), torch.tanh(r(B, hid, H, W_)), r(B, hid, H, W_)
    w, b = r(4 * hid, 2 * hid, 3, 3) / (2.0 * hid ** 0.5), r(4 * hid)
    gh, gc = r(B, hid, H, W_), r(B, hid, H, W_)
    ph, pw = PADC[pads[0]], PADC[pads[1]]
    X, Hp, Cp, Gh, Gc = (cl(t).to(cuda) for t in (x, hp, cp, gh, gc))
    Wg, Bg = w.to(cuda), b.to(cuda)
    img_f = Out((lib.dlwp_conv3x3_image_floats(2 * hid, 4 * hid, 1),), cuda, gen)
    img_b = Out((lib.dlwp_conv3x3_image_floats(2 * hid, 4 * hid, 2),), cuda, gen)
    shp = (B, H, W_, hid)
    h, c, gates = Out(shp, cuda, gen), Out(shp, cuda, gen), Out((B, H, W_, 4 * hid), cuda, gen)
    dz, dcp, gx, ghp = Out((B, H, W_, 4 * hid), cuda, gen), Out(shp, cuda, gen), Out(shp, cuda, gen), Out(shp, cuda, gen)
    gw, gb = Out(tuple(w.shape), cuda, gen, zero=True), Out((4 * hid,), cuda, gen, zero=True)
    ws = Out((lib.dlwp_conv3x3_wgrad_ws_floats(B, H, W_, 2 * hid, 4 * hid),), cuda, gen)
    s = L.stream()
    L.check(lib.dlwp_conv3x3_pack(L.ptr(Wg), L.ptr(img_f.t), 2 * hid, 4 * hid, 1, s))
    L.check(lib.dlwp_conv3x3_pack(L.ptr(Wg), L.ptr(img_b.t), 2 * hid, 4 * hid, 2, s))
    L.check(lib.dlwp_convlstm_cell_fwd(L.ptr(X), L.ptr(Hp), L.ptr(img_f.t), L.ptr(Bg), L.ptr(Cp), L.ptr(h.t), L.ptr(c.t), L.ptr(gates.t),
                                       B, H, W_, hid, hid, ph, pw, s))
    L.check(lib.dlwp_convlstm_gate_bwd(L.ptr(Gh), L.ptr(Gc), L.ptr(gates.t), L.ptr(Cp), L.ptr(c.t), L.ptr(dz.t), L.ptr(dcp.t), B * H * W_,
                                       hid, s))
    L.check(lib.dlwp_conv3x3_fwd(L.ptr(dz.t), None, L.ptr(img_b.t), None, L.ptr(gx.t), L.ptr(ghp.t), B, H, W_, 4 * hid, 0, hid, hid, ph, pw,
                                 0, s))
    L.check(lib.dlwp_conv3x3_wgrad(L.ptr(X), L.ptr(Hp), L.ptr(dz.t), L.ptr(ws.t), L.ptr(gw.t), L.ptr(gb.t), B, H, W_, hid, hid, 4 * hid, ph,
                                   pw, s))
    torch.cuda.synchronize()
    for name, o in dict(img_f=img_f, img_b=img_b, h=h, c=c, gates=gates, dz=dz, dcp=dcp, gx=gx, ghp=ghp, gw=gw, gb=gb, ws=ws).items():
        assert o.sentinels_intact(), f"{name}: the floats behind the buffer were written"
    cf = lambda t: t.permute(0, 3, 1, 2).double().cpu()      # noqa: E731
    zero = torch.zeros(())
    # ---- stored gates against the unfused float64 definition
    xin = torch.cat([x, hp], 1).double()
    z = F.conv2d(pad1(xin, pads), w.double(), b.double())
    S_z = F.conv2d(pad1(xin.abs(), pads), w.double().abs(), b.double().abs())
    zi, ii, ff, oo = torch.split(z, hid, dim=1)
    g_ref = torch.cat([torch.tanh(zi), torch.sigmoid(ii), torch.sigmoid(ff), torch.sigmoid(oo)], 1)
    check("gates", cf(gates.t), g_ref, zero, 1e-6 * S_z + ulp32(z) + FN_ULP)
    # ---- gate backward in float64 on the stored gates and c
    G, Cg = cf(gates.t), cf(c.t)
    gi, ig, fg, og = torch.split(G, hid, dim=1)
    tc = torch.tanh(Cg)
    ghd, gcd, cpd = gh.double(), gc.double(), cp.double()
    dc = gcd + ghd * og * (1 - tc ** 2)
    dz_ref = torch.cat([dc * ig * (1 - gi ** 2), dc * gi * ig * (1 - ig), dc * cpd * fg * (1 - fg), ghd * tc * og * (1 - og)], 1)
    e = (gcd.abs() + ghd.abs()) * cpd.abs().clamp_min(1.0) * (2 * FN_ULP + 16 * 2.0 ** -24)
    check("dz", cf(dz.t), dz_ref, zero, e.repeat(1, 4, 1, 1))
    check("dc_prev", cf(dcp.t), dc * fg, zero, e)
    # ---- the two products on the dz the gate kernel wrote
    dzg = cf(dz.t)
    xa, wa = xin.abs().requires_grad_(True), w.double().abs().requires_grad_(True)
    F.conv2d(pad1(xa, pads), wa).backward(dzg.abs())
    xr, wr = xin.clone().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(pad1(xr, pads), wr).backward(dzg)
    check("dx", cf(gx.t), xr.grad[:, :hid], xa.grad[:, :hid])
    check("dh_prev", cf(ghp.t), xr.grad[:, hid:], xa.grad[:, hid:])
    check("dW", gw.t, wr.grad, wa.grad)
    check("db", gb.t, dzg.sum(dim=(0, 2, 3)), dzg.abs().sum(dim=(0, 2, 3)))
