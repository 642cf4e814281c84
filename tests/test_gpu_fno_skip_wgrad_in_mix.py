"""The skip-weight and bias gradients of an FNO block formed by extra workgroups of the per-mode backward launch
(fno_mix_bwd_skipgrad_kernel) instead of by the backward `spatial` launch, which then runs its chain alone.

1. dlwp_fno_block_bwd_slab_split (rows DFT, the hosting per-mode launch, the four-wave chain) against dlwp_fno_block_bwd_slab of
   the same build on the same tensors: g_x, g_wspec and every float of the slab bit for bit, after a plain-store call on a slab
   full of NaN and after a second, accumulating call with another upstream gradient.  The folded gK and bias gradient are held
   to a float64 computation at the bars of tests/test_gpu_fno_spatial_bwd_roles.py: twice the error of the parent commit's
   dlwp_fno_block_bwd_slab on the same seeded inputs (PARENT_ERR, measured on MI355X with the parent's library), never more
   than its GRAD_TOL.  Shapes: one to three channel tiles, ragged and full, B 1 and 3, block input activated and not, on
     16 x 64, modes (12, 12): 84 mode workgroups (not a multiple of 8); more rows than modes at B 3, fewer at B 1
      8 x 32, modes (4, 4):   12 mode workgroups; two 16-pixel chunks, so the partials of waves 2 and 3 are zero
     32 x 64, modes (8, 18):  two table tiles
2. Wide and 3-D plans and the knob FNO_SKIP_WGRAD_IN_MIX = 0 are refused with DLWP_E_UNSUPPORTED, nothing launched, the error
   string untouched; NULL arguments with DLWP_E_INVALID.
3. The rollout trainer with the knob on and off: loss, gradient buffer after the fold, parameters after two Adam steps and
   prediction, with the fused block-0 launch and without it; the live accounting names the launches that ran.  Block 0 takes the
   hosting launch together with its fused launch (whose first phase then runs without role B); with FNO_FUSE_LIFT_BWD = 0 it keeps
   the two-role `spatial` launch, so at n_layers 1 the hosting launch must then not run at all.

Every figure is printed before it is asserted; FNO_SKIPGRAD_REPORT=<file> appends the figures of part 1 as JSON lines.
"""
import ctypes as C
import json
import math
import os

import pytest
import torch

from oracle import fno_ref

GRAD_TOL = 5e-4          # tests/test_gpu_fno_spatial_bwd_roles.py
SENTINEL = 12345.0
POISON = -54321.0
E_INVALID, E_UNSUPPORTED = -1, -3

GRIDS = [(16, 64, (12, 12)), (8, 32, (4, 4)), (32, 64, (8, 18))]
CASES = [(B, Cc, H, W, nm, act) for (H, W, nm) in GRIDS for Cc in (8, 27, 32, 38) for B in (1, 3) for act in (0, 1)]


def case_id(c):
    return "B%d-C%d-%dx%d-m%dx%d-act%d" % (c[0], c[1], c[2], c[3], c[4][0], c[4][1], c[5])


# max-norm relative error against the float64 reference of the PARENT commit's library (dlwp_fno_block_bwd_slab twice +
# dlwp_fno_block_slab_fold), MI355X, the seeded inputs of make_case(), rounded up to three digits: (gk, gb)
PARENT_ERR = {
    "B1-C8-16x64-m12x12-act0": {"gk": 7.86e-08, "gb": 1.55e-07},
    "B1-C8-16x64-m12x12-act1": {"gk": 1.77e-07, "gb": 2.33e-07},
    "B3-C8-16x64-m12x12-act0": {"gk": 1.22e-07, "gb": 3.96e-08},
    "B3-C8-16x64-m12x12-act1": {"gk": 1.32e-07, "gb": 2.01e-07},
    "B1-C27-16x64-m12x12-act0": {"gk": 1.62e-07, "gb": 1.77e-07},
    "B1-C27-16x64-m12x12-act1": {"gk": 1.27e-07, "gb": 1.26e-07},
    "B3-C27-16x64-m12x12-act0": {"gk": 1.39e-07, "gb": 1.34e-07},
    "B3-C27-16x64-m12x12-act1": {"gk": 1.08e-07, "gb": 1.51e-07},
    "B1-C32-16x64-m12x12-act0": {"gk": 1.13e-07, "gb": 2.05e-07},
    "B1-C32-16x64-m12x12-act1": {"gk": 1.38e-07, "gb": 1.53e-07},
    "B3-C32-16x64-m12x12-act0": {"gk": 1.40e-07, "gb": 1.43e-07},
    "B3-C32-16x64-m12x12-act1": {"gk": 1.48e-07, "gb": 1.56e-07},
    "B1-C38-16x64-m12x12-act0": {"gk": 1.35e-07, "gb": 2.21e-07},
    "B1-C38-16x64-m12x12-act1": {"gk": 1.33e-07, "gb": 1.11e-07},
    "B3-C38-16x64-m12x12-act0": {"gk": 1.15e-07, "gb": 2.05e-07},
    "B3-C38-16x64-m12x12-act1": {"gk": 1.52e-07, "gb": 1.64e-07},
    "B1-C8-8x32-m4x4-act0": {"gk": 9.68e-08, "gb": 1.37e-07},
    "B1-C8-8x32-m4x4-act1": {"gk": 1.59e-07, "gb": 8.40e-08},
    "B3-C8-8x32-m4x4-act0": {"gk": 1.89e-07, "gb": 9.03e-08},
    "B3-C8-8x32-m4x4-act1": {"gk": 1.38e-07, "gb": 1.57e-07},
    "B1-C27-8x32-m4x4-act0": {"gk": 1.28e-07, "gb": 9.78e-08},
    "B1-C27-8x32-m4x4-act1": {"gk": 1.87e-07, "gb": 1.47e-07},
    "B3-C27-8x32-m4x4-act0": {"gk": 1.26e-07, "gb": 9.05e-08},
    "B3-C27-8x32-m4x4-act1": {"gk": 1.42e-07, "gb": 1.03e-07},
    "B1-C32-8x32-m4x4-act0": {"gk": 1.26e-07, "gb": 1.37e-07},
    "B1-C32-8x32-m4x4-act1": {"gk": 9.90e-08, "gb": 1.44e-07},
    "B3-C32-8x32-m4x4-act0": {"gk": 1.04e-07, "gb": 1.19e-07},
    "B3-C32-8x32-m4x4-act1": {"gk": 1.22e-07, "gb": 1.21e-07},
    "B1-C38-8x32-m4x4-act0": {"gk": 9.31e-08, "gb": 1.13e-07},
    "B1-C38-8x32-m4x4-act1": {"gk": 1.31e-07, "gb": 1.26e-07},
    "B3-C38-8x32-m4x4-act0": {"gk": 1.30e-07, "gb": 1.32e-07},
    "B3-C38-8x32-m4x4-act1": {"gk": 1.97e-07, "gb": 1.95e-07},
    "B1-C8-32x64-m8x18-act0": {"gk": 8.78e-08, "gb": 9.14e-08},
    "B1-C8-32x64-m8x18-act1": {"gk": 1.04e-07, "gb": 1.79e-07},
    "B3-C8-32x64-m8x18-act0": {"gk": 1.56e-07, "gb": 1.72e-07},
    "B3-C8-32x64-m8x18-act1": {"gk": 1.64e-07, "gb": 1.97e-07},
    "B1-C27-32x64-m8x18-act0": {"gk": 1.19e-07, "gb": 1.39e-07},
    "B1-C27-32x64-m8x18-act1": {"gk": 1.90e-07, "gb": 2.54e-07},
    "B3-C27-32x64-m8x18-act0": {"gk": 1.26e-07, "gb": 2.03e-07},
    "B3-C27-32x64-m8x18-act1": {"gk": 1.84e-07, "gb": 2.34e-07},
    "B1-C32-32x64-m8x18-act0": {"gk": 9.11e-08, "gb": 1.40e-07},
    "B1-C32-32x64-m8x18-act1": {"gk": 1.43e-07, "gb": 1.12e-07},
    "B3-C32-32x64-m8x18-act0": {"gk": 1.44e-07, "gb": 2.27e-07},
    "B3-C32-32x64-m8x18-act1": {"gk": 1.50e-07, "gb": 9.72e-08},
    "B1-C38-32x64-m8x18-act0": {"gk": 1.26e-07, "gb": 1.55e-07},
    "B1-C38-32x64-m8x18-act1": {"gk": 1.46e-07, "gb": 1.73e-07},
    "B3-C38-32x64-m8x18-act0": {"gk": 1.60e-07, "gb": 2.33e-07},
    "B3-C38-32x64-m8x18-act1": {"gk": 1.75e-07, "gb": 1.84e-07},
}


def bar(key, which):
    return min(2.0 * PARENT_ERR[key][which], GRAD_TOL)


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def make_case(B, Cc, H, W, n_modes, act):
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    g = torch.Generator().manual_seed(2203 + 3 * Cc + 11 * B + H + 5 * n_modes[1] + act)
    x = torch.randn(B, Cc, H, W, generator=g)
    wspec = torch.view_as_complex(torch.randn(Cc, Cc, m1, m2c, 2, generator=g) / Cc ** 0.5)
    wskip = torch.randn(Cc, Cc, generator=g) / Cc ** 0.5
    bias = torch.randn(Cc, generator=g) * 0.1
    gpre = torch.randn(B, Cc, H, W, generator=g)
    gpre_b = torch.randn(B, Cc, H, W, generator=g)     # upstream gradient of the second, accumulating call
    return x, wspec, wskip, bias, gpre, gpre_b


def skip_ref64(x, act, gpre):
    """float64: gK[o][i] = sum g_pre[b][o][h][w] a[b][i][h][w] with a = gelu(x) (exact erf) if act else x; gb = sum g_pre"""
    x, gpre = x.double(), gpre.double()
    a = x * 0.5 * (1.0 + torch.erf(x / 2.0 ** 0.5)) if act else x
    return torch.einsum("bohw,bihw->oi", gpre, a), gpre.sum((0, 2, 3))


@pytest.fixture(scope="module")
def L(cuda):
    from dlwp_benchmark_amd import lib
    lib.load()
    return lib


def padded(dev, n, fill):
    """n floats of `fill` in front of a sentinel tail that no kernel may touch (returns the view and the tail)"""
    flat = torch.full((n + 256,), SENTINEL, device=dev)
    flat[:n] = fill
    return flat[:n], flat[n:]


def bits(t):
    return t.contiguous().view(torch.int32)


def run_entry(L, lib, cuda, entry, plan, case, dev):
    """two calls of `entry` (plain store on a NaN slab, then accumulate with the second gradient) and the fold"""
    B, Cc, H, W, n_modes, act = case
    dx, dw, dk, dg, dg_b, xhat, ws = dev
    nslab = lib.dlwp_fno_block_slab_floats(plan, B)
    slab, tail = padded(cuda, nslab, float("nan"))
    gxf, gx_tail = padded(cuda, B * Cc * H * W, POISON)
    gw = torch.zeros_like(dw)
    snaps = []
    for acc, up in ((0, dg), (1, dg_b)):
        L.check(entry(plan, L.ptr(dx), act, L.ptr(dw), L.ptr(dk), L.ptr(up), L.ptr(xhat), gxf.data_ptr(), L.ptr(gw),
                      slab.data_ptr(), acc, B, L.ptr(ws), L.stream()))
        torch.cuda.synchronize()
        snaps.append((gxf.clone(), gw.clone(), slab.clone()))
    gk, gb = torch.zeros(Cc, Cc, device=cuda), torch.zeros(Cc, device=cuda)
    L.check(lib.dlwp_fno_block_slab_fold(plan, slab.data_ptr(), L.ptr(gk), L.ptr(gb), B, L.stream()))
    torch.cuda.synchronize()
    return snaps, gk, gb, (tail, gx_tail)


def setup_case(L, lib, cuda, plan, case):
    B, Cc, H, W, n_modes, act = case
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    x, wspec, wskip, bias, gpre, gpre_b = make_case(*case)
    ws = torch.empty(lib.dlwp_fno_block_workspace_bytes(plan, B), dtype=torch.uint8, device=cuda)
    dx, dk, db, dg, dg_b = [t.to(cuda) for t in (x, wskip, bias, gpre, gpre_b)]
    dw = fno_ref.spec_to_mode_major(wspec).to(cuda)
    pre = torch.empty(B, Cc, H, W, device=cuda)
    xhat = torch.empty(B, m1, m2c, Cc, 2, device=cuda)
    L.check(lib.dlwp_fno_block_fwd(plan, L.ptr(dx), act, L.ptr(dw), L.ptr(dk), L.ptr(db), L.ptr(pre), L.ptr(xhat), B, L.ptr(ws),
                                   L.stream()))
    gk_a, gb_a = skip_ref64(x, act, gpre)
    gk_b, gb_b = skip_ref64(x, act, gpre_b)
    return (dx, dw, dk, dg, dg_b, xhat, ws), gk_a + gk_b, gb_a + gb_b


def report(line):
    print(json.dumps(line))
    path = os.environ.get("FNO_SKIPGRAD_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_split_entry_bit_for_bit_and_float64(L, cuda, case):
    B, Cc, H, W, n_modes, act = case
    key = case_id(case)
    lib = L.load()
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    plan = C.c_void_p()
    L.check(lib.dlwp_fno_plan_create(Cc, H, W, m1, m2c, C.byref(plan)))
    try:
        dev, ref_gk, ref_gb = setup_case(L, lib, cuda, plan, case)
        with L.kernel_accounting() as acc:
            new = run_entry(L, lib, cuda, lib.dlwp_fno_block_bwd_slab_split, plan, case, dev)
        names = {r["name"]: r["calls"] for r in acc.rows}
        old = run_entry(L, lib, cuda, lib.dlwp_fno_block_bwd_slab, plan, case, dev)
    finally:
        lib.dlwp_fno_plan_destroy(plan)
    err = {"gk": rel_err(new[1], ref_gk), "gb": rel_err(new[2], ref_gb)}
    err_old = {"gk": rel_err(old[1], ref_gk), "gb": rel_err(old[2], ref_gb)}
    report({"case": key, "err": err, "err_bwd_slab": err_old,
            "kernels": sorted(n for n in names if n.startswith(("fno_mix", "fno_spatial")))})
    ncb, nbn = (Cc + 15) // 16, (2 * m2c + 15) // 16
    assert names.get("fno_mix_bwd_skipgrad_kernel<true, %d>" % ncb) == 2, names
    assert names.get("fno_spatial_kernel<%d, %d, %d>" % (ncb, nbn, 1 if act else 2)) == 2, names
    assert not any(n.startswith("fno_spatial_roles") for n in names), names
    for tails in (new[3], old[3]):
        for tail in tails:
            assert bool((tail == SENTINEL).all()), "a kernel wrote past the end of the slab or of g_x"
    stride = (Cc * Cc + Cc + 3) // 4 * 4
    for call, (s_new, s_old) in enumerate(zip(new[0], old[0])):
        for name, a, b_ in zip(("g_x", "g_wspec", "slab"), s_new, s_old):
            assert torch.equal(bits(a), bits(b_)), "call %d: not bit for bit dlwp_fno_block_bwd_slab: %s" % (call, name)
        rows = s_new[2].view(B * H, stride)
        assert bool(torch.isfinite(rows[:, :Cc * Cc + Cc]).all()), "call %d: a live slab element was not written" % call
        assert bool(torch.isnan(rows[:, Cc * Cc + Cc:]).all()), "call %d: a padding float of the slab was written" % call
        assert not bool((s_new[0] == POISON).any())
    for which, e in err.items():
        assert e <= GRAD_TOL, (which, e)
        assert e <= bar(key, which), (which, e, PARENT_ERR[key][which])


def poisoned(cuda, *shape):
    n = math.prod(shape)
    buf, tail = padded(cuda, n, POISON)
    return buf.view(*shape), tail


REFUSALS = {"wide-plan-hidden-80": (80, False, None), "plan-3d": (8, True, None), "knob-0": (32, False, 0)}


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(REFUSALS))
def test_refusals(L, cuda, key):
    Cc, three_d, knob = REFUSALS[key]
    lib = L.load()
    B, H, W, T, m1, m2c = 1, 16, 64, 2, 4, 3
    plan = C.c_void_p()
    if three_d:
        L.check(lib.dlwp_fno_plan_create3d(Cc, T, H, W, 2, m1, m2c, C.byref(plan)))
        rows, nm = T * H, 2 * m1
    else:
        L.check(lib.dlwp_fno_plan_create(Cc, H, W, m1, m2c, C.byref(plan)))
        rows, nm = H, m1
    try:
        z = lambda *s: torch.zeros(*s, device=cuda)      # noqa: E731
        ws = torch.empty(lib.dlwp_fno_block_workspace_bytes(plan, B), dtype=torch.uint8, device=cuda)
        outs = [poisoned(cuda, B, Cc, rows, W), poisoned(cuda, nm, m2c, Cc, Cc, 2), poisoned(cuda, B * rows * (Cc * Cc + Cc + 4))]
        g_x, g_wspec, slab = [o[0] for o in outs]
        args = [plan, L.ptr(z(B, Cc, rows, W)), 1, L.ptr(z(nm, m2c, Cc, Cc, 2)), L.ptr(z(Cc, Cc)), L.ptr(z(B, Cc, rows, W)),
                L.ptr(z(B, nm, m2c, Cc, 2)), g_x.data_ptr(), g_wspec.data_ptr(), slab.data_ptr(), 0, B, L.ptr(ws), L.stream()]
        assert lib.dlwp_fno_block_bwd_slab_split(None, *args[1:]) == E_INVALID       # leaves a known error string behind
        before = lib.dlwp_last_error()
        assert b"fno_block_bwd_slab_split" in before
        if knob is not None:
            L.set_tuning("FNO_SKIP_WGRAD_IN_MIX", knob)
        try:
            rc = lib.dlwp_fno_block_bwd_slab_split(*args)
        finally:
            L.set_tuning("FNO_SKIP_WGRAD_IN_MIX", None)
        after = lib.dlwp_last_error()
        torch.cuda.synchronize()
        invalid = []
        for i in (1, 3, 4, 5, 6, 7, 8, 9, 12):       # every pointer argument in turn
            bad = list(args)
            bad[i] = None
            invalid.append(lib.dlwp_fno_block_bwd_slab_split(*bad))
        invalid.append(lib.dlwp_fno_block_bwd_slab_split(*(args[:11] + [0] + args[12:])))      # B = 0
        torch.cuda.synchronize()
    finally:
        lib.dlwp_fno_plan_destroy(plan)
    assert rc == E_UNSUPPORTED, rc
    assert before == after, (before, after)
    assert all(r == E_INVALID for r in invalid), invalid
    for buf, tail in outs:
        assert bool((buf == POISON).all()) and bool((tail == SENTINEL).all())


TRAINER = [(hidden, n_layers, fuse) for hidden in (8, 27) for n_layers in (1, 2) for fuse in (1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,n_layers,fuse", TRAINER, ids=["C%d-L%d-fuse%d" % t for t in TRAINER])
def test_trainer_knob_on_and_off(L, cuda, hidden, n_layers, fuse):
    from dlwp_benchmark_amd import nsbench
    B, T, H, W, ctx = 2, 4, 16, 64, 2
    torch.manual_seed(4099 + hidden + n_layers)
    module = nsbench.TFNO2DModule(n_modes=[12, 12], in_channels=1, hidden_channels=hidden, lifting_channels=32,
                                  projection_channels=32, out_channels=1, n_layers=n_layers, context_size=ctx).to(cuda)
    g = torch.Generator().manual_seed(211)
    x = torch.randn(B, T, 1, H, W, generator=g).to(cuda)
    y = torch.randn(B, T, 1, H, W, generator=g).to(cuda)
    p0 = module.flat_params.data.clone()

    def run(knob):
        L.set_tuning("FNO_SKIP_WGRAD_IN_MIX", knob)
        L.set_tuning("FNO_FUSE_LIFT_BWD", fuse)
        try:
            module.flat_params.data.copy_(p0)
            tr = module.trainer(B, T, H, W, ctx)
            opt = module.make_optimizer(lr=1e-3)
            module.flat_grad.zero_()
            with L.kernel_accounting() as acc:
                loss = module.train_step(x, y, ctx, optimizer=None, use_graph=False)
                torch.cuda.synchronize()
            out = dict(loss=loss.clone(), grad=module.flat_grad.clone(), names={r["name"]: r["calls"] for r in acc.rows})
            module.flat_grad.zero_()
            for _ in range(2):
                module.train_step(x, y, ctx, optimizer=opt, use_graph=False)
            tr.forward(keep_activations=False)       # the evaluation path runs
            torch.cuda.synchronize()
            out.update(params=module.flat_params.data.clone(), pred=tr.out.clone())
            return out
        finally:
            L.set_tuning("FNO_SKIP_WGRAD_IN_MIX", None)
            L.set_tuning("FNO_FUSE_LIFT_BWD", None)

    off_a, off_b, on = run(0), run(0), run(1)
    ncb = (hidden + 15) // 16
    # net calls of the rollout, counted on the knob-0 path: its block-0 backward launch runs once per call
    ncalls = off_a["names"]["fno_spatial_lift_bwd_kernel<%d, 1, 1>" % ncb if fuse else "fno_spatial_roles_kernel<%d, 1, 2>" % ncb]
    assert ncalls >= 2
    host = "fno_mix_bwd_skipgrad_kernel<true, %d>" % ncb
    lift = "fno_spatial_lift_bwd_kernel<%d, 1, 1>" % ncb      # one accounting row for both forms of its first phase
    show = lambda r: {k: v for k, v in r["names"].items() if k.startswith(("fno_mix", "fno_spatial"))}      # noqa: E731
    # the loss is one float atomic per workgroup: its scatter between two runs of one build, and never less than two ulps
    width = max((off_a["loss"] - off_b["loss"]).abs().item(), 2.0 ** -22 * off_a["loss"].abs().item())
    print({"on": show(on), "off": show(off_a), "loss": [r["loss"].item() for r in (off_a, off_b, on)], "width": width})
    # path check.  Blocks l >= 1 always take the hosting launch; block 0 takes it together with its fused launch
    hosted = ncalls * ((n_layers - 1) + (1 if fuse else 0))
    assert on["names"].get(host, 0) == hosted, show(on)
    assert host not in off_a["names"], show(off_a)
    assert on["names"].get(lift, 0) == off_a["names"].get(lift, 0) == (ncalls if fuse else 0), (show(on), show(off_a))
    assert not any(n.startswith("fno_spatial_roles_kernel<%d, 1, 1>" % ncb) for n in on["names"]), show(on)
    if n_layers > 1:
        assert off_a["names"].get("fno_spatial_roles_kernel<%d, 1, 1>" % ncb) == ncalls * (n_layers - 1), show(off_a)
        assert on["names"].get("fno_spatial_kernel<%d, 1, 1>" % ncb) == ncalls * (n_layers - 1), show(on)
    assert bool(on["grad"].abs().max() > 0)
    assert abs(on["loss"].item() - off_a["loss"].item()) <= width, (on["loss"].item(), off_a["loss"].item(), width)
    for name in ("grad", "params", "pred"):
        assert torch.equal(bits(off_a[name]), bits(off_b[name])), "knob 0 does not repeat: " + name
        assert torch.equal(bits(on[name]), bits(off_a[name])), "differs between knob 1 and knob 0: " + name
