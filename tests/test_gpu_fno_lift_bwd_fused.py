"""Block 0's backward `spatial` and the lifting MLP's backward as one launch (fno_spatial_lift_bwd_kernel): the gradient of the
lifting output stays in LDS between the two bodies instead of going through a [B, C, H, W] tensor.

1. dlwp_fno_block_lift_bwd_slab against the two-launch sequence of the same build -- dlwp_fno_block_bwd_slab (act_in = 0) then
   dlwp_pwmlp_bwd_slab on its g_x -- as the rollout trainer runs them: a plain-store call, an accumulating call, the folds; with
   the knob FNO_SKIP_WGRAD_IN_MIX at 1 (the trainer's default block-0 route: hosting per-mode launch, phase 1 without role B)
   and at 0 (plain per-mode launch, role B).
   Both sequences run the same phase text on the same workgroup with the same slabs, so every output is compared bit for bit;
   each is also held to a float64 reference (autograd on the oracle's block and MLP in double) under the 5e-4 of
   tests/test_gpu_fno.py.  Shapes: one channel tile with a ragged hidden width; the headline's channels on a quarter-height
   grid; 27 channels with different mode counts; three channel tiles with two input-channel tiles.
2. The shapes the library keeps on two launches are refused with DLWP_E_UNSUPPORTED.
3. The rollout trainer takes the fused launch by itself and the two launches with the knob FNO_FUSE_LIFT_BWD = 0; gradient
   buffer and prediction are bit for bit equal, and the eager accounting names the kernels that ran.
"""
import ctypes as C

import pytest
import torch

from oracle import fno_ref

GRAD_TOL = 5e-4
SENTINEL = 12345.0
POISON = -54321.0
E_UNSUPPORTED = -3

# (B, C, H, n_modes, Cin, Ch); rows are 64 wide
CASES = [(1, 8, 8, (4, 4), 3, 40), (2, 32, 16, (12, 12), 10, 256), (4, 27, 8, (4, 12), 10, 64), (1, 38, 8, (4, 4), 20, 32)]
W = 64


def case_id(c):
    return "B%d-C%d-%dx64-m%dx%d-Cin%d-Ch%d" % (c[0], c[1], c[2], c[3][0], c[3][1], c[4], c[5])


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def make_case(B, Cc, H, n_modes, Cin, Ch):
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    g = torch.Generator().manual_seed(1307 + 3 * Cc + 11 * B + H + 5 * n_modes[1] + 7 * Cin + Ch)
    t = {}
    t["x"] = torch.randn(B, Cin, H, W, generator=g)
    t["w1"] = torch.randn(Ch, Cin, generator=g) / Cin ** 0.5
    t["b1"] = torch.randn(Ch, generator=g) * 0.1
    t["w2"] = torch.randn(Cc, Ch, generator=g) / Ch ** 0.5
    t["b2"] = torch.randn(Cc, generator=g) * 0.1
    t["wspec"] = torch.view_as_complex(torch.randn(Cc, Cc, m1, m2c, 2, generator=g) / Cc ** 0.5)
    t["wskip"] = torch.randn(Cc, Cc, generator=g) / Cc ** 0.5
    t["bias"] = torch.randn(Cc, generator=g) * 0.1
    t["gpre"] = torch.randn(B, Cc, H, W, generator=g)
    t["gpre_b"] = torch.randn(B, Cc, H, W, generator=g)     # upstream gradient of the second, accumulating call
    return t


def ref64(t, n_modes, gpre):
    """float64 autograd through the oracle: lifting MLP -> block 0 (no activation in front); gradients of <pre, gpre>"""
    leaves = {k: t[k].double().clone().requires_grad_(True) for k in ("x", "w1", "b1", "w2", "b2", "wskip", "bias")}
    wspec = t["wspec"].to(torch.complex128).clone().requires_grad_(True)
    h0 = fno_ref.pw_mlp(leaves["x"], leaves["w1"], leaves["b1"], leaves["w2"], leaves["b2"])
    pre = fno_ref.fno_block(h0, wspec, leaves["wskip"], leaves["bias"], list(n_modes))
    pre.backward(gpre.double())
    return dict(gx=leaves["x"].grad, gw1=leaves["w1"].grad, gb1=leaves["b1"].grad, gw2=leaves["w2"].grad,
                gb2=leaves["b2"].grad, gk=leaves["wskip"].grad, gb=leaves["bias"].grad,
                gwspec=fno_ref.spec_to_mode_major(wspec.grad))


@pytest.fixture(scope="module")
def L(cuda):
    from dlwp_benchmark_amd import lib
    lib.load()
    return lib


def padded(dev, *shape):
    """a buffer of `shape` in front of a sentinel tail that no kernel may touch (returns the view and the tail)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 256,), SENTINEL, device=dev)
    return flat[:n].view(*shape), flat[n:]


def lift_call(L, lib, plan, d, up, xhat, gwspec, slab_skip, gx, slab_lift, acc, B, Cin, Ch, ws):
    return lib.dlwp_fno_block_lift_bwd_slab(plan, L.ptr(d["h0"]), L.ptr(d["wspec"]), L.ptr(d["wskip"]), L.ptr(up), L.ptr(xhat),
                                            L.ptr(gwspec), L.ptr(slab_skip), acc, L.ptr(d["x"]), L.ptr(d["w1"]), L.ptr(d["b1"]),
                                            L.ptr(d["w2"]), gx.data_ptr(), 0, L.ptr(slab_lift), acc, B, Cin, Ch, L.ptr(ws),
                                            L.stream())


NAMES = ("gx", "gw1", "gb1", "gw2", "gb2", "gk", "gb", "gwspec")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_entry_point_against_two_launches(L, cuda, case):
    """Both values of FNO_SKIP_WGRAD_IN_MIX: the entry takes the per-mode form the trainer takes for block 0.  On (the default), the
    launch that hosts the skip-gradient workgroups, followed by the phase-1 form without role B; off, the plain per-mode launch and
    role B.  Every output of either is bit for bit the two launches'."""
    B, Cc, H, n_modes, Cin, Ch = case
    lib = L.load()
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    P = H * W
    t = make_case(*case)
    ref_a, ref_b = ref64(t, n_modes, t["gpre"]), ref64(t, n_modes, t["gpre_b"])
    plan = C.c_void_p()
    L.check(lib.dlwp_fno_plan_create(Cc, H, W, m1, m2c, C.byref(plan)))
    try:
        ws = torch.empty(lib.dlwp_fno_block_workspace_bytes(plan, B), dtype=torch.uint8, device=cuda)
        d = {k: t[k].to(cuda) for k in ("x", "w1", "b1", "w2", "b2", "wskip", "bias", "gpre", "gpre_b")}
        d["wspec"] = fno_ref.spec_to_mode_major(t["wspec"]).to(cuda)
        d["h0"] = torch.empty(B, Cc, H, W, device=cuda)
        L.check(lib.dlwp_pwmlp_fwd(L.ptr(d["x"]), L.ptr(d["w1"]), L.ptr(d["b1"]), L.ptr(d["w2"]), L.ptr(d["b2"]), L.ptr(d["h0"]),
                                   B, Cin, Ch, Cc, P, L.stream()))
        pre = torch.empty(B, Cc, H, W, device=cuda)
        xhat = torch.empty(B, m1, m2c, Cc, 2, device=cuda)
        L.check(lib.dlwp_fno_block_fwd(plan, L.ptr(d["h0"]), 0, L.ptr(d["wspec"]), L.ptr(d["wskip"]), L.ptr(d["bias"]), L.ptr(pre),
                                       L.ptr(xhat), B, L.ptr(ws), L.stream()))

        def run(fused):
            gx, tail = padded(cuda, B, Cin, H, W)
            g_h0 = torch.full((B, Cc, H, W), POISON, device=cuda)      # the tensor the fused launch must never write
            slab_skip = torch.full((lib.dlwp_fno_block_slab_floats(plan, B),), 1e30, device=cuda)   # stale values must not leak
            slab_lift = torch.full((lib.dlwp_pwmlp_slab_floats(B, Cin, Ch, Cc, P),), 1e30, device=cuda)
            gwspec = torch.zeros_like(d["wspec"])
            g = {k: torch.zeros_like(d[k]) for k in ("w1", "b1", "w2", "b2", "wskip", "bias")}
            for acc, up in ((0, d["gpre"]), (1, d["gpre_b"])):
                if fused:
                    L.check(lift_call(L, lib, plan, d, up, xhat, gwspec, slab_skip, gx, slab_lift, acc, B, Cin, Ch, ws))
                else:
                    L.check(lib.dlwp_fno_block_bwd_slab(plan, L.ptr(d["h0"]), 0, L.ptr(d["wspec"]), L.ptr(d["wskip"]), L.ptr(up),
                                                        L.ptr(xhat), L.ptr(g_h0), L.ptr(gwspec), L.ptr(slab_skip), acc, B,
                                                        L.ptr(ws), L.stream()))
                    L.check(lib.dlwp_pwmlp_bwd_slab(L.ptr(d["x"]), L.ptr(d["w1"]), L.ptr(d["b1"]), L.ptr(d["w2"]), L.ptr(g_h0),
                                                    gx.data_ptr(), L.ptr(slab_lift), acc, B, Cin, Ch, Cc, P, L.stream()))
            L.check(lib.dlwp_fno_block_slab_fold(plan, L.ptr(slab_skip), L.ptr(g["wskip"]), L.ptr(g["bias"]), B, L.stream()))
            L.check(lib.dlwp_pwmlp_slab_fold(L.ptr(slab_lift), L.ptr(g["w1"]), L.ptr(g["b1"]), L.ptr(g["w2"]), L.ptr(g["b2"]), B,
                                             Cin, Ch, Cc, P, L.stream()))
            torch.cuda.synchronize()
            return dict(gx=gx, gw1=g["w1"], gb1=g["b1"], gw2=g["w2"], gb2=g["b2"], gk=g["wskip"], gb=g["bias"], gwspec=gwspec), tail, g_h0

        fused = {}
        try:
            for knob in (1, 0):
                L.set_tuning("FNO_SKIP_WGRAD_IN_MIX", knob)
                with L.kernel_accounting() as acc:
                    res = run(True)
                fused[knob] = res + ({r["name"]: r["calls"] for r in acc.rows},)
        finally:
            L.set_tuning("FNO_SKIP_WGRAD_IN_MIX", None)
        two, tail2, g_h0_two = run(False)
    finally:
        lib.dlwp_fno_plan_destroy(plan)

    # float64: gx is the last call's (overwritten), the parameter gradients are the sum of both calls
    ref = {k: (ref_b[k] if k == "gx" else ref_a[k] + ref_b[k]) for k in NAMES}
    nib, ncb, nbn = (Cin + 15) // 16, (Cc + 15) // 16, (2 * m2c + 15) // 16
    assert bool((tail2 == SENTINEL).all()), "a kernel wrote past the end of gx"
    assert not bool((g_h0_two == POISON).any())
    for knob, (got, tail, g_h0, calls) in fused.items():
        names = set(calls)
        err = {k: rel_err(got[k], ref[k]) for k in ref}
        print({"case": case_id(case), "knob": knob, "err": err,
               "kernels": sorted(n for n in names if n.startswith(("fno_mix", "fno_spatial", "pwmlp_bwd")))})
        assert "fno_spatial_lift_bwd_kernel<%d, %d, %d>" % (ncb, nbn, nib) in names, names
        assert not any(n.startswith(("fno_spatial_roles", "pwmlp_bwd")) for n in names), names
        # Which per-mode launch ran.  The hosting launch has an accounting row; the plain fno_mix_bwd launch has none, so that it
        # ran in both calls shows in gwspec, which only a per-mode launch accumulates: it is held to the sum of the two calls below.
        host = "fno_mix_bwd_skipgrad_kernel<true, %d>" % ncb
        mix = {n: c for n, c in calls.items() if n.startswith("fno_mix_bwd")}
        assert mix == ({host: 2} if knob else {}), (knob, mix)
        assert bool((tail == SENTINEL).all()), "a kernel wrote past the end of gx"
        assert bool((g_h0 == POISON).all()), "the fused launch wrote the gradient of the lifting output"
        for k in NAMES:
            assert torch.equal(got[k].view(torch.int32), two[k].view(torch.int32)), "not bit for bit the two launches: " + k
        for k, e in err.items():
            assert e <= GRAD_TOL, (knob, k, e)


@pytest.mark.gpu
@pytest.mark.parametrize("Cc,H,Wd,n_modes", [(8, 8, 32, (4, 4)), (54, 64, 64, (12, 12)), (80, 8, 64, (4, 4))],
                         ids=["rows-32-wide", "C54-64x64", "wide-plan"])
def test_refusals(L, cuda, Cc, H, Wd, n_modes):
    """shapes the trainer keeps on two launches: the entry returns DLWP_E_UNSUPPORTED (and launches nothing)"""
    lib = L.load()
    B, Cin, Ch = 1, 3, 16
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    plan = C.c_void_p()
    L.check(lib.dlwp_fno_plan_create(Cc, H, Wd, m1, m2c, C.byref(plan)))
    try:
        z = lambda *s: torch.zeros(*s, device=cuda)
        ws = torch.empty(lib.dlwp_fno_block_workspace_bytes(plan, B), dtype=torch.uint8, device=cuda)
        gx, tail = padded(cuda, B, Cin, H, Wd)
        gx.fill_(POISON)
        slab_lift = z(lib.dlwp_pwmlp_slab_floats(B, Cin, Ch, Cc, H * Wd))
        slab_skip = z(B * H * ((Cc * Cc + Cc + 3) // 4 * 4))
        rc = lib.dlwp_fno_block_lift_bwd_slab(plan, L.ptr(z(B, Cc, H, Wd)), L.ptr(z(m1, m2c, Cc, Cc, 2)), L.ptr(z(Cc, Cc)),
                                              L.ptr(z(B, Cc, H, Wd)), L.ptr(z(B, m1, m2c, Cc, 2)), L.ptr(z(m1, m2c, Cc, Cc, 2)),
                                              L.ptr(slab_skip), 0, L.ptr(z(B, Cin, H, Wd)), L.ptr(z(Ch, Cin)), L.ptr(z(Ch)),
                                              L.ptr(z(Cc, Ch)), gx.data_ptr(), 0, L.ptr(slab_lift), 0, B, Cin, Ch, L.ptr(ws),
                                              L.stream())
        torch.cuda.synchronize()
    finally:
        lib.dlwp_fno_plan_destroy(plan)
    assert rc == E_UNSUPPORTED, rc
    assert bool((gx == POISON).all()) and bool((tail == SENTINEL).all())


@pytest.mark.gpu
def test_trainer_takes_the_fused_launch(L, cuda):
    from dlwp_benchmark_amd import nsbench
    module = nsbench.TFNO2DModule(n_modes=[8, 12], in_channels=1, hidden_channels=32, lifting_channels=64,
                                  projection_channels=64, out_channels=1, n_layers=2, context_size=10).to(cuda)
    g = torch.Generator().manual_seed(97)
    x = torch.randn(2, 13, 1, 16, 64, generator=g).to(cuda)
    y = torch.randn(2, 13, 1, 16, 64, generator=g).to(cuda)

    def step():
        tr = module.trainer(2, 13, 16, 64, 10)
        module.flat_grad.zero_()
        with L.kernel_accounting() as acc:
            module.train_step(x, y, 10, optimizer=None, use_graph=False)
            torch.cuda.synchronize()
        return module.flat_grad.clone(), tr.out.clone(), {r["name"] for r in acc.rows}

    fused, old = "fno_spatial_lift_bwd_kernel<2, 1, 1>", ("fno_spatial_roles_kernel<2, 1, 2>", "pwmlp_bwd_kernel<1, 2, 8>")
    L.set_tuning("FNO_FUSE_LIFT_BWD", None)
    try:
        grad_f, out_f, names_f = step()
        L.set_tuning("FNO_FUSE_LIFT_BWD", 0)
        grad_2, out_2, names_2 = step()
    finally:
        L.set_tuning("FNO_FUSE_LIFT_BWD", None)
    print(sorted(names_f), sorted(names_2))
    assert fused in names_f and not any(n in names_f for n in old), names_f
    assert fused not in names_2 and all(n in names_2 for n in old), names_2
    assert bool(grad_f.abs().max() > 0)
    assert torch.equal(grad_f.view(torch.int32), grad_2.view(torch.int32)), "gradient buffer differs between the two dispatches"
    assert torch.equal(out_f.view(torch.int32), out_2.view(torch.int32)), "prediction differs between the two dispatches"
