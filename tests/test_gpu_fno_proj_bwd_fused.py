"""The previous net call's projection backward as the third phase of block 0's fused backward launch
(fno_spatial_lift_proj_bwd_kernel, accounting row fno_spatial_lift_bwd_kernel<N, M, I>): in the rollout's backward chain the
launch behind block 0 of call k is the scalar-output projection backward of call k - 1 on the same 64-pixel rows, and all it needs
from that launch is its own rows of the closed-loop gradient.

1. dlwp_fno_block_lift_proj_bwd_slab against the two launches of the same build -- dlwp_fno_block_lift_bwd_slab, then
   dlwp_pwmlp_proj_bwd_rows_slab -- on the same tensors, as the trainer runs them: the lifting gradient accumulates into a tensor
   that already holds a gradient, and one plane of that tensor is the projection's upstream gradient (plus the MSE term).  A
   plain-store call on NaN-filled slabs, then an accumulating call; with FNO_SKIP_WGRAD_IN_MIX at 1 and at 0 (phase 1 without and
   with role B).  Both forms run the same text on the same workgroup, so everything is compared bit for bit: gcur, x1, the tensor
   the lifting gradient accumulates into, every float of the two MLP slabs after each call, the skip slab and g_wspec.
2. The projection phase against float64 (autograd through oracle.fno_ref.pw_mlp in double, upstream = the float32 plane the launch
   read + mse_scale * (pred - target)): relative max-norm error of gcur and of the folded parameter gradients at most twice the
   error of the parent commit's library on the same inputs, case by case, never more than 5e-4.  PARENT_ERR below was measured on
   an MI355X with the parent's build by tools/measure_proj_bwd_parent_err.py: its dlwp_fno_block_lift_bwd_slab, then its
   dlwp_pwmlp_bwd_rows_ex with pred and target (the routine its trainer calls: the MSE term is added in the kernel), then the fold.
   x1 has no bound of its own: it is bit for bit the stand-alone launch's, which is the parent's kernel.
3. Refusals (DLWP_E_UNSUPPORTED, nothing launched, outputs keep their poison): two output channels, a residual path's gradient,
   rows that are not 64 wide, FNO_FUSE_LIFT_BWD = 0, FNO_FUSE_PROJ_BWD = 0.
4. The rollout trainer with n_layers 1, 2, 3 (both parities of the gA / gB ping-pong) at T = 4 and 5, context 2, knob
   FNO_FUSE_PROJ_BWD on and off: gradient, parameters after two optimizer steps and prediction bit for bit equal, and the number
   of launches drops by ncalls - 1 (the last call's projection backward keeps its launch).
"""
import ctypes as C

import pytest
import torch

from oracle import fno_ref

W, H, N_MODES = 64, 16, (12, 12)
MSE_SCALE = 0.25
E_UNSUPPORTED = -3
POISON = -54321.0
CAP = 5e-4

# (B, hidden, lifting Cin, lifting width, projection width)
CASES = [(1, 8, 2, 32, 40), (2, 27, 10, 40, 256), (2, 32, 10, 256, 32), (1, 32, 2, 40, 256), (2, 8, 10, 256, 32),
         (1, 27, 2, 32, 40)]
# relative max-norm error against float64 of the parent commit's library on CASES, in their order (MI355X)
PARENT_ERR = {
    "gcur": [1.431e-07, 1.662e-07, 1.721e-07, 1.723e-07, 2.299e-07, 2.608e-07],
    "gw1": [2.652e-07, 2.034e-07, 2.194e-07, 1.237e-07, 2.049e-07, 2.137e-07],
    "gb1": [1.236e-07, 2.277e-07, 1.838e-07, 8.358e-08, 1.768e-07, 8.635e-08],
    "gw2": [2.625e-07, 1.873e-07, 1.909e-07, 1.432e-07, 1.652e-07, 2.949e-07],
    "gb2": [4.458e-08, 5.053e-08, 1.334e-07, 8.364e-08, 2.854e-07, 1.069e-08],
}
QUANT = ("gcur", "gw1", "gb1", "gw2", "gb2")


def bound(k, case):
    """twice the parent's error of quantity k on this case, never more than CAP"""
    return min(2.0 * PARENT_ERR[k][CASES.index(case)], CAP)


def case_id(c):
    return "B%d-C%d-Cin%d-L%d-P%d" % c


def bits(t):
    return t.contiguous().view(torch.int32)


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def make_case(B, Cc, Cin, Ch, PCh):
    m1, m2c = N_MODES[0], N_MODES[1] // 2 + 1
    g = torch.Generator().manual_seed(2909 + 3 * Cc + 11 * B + 7 * Cin + Ch + 5 * PCh)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    t = {}
    t["x"] = r(B, Cin, H, W)
    t["w1"] = r(Ch, Cin) / Cin ** 0.5
    t["b1"] = r(Ch) * 0.1
    t["w2"] = r(Cc, Ch) / Ch ** 0.5
    t["b2"] = r(Cc) * 0.1
    t["wspec"] = torch.view_as_complex(r(Cc, Cc, m1, m2c, 2) / Cc ** 0.5)
    t["wskip"] = r(Cc, Cc) / Cc ** 0.5
    t["bias"] = r(Cc) * 0.1
    t["gpre"] = r(B, Cc, H, W)
    t["gpre_b"] = r(B, Cc, H, W)
    t["g0"] = r(B, Cin, H, W)            # what the window's gradient planes hold before this launch
    t["px"] = r(B, Cc, H, W)             # `pre` of the previous call's last block
    t["pw1"] = r(PCh, Cc) / Cc ** 0.5
    t["pb1"] = r(PCh) * 0.1
    t["pw2"] = r(1, PCh) / PCh ** 0.5
    t["pred"] = r(B, 1, H, W)
    t["target"] = r(B, 1, H, W)
    return t


def proj_ref64(t, gy):
    """float64 gradients of the projection MLP for the upstream gradient gy + MSE_SCALE * (pred - target)"""
    leaves = {k: t[k].double().clone().requires_grad_(True) for k in ("px", "pw1", "pb1", "pw2")}
    b2 = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    y = fno_ref.pw_mlp(leaves["px"], leaves["pw1"], leaves["pb1"], leaves["pw2"], b2)
    up = gy.detach().cpu().double()[:, None] + MSE_SCALE * (t["pred"].double() - t["target"].double())
    y.backward(up)
    return dict(gcur=leaves["px"].grad, gw1=leaves["pw1"].grad, gb1=leaves["pb1"].grad, gw2=leaves["pw2"].grad, gb2=b2.grad)


@pytest.fixture(scope="module")
def L(cuda):
    from dlwp_benchmark_amd import lib
    lib.load()
    return lib


class Bench:
    """the tensors of one case on the device, with the forward results the backward entry points read"""

    def __init__(self, L, cuda, case):
        B, Cc, Cin, Ch, PCh = case
        self.L, self.lib, self.case, self.dev = L, L.load(), case, cuda
        lib = self.lib
        self.m1, self.m2c = N_MODES[0], N_MODES[1] // 2 + 1
        self.P = H * W
        self.t = make_case(*case)
        self.plan = C.c_void_p()
        L.check(lib.dlwp_fno_plan_create(Cc, H, W, self.m1, self.m2c, C.byref(self.plan)))
        self.ws = torch.empty(lib.dlwp_fno_block_workspace_bytes(self.plan, B), dtype=torch.uint8, device=cuda)
        d = {k: v.to(cuda) for k, v in self.t.items() if k != "wspec"}
        d["wspec"] = fno_ref.spec_to_mode_major(self.t["wspec"]).to(cuda)
        d["h0"] = torch.empty(B, Cc, H, W, device=cuda)
        L.check(lib.dlwp_pwmlp_fwd(L.ptr(d["x"]), L.ptr(d["w1"]), L.ptr(d["b1"]), L.ptr(d["w2"]), L.ptr(d["b2"]), L.ptr(d["h0"]),
                                   B, Cin, Ch, Cc, self.P, L.stream()))
        pre = torch.empty(B, Cc, H, W, device=cuda)
        self.xhat = torch.empty(B, self.m1, self.m2c, Cc, 2, device=cuda)
        L.check(lib.dlwp_fno_block_fwd(self.plan, L.ptr(d["h0"]), 0, L.ptr(d["wspec"]), L.ptr(d["wskip"]), L.ptr(d["bias"]),
                                       L.ptr(pre), L.ptr(self.xhat), B, L.ptr(self.ws), L.stream()))
        self.d = d

    def close(self):
        self.lib.dlwp_fno_plan_destroy(self.plan)

    def proj_two(self, gy, gy_bstride, gcur, x1, slab_proj, acc):
        """the stand-alone projection backward launch of this build"""
        L, lib, d = self.L, self.lib, self.d
        B, Cc, Cin, Ch, PCh = self.case
        L.check(lib.dlwp_pwmlp_proj_bwd_rows_slab(
            self.plan, L.ptr(d["px"]), L.ptr(d["pw1"]), L.ptr(d["pb1"]), L.ptr(d["pw2"]), gy.data_ptr(), gy_bstride,
            L.ptr(d["pred"]), L.ptr(d["target"]), MSE_SCALE, L.ptr(gcur), L.ptr(x1), L.ptr(slab_proj), acc, B, PCh, 1, L.stream()))

    def run(self, form, proj=None):
        """two backward steps (plain store on NaN-filled slabs, then accumulating), "fused" (the entry point under test) or "two"
        (the two launches it replaces; proj: the second of them, default proj_two -- tools/measure_proj_bwd_parent_err.py passes
        the parent library's own routine)"""
        assert form in ("fused", "two"), form
        proj = proj or self.proj_two
        L, lib, d, dev = self.L, self.lib, self.d, self.dev
        B, Cc, Cin, Ch, PCh = self.case
        P, plan, ws = self.P, self.plan, self.ws
        nan = lambda n: torch.full((n,), float("nan"), device=dev)      # noqa: E731
        gx = d["g0"].clone()
        c0 = Cin - 1                                  # the window plane that is the previous call's output
        gy = gx[:, c0]                                # [B, H, W], batch stride Cin * P
        gcur = torch.full((B, Cc, H, W), POISON, device=dev)
        x1 = torch.full((B, H, self.m2c, Cc, 2), POISON, device=dev)
        slab_skip = nan(lib.dlwp_fno_block_slab_floats(plan, B))
        slab_lift = nan(lib.dlwp_pwmlp_slab_floats(B, Cin, Ch, Cc, P))
        slab_proj = nan(lib.dlwp_pwmlp_slab_floats(B, Cc, PCh, 1, P))
        gwspec = torch.zeros_like(d["wspec"])
        snaps, gy_read = [], []
        for acc, up in ((0, d["gpre"]), (1, d["gpre_b"])):
            lift_args = [plan, L.ptr(d["h0"]), L.ptr(d["wspec"]), L.ptr(d["wskip"]), L.ptr(up), L.ptr(self.xhat), L.ptr(gwspec),
                         L.ptr(slab_skip), acc, L.ptr(d["x"]), L.ptr(d["w1"]), L.ptr(d["b1"]), L.ptr(d["w2"]), L.ptr(gx), 1,
                         L.ptr(slab_lift), acc, B, Cin, Ch]
            if form == "fused":
                L.check(lib.dlwp_fno_block_lift_proj_bwd_slab(
                    *lift_args, L.ptr(d["px"]), L.ptr(d["pw1"]), L.ptr(d["pb1"]), L.ptr(d["pw2"]), gy.data_ptr(), Cin * P,
                    L.ptr(d["pred"]), L.ptr(d["target"]), MSE_SCALE, None, L.ptr(gcur), L.ptr(x1), L.ptr(slab_proj), acc, PCh, 1,
                    L.ptr(ws), L.stream()))
            else:
                L.check(lib.dlwp_fno_block_lift_bwd_slab(*lift_args, L.ptr(ws), L.stream()))
                proj(gy, Cin * P, gcur, x1, slab_proj, acc)
            torch.cuda.synchronize()
            gy_read.append(gy.clone())
            snaps.append(dict(slab_proj=slab_proj.clone(), slab_lift=slab_lift.clone(), gcur=gcur.clone(), x1=x1.clone(),
                              gx=gx.clone()))
        g = {k: torch.zeros_like(d[k]) for k in ("pw1", "pb1", "pw2")}
        gb2 = torch.zeros(1, device=dev)
        L.check(lib.dlwp_pwmlp_slab_fold(L.ptr(slab_proj), L.ptr(g["pw1"]), L.ptr(g["pb1"]), L.ptr(g["pw2"]), L.ptr(gb2), B, Cc, PCh,
                                         1, P, L.stream()))
        torch.cuda.synchronize()
        out = dict(gcur=gcur, x1=x1, gx=gx, slab_skip=slab_skip, gwspec=gwspec, gw1=g["pw1"], gb1=g["pb1"], gw2=g["pw2"], gb2=gb2)
        return out, snaps, gy_read

    def errors(self, out, gy_read):
        """relative max-norm errors of the projection phase against float64: gcur is the last call's, the parameter gradients are
        the sum of both calls"""
        ra, rb = proj_ref64(self.t, gy_read[0]), proj_ref64(self.t, gy_read[1])
        ref = {k: (rb[k] if k == "gcur" else ra[k] + rb[k]) for k in QUANT}
        return {k: rel_err(out[k], ref[k]) for k in QUANT}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_entry_point_against_two_launches(L, cuda, case):
    B, Cc, Cin, Ch, PCh = case
    bench = Bench(L, cuda, case)
    try:
        fused = {}
        try:
            for knob in (1, 0):
                L.set_tuning("FNO_SKIP_WGRAD_IN_MIX", knob)
                with L.kernel_accounting() as acc:
                    res = bench.run("fused")
                fused[knob] = res + ({r["name"]: r["calls"] for r in acc.rows},)
        finally:
            L.set_tuning("FNO_SKIP_WGRAD_IN_MIX", None)
        with L.kernel_accounting() as acc:
            two, snaps2, gy2 = bench.run("two")
        names2 = {r["name"]: r["calls"] for r in acc.rows}
        err2 = bench.errors(two, gy2)
    finally:
        bench.close()
    ncb, nib = (Cc + 15) // 16, (Cin + 15) // 16
    lift, proj = "fno_spatial_lift_bwd_kernel<%d, 1, %d>" % (ncb, nib), "pwmlp_bwd_kernel<%d, 0, 8>" % ncb
    assert names2.get(lift) == 2 and names2.get(proj) == 2, names2
    assert not bool((two["gcur"] == POISON).any()) and not bool((two["x1"] == POISON).any())
    for knob, (got, snaps, gy_read, names) in fused.items():
        err = bench.errors(got, gy_read)
        print({"case": case_id(case), "knob": knob, "err": err, "err_two_launches": err2, "bound": {k: bound(k, case) for k in QUANT}})
        assert names.get(lift) == 2, names
        assert not any(n.startswith(("pwmlp_bwd", "fno_spatial_roles", "fno_rows")) for n in names), names
        for k in got:
            assert torch.equal(bits(got[k]), bits(two[k])), "not bit for bit the two launches: " + k
        for i in (0, 1):
            for k in snaps[i]:
                assert torch.equal(bits(snaps[i][k]), bits(snaps2[i][k])), "call %d not bit for bit the two launches: %s" % (i, k)
        for k in QUANT:
            assert err[k] <= bound(k, case), (knob, k, err[k], bound(k, case))


REFUSALS = ["cout2", "gres", "rows-32-wide", "lift-knob-0", "proj-knob-0"]


@pytest.mark.gpu
@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(L, cuda, what):
    lib = L.load()
    B, Cc, Cin, Ch, PCh = 1, 8, 3, 16, 16
    Wd = 32 if what == "rows-32-wide" else 64
    PCout = 2 if what == "cout2" else 1
    Hh, m1, m2c = 8, 4, 3
    P = Hh * Wd
    plan = C.c_void_p()
    L.check(lib.dlwp_fno_plan_create(Cc, Hh, Wd, m1, m2c, C.byref(plan)))
    z = lambda *s: torch.zeros(*s, device=cuda)               # noqa: E731
    poison = lambda *s: torch.full(s, POISON, device=cuda)    # noqa: E731
    knob = {"lift-knob-0": "FNO_FUSE_LIFT_BWD", "proj-knob-0": "FNO_FUSE_PROJ_BWD"}.get(what)
    try:
        if knob:
            L.set_tuning(knob, 0)
        ws = torch.empty(lib.dlwp_fno_block_workspace_bytes(plan, B), dtype=torch.uint8, device=cuda)
        outs = dict(gx=poison(B, Cin, Hh, Wd), gcur=poison(B, Cc, Hh, Wd), x1=poison(B, Hh, m2c, Cc, 2),
                    slab_skip=poison(B * Hh * ((Cc * Cc + Cc + 3) // 4 * 4)),
                    slab_lift=poison(lib.dlwp_pwmlp_slab_floats(B, Cin, Ch, Cc, P)),
                    slab_proj=poison(lib.dlwp_pwmlp_slab_floats(B, Cc, PCh, PCout, P)), gwspec=poison(m1, m2c, Cc, Cc, 2))
        gres = z(B, PCout, Hh, Wd) if what == "gres" else None
        with L.kernel_accounting() as acc:
            rc = lib.dlwp_fno_block_lift_proj_bwd_slab(
                plan, L.ptr(z(B, Cc, Hh, Wd)), L.ptr(z(m1, m2c, Cc, Cc, 2)), L.ptr(z(Cc, Cc)), L.ptr(z(B, Cc, Hh, Wd)),
                L.ptr(z(B, m1, m2c, Cc, 2)), L.ptr(outs["gwspec"]), L.ptr(outs["slab_skip"]), 0, L.ptr(z(B, Cin, Hh, Wd)),
                L.ptr(z(Ch, Cin)), L.ptr(z(Ch)), L.ptr(z(Cc, Ch)), L.ptr(outs["gx"]), 1, L.ptr(outs["slab_lift"]), 0, B, Cin, Ch,
                L.ptr(z(B, Cc, Hh, Wd)), L.ptr(z(PCh, Cc)), L.ptr(z(PCh)), L.ptr(z(PCout, PCh)), L.ptr(z(B, PCout, Hh, Wd)),
                PCout * P, L.ptr(z(B, PCout, Hh, Wd)), L.ptr(z(B, PCout, Hh, Wd)), MSE_SCALE, L.ptr(gres), L.ptr(outs["gcur"]),
                L.ptr(outs["x1"]), L.ptr(outs["slab_proj"]), 0, PCh, PCout, L.ptr(ws), L.stream())
            torch.cuda.synchronize()
    finally:
        if knob:
            L.set_tuning(knob, None)
        lib.dlwp_fno_plan_destroy(plan)
    assert rc == E_UNSUPPORTED, rc
    assert acc.rows == [], acc.rows
    for k, v in outs.items():
        assert bool((v == POISON).all()), k


TRAINER = [(n_layers, T) for n_layers in (1, 2, 3) for T in (4, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_layers,T", TRAINER, ids=["L%d-T%d" % t for t in TRAINER])
def test_trainer_knob_on_and_off(L, cuda, n_layers, T):
    from dlwp_benchmark_amd import nsbench
    B, ctx, hidden = 2, 2, (8, 27, 32)[n_layers - 1]
    torch.manual_seed(5003 + n_layers + T)
    module = nsbench.TFNO2DModule(n_modes=[12, 12], in_channels=1, hidden_channels=hidden, lifting_channels=32,
                                  projection_channels=40, out_channels=1, n_layers=n_layers, context_size=ctx).to(cuda)
    g = torch.Generator().manual_seed(223)
    x = torch.randn(B, T, 1, H, W, generator=g).to(cuda)
    y = torch.randn(B, T, 1, H, W, generator=g).to(cuda)
    p0 = module.flat_params.data.clone()

    def run(knob):
        L.set_tuning("FNO_FUSE_PROJ_BWD", knob)
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
                module.train_step(x, y, ctx, optimizer=opt, use_graph=True)
            tr.forward(keep_activations=False)
            torch.cuda.synchronize()
            out.update(params=module.flat_params.data.clone(), pred=tr.out.clone())
            return out
        finally:
            L.set_tuning("FNO_FUSE_PROJ_BWD", None)

    on, off, default = run(1), run(0), run(None)
    ncalls, ncb = T - (ctx - 1), (hidden + 15) // 16
    lift, proj = "fno_spatial_lift_bwd_kernel<%d, 1, 1>" % ncb, "pwmlp_bwd_kernel<%d, 0, 8>" % ncb
    print({"on": on["names"], "off": off["names"], "loss": [r["loss"].item() for r in (on, off)]})
    assert on["names"].get(lift) == off["names"].get(lift) == ncalls, (on["names"], off["names"])
    assert off["names"].get(proj) == ncalls and on["names"].get(proj) == 1, (on["names"], off["names"])
    assert sum(off["names"].values()) - sum(on["names"].values()) == ncalls - 1
    assert default["names"] == on["names"], "the fused form is the default"
    assert bool(on["grad"].abs().max() > 0)
    for name in ("grad", "params", "pred"):
        assert torch.equal(bits(on[name]), bits(off[name])), "differs between knob 1 and knob 0: " + name
        assert torch.equal(bits(on[name]), bits(default[name])), "differs between knob 1 and the default: " + name
