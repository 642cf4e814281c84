"""The last block's forward `spatial` and the projection MLP (chained with the next net call's lifting MLP) as one launch
(fno_spatial_proj_fwd_kernel): the row `spatial` finishes in LDS is the projection's input tile in place; `pre` is still written.

1. dlwp_fno_block_proj_fwd against the two-launch sequence of the same build -- dlwp_fno_block_fwd, then dlwp_pwmlp_proj_lift_fwd
   (pwmlp_fwd_chain_kernel, or pwmlp_fwd_kernel without a second MLP) -- bit for bit (both run the same phase functions on the
   same threads), and against float64 (oracle/fno_ref.py: fno_block, pw_mlp) under the FWD_TOL of tests/test_gpu_fno.py.
   Sentinel tails behind every output, poison inside.  Shapes: one channel tile with ragged hidden widths; the headline's tiles
   at quarter height with a handed-over channel; 27 channels (padding rows of the handed-over tile), projection only with a
   residual; two handed-over channels; 38 channels (three channel tiles), projection only.
2. The shapes the library keeps on two launches are refused with DLWP_E_UNSUPPORTED and the outputs keep their poison.
3. The rollout trainer takes the fused launch by itself on the training path and the two launches with FNO_FUSE_PROJ_FWD = 0;
   gradient buffer and prediction are bit for bit equal and the eager accounting names the kernels that ran.  The evaluation
   path (keep_activations = 0) keeps the chained launch.
"""
import ctypes as C

import pytest
import torch

from oracle import fno_ref

FWD_TOL = 1e-4
SENTINEL = 12345.0
POISON = -54321.0
E_UNSUPPORTED = -3
W = 64

# (B, C, H, n_modes, Ch1, Cout1, residual, (Cin2, Ch2, next_ch) or None, act_in)
CASES = [
    # (projection 40 -> 1 with lifting 3 -> 40 -> 8 is refused by the chained launch itself: a 48 x 20 W1 image cannot host the
    #  lifting MLP's partial tiles, a 16 x 52 W2 image not the DFT table -- see REFUSALS; the widths here are the smallest ragged
    #  ones it takes)
    (1, 8, 8, (4, 4), 220, 1, False, (3, 136, (2,)), 0),
    (2, 32, 16, (12, 12), 256, 1, False, (10, 256, (9,)), 1),
    (4, 27, 8, (4, 12), 64, 1, True, None, 1),
    (2, 32, 16, (12, 12), 256, 2, False, (6, 256, (4, 5)), 1),      # (12 row frequencies need at least 12 rows: H 16, not 8)
    (1, 38, 8, (4, 4), 48, 1, False, None, 1),
]


def case_id(c):
    s = "B%d-C%d-%dx64-m%dx%d-proj%d-%d" % (c[0], c[1], c[2], c[3][0], c[3][1], c[4], c[5])
    if c[6]:
        s += "-res"
    if c[7]:
        s += "-lift%d-%d" % (c[7][0], c[7][1])
    return s


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def L(cuda):
    from dlwp_benchmark_amd import lib
    lib.load()
    return lib


def padded(dev, *shape):
    """a poisoned buffer of `shape` in front of a sentinel tail that no kernel may touch (returns the view and the tail)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 256,), SENTINEL, device=dev)
    flat[:n] = POISON
    return flat[:n].view(*shape), flat[n:]


def next_ch_bytes(next_ch):
    v = [-1] * 8
    for o, ch in enumerate(next_ch or ()):
        v[o] = ch
    return bytes(x & 0xFF for x in v)


def make_case(B, Cc, H, n_modes, Ch1, Cout1, residual, lift, act_in):
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    g = torch.Generator().manual_seed(4111 + 3 * Cc + 11 * B + H + 5 * n_modes[1] + Ch1 + 7 * Cout1)
    t = {}
    t["x"] = torch.randn(B, Cc, H, W, generator=g)
    t["wspec"] = torch.view_as_complex(torch.randn(Cc, Cc, m1, m2c, 2, generator=g) / Cc ** 0.5)
    t["wskip"] = torch.randn(Cc, Cc, generator=g) / Cc ** 0.5
    t["bias"] = torch.randn(Cc, generator=g) * 0.1
    t["pw1"] = torch.randn(Ch1, Cc, generator=g) / Cc ** 0.5
    t["pb1"] = torch.randn(Ch1, generator=g) * 0.1
    t["pw2"] = torch.randn(Cout1, Ch1, generator=g) / Ch1 ** 0.5
    t["pb2"] = torch.randn(Cout1, generator=g) * 0.1
    if residual:
        t["res"] = torch.randn(B, Cout1, H, W, generator=g)
    if lift:
        Cin2, Ch2, _ = lift
        t["window"] = torch.randn(B, Cin2, H, W, generator=g)
        t["lw1"] = torch.randn(Ch2, Cin2, generator=g) / Cin2 ** 0.5
        t["lb1"] = torch.randn(Ch2, generator=g) * 0.1
        t["lw2"] = torch.randn(Cc, Ch2, generator=g) / Ch2 ** 0.5
        t["lb2"] = torch.randn(Cc, generator=g) * 0.1
    return t


def ref64(t, n_modes, lift, act_in):
    d = {k: (v.to(torch.complex128) if v.is_complex() else v.double()) for k, v in t.items()}
    xin = torch.nn.functional.gelu(d["x"]) if act_in else d["x"]
    m2c = n_modes[1] // 2 + 1
    Wd, H = xin.shape[-1], xin.shape[-2]
    out = {"pre": fno_ref.fno_block(xin, d["wspec"], d["wskip"], d["bias"], list(n_modes))}
    frame = fno_ref.pw_mlp(out["pre"], d["pw1"], d["pb1"], d["pw2"], d["pb2"])
    if "res" in d:
        frame = frame + d["res"]
    out["frame"] = frame
    if lift:
        win = d["window"].clone()
        for o, ch in enumerate(lift[2]):
            win[:, ch] = frame[:, o]
        h0 = fno_ref.pw_mlp(win, d["lw1"], d["lb1"], d["lw2"], d["lb2"])
        out["h0_next"] = h0
        # x1[b][h][kx][c] = sum_w h0[b][c][h][w] e^{-2 pi i kx w / W} / (H W)
        x1 = torch.fft.fft(h0, dim=-1)[..., :m2c] / (H * Wd)
        out["x1_next"] = torch.view_as_real(x1.permute(0, 2, 3, 1).contiguous())
    return out


def run_case(L, lib, cuda, plan, t, case, fused):
    B, Cc, H, n_modes, Ch1, Cout1, residual, lift, act_in = case
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    d = {k: v.to(cuda) for k, v in t.items() if k != "wspec"}
    d["wspec"] = fno_ref.spec_to_mode_major(t["wspec"]).to(cuda)
    ws = torch.empty(lib.dlwp_fno_block_workspace_bytes(plan, B), dtype=torch.uint8, device=cuda)
    o, tails = {}, {}
    o["pre"], tails["pre"] = padded(cuda, B, Cc, H, W)
    o["xhat"], tails["xhat"] = padded(cuda, B, m1, m2c, Cc, 2)
    o["frame"], tails["frame"] = padded(cuda, B, Cout1, H, W)
    o["h0_next"], tails["h0_next"] = padded(cuda, B, Cc, H, W)
    o["x1_next"], tails["x1_next"] = padded(cuda, B, H, m2c, Cc, 2)
    Cin2, Ch2, nch = lift if lift else (0, 0, None)
    g = lambda k: L.ptr(d[k]) if k in d else None
    mlp2 = (g("window"), g("lw1"), g("lb1"), g("lw2"), g("lb2"), o["h0_next"].data_ptr(), o["x1_next"].data_ptr(), Cin2, Ch2,
            next_ch_bytes(nch), B)
    proj = (g("pw1"), g("pb1"), g("pw2"), g("pb2"), g("res"), o["frame"].data_ptr(), Ch1, Cout1)
    if fused:
        rc = lib.dlwp_fno_block_proj_fwd(plan, g("x"), act_in, g("wspec"), g("wskip"), g("bias"), o["pre"].data_ptr(),
                                         o["xhat"].data_ptr(), *proj, *mlp2, L.ptr(ws), L.stream())
    else:
        rc = lib.dlwp_fno_block_fwd(plan, g("x"), act_in, g("wspec"), g("wskip"), g("bias"), o["pre"].data_ptr(),
                                    o["xhat"].data_ptr(), B, L.ptr(ws), L.stream())
        if rc == 0:
            rc = lib.dlwp_pwmlp_proj_lift_fwd(plan, o["pre"].data_ptr(), *proj, *mlp2, L.stream())
    torch.cuda.synchronize()
    return rc, o, tails


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_entry_point_against_two_launches(L, cuda, case):
    B, Cc, H, n_modes, Ch1, Cout1, residual, lift, act_in = case
    lib = L.load()
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    t = make_case(*case)
    ref = ref64(t, n_modes, lift, act_in)
    plan = C.c_void_p()
    L.check(lib.dlwp_fno_plan_create(Cc, H, W, m1, m2c, C.byref(plan)))
    try:
        with L.kernel_accounting() as acc:
            rc, got, tails = run_case(L, lib, cuda, plan, t, case, True)
        L.check(rc)
        names = {r["name"] for r in acc.rows}
        with L.kernel_accounting() as acc2:
            rc2, two, tails2 = run_case(L, lib, cuda, plan, t, case, False)
        L.check(rc2)
        names2 = {r["name"] for r in acc2.rows}
    finally:
        lib.dlwp_fno_plan_destroy(plan)

    keys = ["pre", "xhat", "frame"] + (["h0_next", "x1_next"] if lift else [])
    err = {k: rel_err(got[k], ref[k]) for k in keys if k != "xhat"}
    print({"case": case_id(case), "err": err, "kernels": sorted(n for n in names if n.startswith(("fno_spatial", "pwmlp_fwd")))})
    ncb, nbn = (Cc + 15) // 16, (2 * m2c + 15) // 16
    assert "fno_spatial_proj_fwd_kernel<%d, %d, %d>" % (ncb, nbn, ncb if lift else 0) in names, names
    assert not any(n.startswith(("fno_spatial_kernel", "pwmlp_fwd")) for n in names), names
    assert "fno_spatial_kernel<%d, %d, 0>" % (ncb, nbn) in names2, names2
    assert ("pwmlp_fwd_chain_kernel<1, %d, 16>" % ncb if lift else "pwmlp_fwd_kernel<1, 16>") in names2, names2
    for k in ("pre", "xhat", "frame", "h0_next", "x1_next"):
        assert bool((tails[k] == SENTINEL).all()) and bool((tails2[k] == SENTINEL).all()), "a kernel wrote past the end of " + k
        if k in keys:
            assert not bool((got[k] == POISON).any()) and not bool((two[k] == POISON).any()), "poison left in " + k
            assert torch.equal(got[k].view(torch.int32), two[k].view(torch.int32)), "not bit for bit the two launches: " + k
        else:
            assert bool((got[k] == POISON).all()) and bool((two[k] == POISON).all()), "an unused output was written: " + k
    for k, e in err.items():
        assert e <= FWD_TOL, (k, e)


# (C, H, W, n_modes, Ch1, Cout1, lift, knob, 3-D)
REFUSALS = {
    "rows-32-wide": (8, 8, 32, (4, 4), 224, 1, True, None, False),
    "rows-128-wide": (8, 8, 128, (4, 4), 224, 1, True, None, False),
    "C_pad-64": (54, 8, 64, (4, 4), 224, 1, False, None, False),
    "wide-plan": (80, 8, 64, (4, 4), 224, 1, False, None, False),
    "3-D-plan": (8, 8, 64, (4, 4), 224, 1, False, None, True),
    "Cout1-9": (8, 8, 64, (4, 4), 224, 9, False, None, False),
    "knob-0": (8, 8, 64, (4, 4), 224, 1, True, 0, False),
    "chain-refuses": (8, 8, 64, (4, 4), 40, 1, True, None, False),      # the lifting MLP's partial tiles do not fit the W1 image
}


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(REFUSALS))
def test_refusals(L, cuda, key):
    """shapes and settings the trainer keeps on two launches: the entry returns DLWP_E_UNSUPPORTED and launches nothing"""
    Cc, H, Wd, n_modes, Ch1, Cout1, lift, knob, three_d = REFUSALS[key]
    lib = L.load()
    B, Cin2, Ch2, T = 1, 3, 16, 2
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    plan = C.c_void_p()
    if three_d:
        L.check(lib.dlwp_fno_plan_create3d(Cc, T, H, Wd, 2, m1, m2c, C.byref(plan)))
        rows, nm = T * H, 2 * m1
    else:
        L.check(lib.dlwp_fno_plan_create(Cc, H, Wd, m1, m2c, C.byref(plan)))
        rows, nm = H, m1
    try:
        z = lambda *s: torch.zeros(*s, device=cuda)
        ws = torch.empty(lib.dlwp_fno_block_workspace_bytes(plan, B), dtype=torch.uint8, device=cuda)
        outs = [padded(cuda, B, Cc, rows, Wd), padded(cuda, B, nm, m2c, Cc, 2), padded(cuda, B, Cout1, rows, Wd),
                padded(cuda, B, Cc, rows, Wd), padded(cuda, B, rows, m2c, Cc, 2)]
        pre, xhat, frame, h0n, x1n = [o[0] for o in outs]
        if knob is not None:
            L.set_tuning("FNO_FUSE_PROJ_FWD", knob)
        try:
            rc = lib.dlwp_fno_block_proj_fwd(plan, L.ptr(z(B, Cc, rows, Wd)), 1, L.ptr(z(nm, m2c, Cc, Cc, 2)), L.ptr(z(Cc, Cc)),
                                             L.ptr(z(Cc)), pre.data_ptr(), xhat.data_ptr(), L.ptr(z(Ch1, Cc)), L.ptr(z(Ch1)),
                                             L.ptr(z(Cout1, Ch1)), L.ptr(z(Cout1)), None, frame.data_ptr(), Ch1, Cout1,
                                             L.ptr(z(B, Cin2, rows, Wd)) if lift else None, L.ptr(z(Ch2, Cin2)), L.ptr(z(Ch2)),
                                             L.ptr(z(Cc, Ch2)), L.ptr(z(Cc)), h0n.data_ptr(), x1n.data_ptr(), Cin2, Ch2,
                                             next_ch_bytes((1,)), B, L.ptr(ws), L.stream())
        finally:
            L.set_tuning("FNO_FUSE_PROJ_FWD", None)
        torch.cuda.synchronize()
    finally:
        lib.dlwp_fno_plan_destroy(plan)
    assert rc == E_UNSUPPORTED, rc
    for buf, tail in outs:
        assert bool((buf == POISON).all()) and bool((tail == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n_layers", [2, 1])
def test_trainer_takes_the_fused_launch(L, cuda, n_layers):
    """n_layers 1: the last block is block 0 and its input (the lifting output) is not activated"""
    from dlwp_benchmark_amd import nsbench
    module = nsbench.TFNO2DModule(n_modes=[12, 12], in_channels=1, hidden_channels=32, lifting_channels=256,
                                  projection_channels=256, out_channels=1, n_layers=n_layers, context_size=3).to(cuda)
    g = torch.Generator().manual_seed(131)
    x = torch.randn(2, 6, 1, 64, 64, generator=g).to(cuda)
    y = torch.randn(2, 6, 1, 64, 64, generator=g).to(cuda)

    def step():
        tr = module.trainer(2, 6, 64, 64, 3)
        module.flat_grad.zero_()
        with L.kernel_accounting() as acc:
            module.train_step(x, y, 3, optimizer=None, use_graph=False)
            torch.cuda.synchronize()
        return module.flat_grad.clone(), tr.out.clone(), {r["name"] for r in acc.rows}

    fused = ("fno_spatial_proj_fwd_kernel<2, 1, 2>", "fno_spatial_proj_fwd_kernel<2, 1, 0>")      # chained calls, the last call
    L.set_tuning("FNO_FUSE_PROJ_FWD", None)
    try:
        grad_f, out_f, names_f = step()
        L.set_tuning("FNO_FUSE_PROJ_FWD", 0)
        grad_2, out_2, names_2 = step()
    finally:
        L.set_tuning("FNO_FUSE_PROJ_FWD", None)
    with L.kernel_accounting() as acc:
        tr = module.trainer(2, 6, 64, 64, 3)
        tr.forward(keep_activations=False)
        torch.cuda.synchronize()
    names_e = {r["name"] for r in acc.rows}
    print(sorted(names_f), sorted(names_2), sorted(names_e))
    assert all(n in names_f for n in fused) and not any(n.startswith("pwmlp_fwd_chain_kernel") for n in names_f), names_f
    assert not any(n.startswith("fno_spatial_proj_fwd") for n in names_2) and "pwmlp_fwd_chain_kernel<1, 2, 16>" in names_2, names_2
    assert "pwmlp_fwd_chain_kernel<1, 2, 16>" in names_e and not any(n.startswith("fno_spatial_proj_fwd") for n in names_e), names_e
    assert bool(grad_f.abs().max() > 0)
    assert torch.equal(grad_f.view(torch.int32), grad_2.view(torch.int32)), "gradient buffer differs between the two dispatches"
    assert torch.equal(out_f.view(torch.int32), out_2.view(torch.int32)), "prediction differs between the two dispatches"
