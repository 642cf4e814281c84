"""Host-side refusals of dlwp_crps_loss_fwd_bwd / dlwp_crps_loss_ws_floats (csrc/ensemble.hip), of the wrappers in
dlwp_benchmark_amd/ensemble.py and of train_dlwp's loss keywords: every call here is rejected before anything touches a GPU, so the
checks run on a CPU-only box."""
import numpy as np
import pytest
import torch

E_INVALID, E_UNSUPPORTED = -1, -3
P = 4096          # a non-NULL, 16-byte aligned pointer value: never dereferenced, the calls are refused first


@pytest.fixture(scope="module")
def L():
    from dlwp_benchmark_amd import lib
    lib.load()
    return lib


def crps(lib, **kw):
    """a valid call (B 2, M 5, T 4, V 3, 8 x 16, dense members, fair) with the named arguments replaced"""
    a = dict(members=P, bs=5 * 4 * 3 * 128, ms=4 * 3 * 128, ts=3 * 128, target=P, roww=None, varw=None, B=2, M=5, T=4, V=3, H=8, W=16,
             lam=1.0, loss=P, grad=P, ws=P)
    a.update(kw)
    return lib.dlwp_crps_loss_fwd_bwd(a["members"], a["bs"], a["ms"], a["ts"], a["target"], a["roww"], a["varw"], a["B"], a["M"], a["T"],
                                      a["V"], a["H"], a["W"], a["lam"], a["loss"], a["grad"], a["ws"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(members=None), E_INVALID, b"members is NULL"),
    (dict(target=None), E_INVALID, b"target is NULL"),
    (dict(loss=None), E_INVALID, b"loss_out is NULL"),
    (dict(ws=None), E_INVALID, b"ws is NULL"),
    (dict(B=0), E_INVALID, b"Bc 0"),
    (dict(T=-1), E_INVALID, b"Tc -1"),
    (dict(V=0), E_INVALID, b"V 0"),
    (dict(H=0), E_INVALID, b"H 0"),
    (dict(W=-3), E_INVALID, b"W -3"),
    (dict(M=1), E_INVALID, b"M 1 members"),
    (dict(M=0), E_INVALID, b"M 0 members"),
    (dict(M=65), E_UNSUPPORTED, b"M 65 members above 64"),
    (dict(bs=-1), E_INVALID, b"batch -1"),
    (dict(ms=-1536), E_INVALID, b"member -1536"),
    (dict(ts=-384), E_INVALID, b"time -384"),
    (dict(H=2048, W=2048), E_UNSUPPORTED, b"2048 x 2048"),
    (dict(V=70000), E_UNSUPPORTED, b"V 70000"),
    (dict(B=70000), E_UNSUPPORTED, b"Bc 70000"),
    (dict(lam=-0.25), E_INVALID, b"pair_coeff -0.25"),
    (dict(lam=1.5), E_INVALID, b"pair_coeff 1.5"),
    (dict(lam=float("nan")), E_INVALID, b"pair_coeff nan"),
    (dict(lam=float("inf")), E_INVALID, b"pair_coeff inf"),
])
def test_refusals(L, kw, code, word):
    lib = L.load()
    assert crps(lib, **kw) == code
    assert b"crps_loss" in lib.dlwp_last_error() and word in lib.dlwp_last_error(), lib.dlwp_last_error()


def test_knob_and_workspace(L):
    lib = L.load()
    assert "dlwp_crps_loss_fwd_bwd" in L.tuning_knobs()["ENS_BUCKET"]
    # one partial per (sample, frame, variable) and pixel block; the blocks are dlwp_ens_diag's: a function of H W only
    assert lib.dlwp_crps_loss_ws_floats(2, 5, 4, 3, 8, 16) == 2 * 4 * 3 * 1
    assert lib.dlwp_crps_loss_ws_floats(1, 64, 1, 8, 32, 64) == 8 * 8                           # 2048 pixels: 8 blocks of 256
    assert lib.dlwp_crps_loss_ws_floats(3, 2, 1, 8, 32, 64) == 3 * 8 * 8                        # ... whatever M is
    assert lib.dlwp_crps_loss_ws_floats(1, 2, 1, 1, 721, 1440) == 254                           # 16 pixels per thread: 254 blocks
    assert lib.dlwp_crps_loss_ws_floats(0, 5, 4, 3, 8, 16) == E_INVALID and b"Bc 0" in lib.dlwp_last_error()
    assert lib.dlwp_crps_loss_ws_floats(2, 1, 4, 3, 8, 16) == E_INVALID and b"M 1" in lib.dlwp_last_error()
    assert lib.dlwp_crps_loss_ws_floats(2, 65, 4, 3, 8, 16) == E_UNSUPPORTED and b"M 65" in lib.dlwp_last_error()
    assert lib.dlwp_crps_loss_ws_floats(2, 5, 4, 3, 4096, 4096) == E_UNSUPPORTED and b"4096 x 4096" in lib.dlwp_last_error()
    for value, m, code, word in [(7, 5, E_INVALID, b"crps_loss: ENS_BUCKET 7"), (8, 9, E_UNSUPPORTED, b"ENS_BUCKET 8 cannot hold M 9")]:
        L.set_tuning("ENS_BUCKET", value)
        try:
            assert crps(lib, M=m, bs=m * 4 * 3 * 128) == code and word in lib.dlwp_last_error()
        finally:
            L.set_tuning("ENS_BUCKET", None)


def test_wrappers_refuse_on_the_host():
    from dlwp_benchmark_amd import ensemble as E, lib as L
    m, t = torch.zeros(2, 4, 3, 2, 4, 8), torch.zeros(2, 3, 2, 4, 8)
    for call in (E.crps_loss, E.crps_loss_and_grad):
        with pytest.raises(ValueError, match="differ"):
            call(m[:, :, :2], t)
        with pytest.raises(ValueError, match=r"\[B, M, T, V, H, W\]"):
            call(m[0], t)
        with pytest.raises(ValueError, match="M = 1 members"):
            call(m[:, :1], t)
        with pytest.raises(ValueError, match="M = 65 members"):
            call(torch.zeros(1, 65, 1, 1, 2, 2), torch.zeros(1, 1, 1, 2, 2))
        with pytest.raises(ValueError, match="alpha = 1.5"):
            call(m, t, alpha=1.5)
        with pytest.raises(ValueError, match="alpha = -0.1"):
            call(m, t, alpha=-0.1)
        with pytest.raises(ValueError, match="alpha = nan"):
            call(m, t, alpha=float("nan"))
        with pytest.raises(L.DlwpError, match="no CPU fallback"):            # CPU tensors are refused, never computed on
            call(m, t)
        with pytest.raises(L.DlwpError, match="float32"):
            call(m.double(), t.double())
    hm, ht = torch.zeros(2, 3, 2, 2, 12, 2, 2), torch.zeros(2, 2, 2, 12, 2, 2)
    assert E._crps_weights((12, 2, 2), None, None, 2, "cpu") == (24, 2, None, None)       # HPX planes: H = 12 n, W = n
    with pytest.raises(ValueError, match="equal area"):
        E._crps_weights((12, 2, 2), np.zeros(24), None, 2, "cpu")
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        E.crps_loss(hm, ht)
    with pytest.raises(ValueError, match=r"\[12, n, n\]"):
        E._crps_weights((12, 2, 3), None, None, 2, "cpu")
    with pytest.raises(ValueError, match="lats_deg must have 4"):
        E._crps_weights((4, 8), np.zeros(5), None, 2, "cpu")
    with pytest.raises(ValueError, match=r"one entry per variable \(2\)"):
        E._crps_weights((4, 8), None, [1.0, 2.0, 3.0], 2, "cpu")
    with pytest.raises(ValueError, match="finite and not negative"):
        E._crps_weights((4, 8), None, [1.0, -2.0], 2, "cpu")
    H, W, roww, varw = E._crps_weights((4, 8), [-60.0, -20.0, 20.0, 60.0], [1.0, 0.5], 2, "cpu")
    from dlwp_benchmark_amd.evaluate import lat_weights
    assert (H, W) == (4, 8) and torch.equal(roww, lat_weights([-60.0, -20.0, 20.0, 60.0])) and varw.tolist() == [1.0, 0.5]
    assert E.pair_coefficient(1.0, 4) == 1.0 and E.pair_coefficient(0.0, 4) == 0.75

    with pytest.raises(ValueError, match="members = 1"):
        E.CrpsLoss(1)
    with pytest.raises(ValueError, match="members = 65"):
        E.CrpsLoss(65)
    with pytest.raises(ValueError, match="alpha = 2.0"):
        E.CrpsLoss(4, alpha=2.0)
    with pytest.raises(ValueError, match="is not 4 members of the target"):
        E.CrpsLoss(4).loss_and_grad(torch.zeros(6, 3, 2, 4, 8), t)
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        E.CrpsLoss(4).loss_and_grad(torch.zeros(8, 3, 2, 4, 8), t)

    x = torch.zeros(2, 2, 3, 5, 7)
    with pytest.raises(ValueError, match="validate_items=False takes an int32"):
        E.perturb_members(x, [0, 1], 4, 0.1, 1, validate_items=False)
    with pytest.raises(ValueError, match="validate_items=False takes an int32"):
        E.perturb_members(x, torch.zeros(2, dtype=torch.int64), 4, 0.1, 1, validate_items=False)
    with pytest.raises(ValueError, match="validate_items=False takes an int32"):
        E.perturb_members(x, torch.zeros(3, dtype=torch.int32), 4, 0.1, 1, validate_items=False)
    with pytest.raises(L.DlwpError, match="no CPU fallback"):                # a well-formed table passes the checks; the CPU tensor does not
        E.perturb_members(x, torch.zeros(2, dtype=torch.int32), 4, 0.1, 1, validate_items=False)


def test_train_dlwp_refuses_on_the_host():
    from dlwp_benchmark_amd import train_loop
    model = torch.nn.Linear(1, 1)
    for kw, word in [(dict(loss="crps"), "needs ensemble"),
                     (dict(loss="crps", ensemble=1), "ensemble = 1 members"),
                     (dict(loss="crps", ensemble=65), "ensemble = 65 members"),
                     (dict(loss="mse", ensemble=4), "needs loss='crps'"),
                     (dict(ensemble=4), "needs loss='crps'"),
                     (dict(loss="crps", ensemble=4, ensemble_sigma=0.1), "needs a seed"),
                     (dict(loss="crps", ensemble=4, ensemble_sigma=-0.1, ensemble_seed=1), "finite and not negative"),
                     (dict(loss="crps", ensemble=4, crps_alpha=1.5), "alpha = 1.5"),
                     (dict(loss="mae"), "loss = 'mae'")]:
        with pytest.raises(ValueError, match=word):
            train_loop.train_dlwp(model, None, None, save_model=False, **kw)       # refused before the datasets are looked at
