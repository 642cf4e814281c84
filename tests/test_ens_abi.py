"""Host-side refusals of dlwp_ens_perturb / dlwp_ens_diag / dlwp_ens_diag_ws_floats (csrc/ensemble.hip) and of the wrappers in
dlwp_benchmark_amd/ensemble.py and the drivers' ensemble keywords: every call here is rejected before anything touches a GPU, so the
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


def perturb(lib, **kw):
    """a valid call (B 2, two frames of V 3 planes of 35 floats, M 4) with the named arguments replaced"""
    a = dict(x=P, items=P, sigma=P, B=2, F=2 * 3 * 35, P=35, V=3, M=4, control=1, seed=1234, out=P)
    a.update(kw)
    return lib.dlwp_ens_perturb(a["x"], a["items"], a["sigma"], a["B"], a["F"], a["P"], a["V"], a["M"], a["control"], a["seed"], a["out"],
                                None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(x=None), E_INVALID, b"x is NULL"),
    (dict(items=None), E_INVALID, b"items is NULL"),
    (dict(sigma=None), E_INVALID, b"sigma is NULL"),
    (dict(out=None), E_INVALID, b"out is NULL"),
    (dict(B=0), E_INVALID, b"B 0"),
    (dict(F=0), E_INVALID, b"F 0"),
    (dict(P=0), E_INVALID, b"P 0"),
    (dict(V=-1), E_INVALID, b"V -1"),
    (dict(M=0), E_INVALID, b"M 0"),
    (dict(M=65), E_UNSUPPORTED, b"M 65"),
    (dict(F=211), E_INVALID, b"F 211 is not a multiple"),
    (dict(P=300), E_INVALID, b"F 210 is not a multiple"),
    (dict(F=(1 << 34) + 2, P=1), E_UNSUPPORTED, b"noise counter"),          # a multiple of V = 3
    (dict(B=70000), E_UNSUPPORTED, b"B 70000"),
])
def test_perturb_refusals(L, kw, code, word):
    lib = L.load()
    assert perturb(lib, **kw) == code
    assert word in lib.dlwp_last_error(), lib.dlwp_last_error()


def diag(lib, **kw):
    """a valid call (B 2, M 5, T 5, V 3, 8 x 16, dense members) with the named arguments replaced"""
    a = dict(members=P, bs=5 * 5 * 3 * 128, ms=5 * 3 * 128, ts=3 * 128, target=P, roww=None, Bc=2, M=5, Tc=5, V=3, H=8, W=16, t_begin=0, T=5,
             sums=P, ranks=P, ws=P)
    a.update(kw)
    return lib.dlwp_ens_diag(a["members"], a["bs"], a["ms"], a["ts"], a["target"], a["roww"], a["Bc"], a["M"], a["Tc"], a["V"], a["H"],
                             a["W"], a["t_begin"], a["T"], a["sums"], a["ranks"], a["ws"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(members=None), E_INVALID, b"members is NULL"),
    (dict(target=None), E_INVALID, b"target is NULL"),
    (dict(sums=None), E_INVALID, b"sums is NULL"),
    (dict(ranks=None), E_INVALID, b"ranks is NULL"),
    (dict(ws=None), E_INVALID, b"ws is NULL"),
    (dict(Bc=0), E_INVALID, b"Bc 0"),
    (dict(Tc=-1), E_INVALID, b"Tc -1"),
    (dict(V=0), E_INVALID, b"V 0"),
    (dict(H=0), E_INVALID, b"H 0"),
    (dict(W=0), E_INVALID, b"W 0"),
    (dict(T=0, t_begin=0), E_INVALID, b"T 0"),
    (dict(M=1), E_INVALID, b"M 1 members"),
    (dict(M=0), E_INVALID, b"M 0 members"),
    (dict(M=65), E_UNSUPPORTED, b"M 65 members above 64"),
    (dict(bs=-1), E_INVALID, b"batch -1"),
    (dict(ms=-1920), E_INVALID, b"member -1920"),
    (dict(ts=-384), E_INVALID, b"time -384"),
    (dict(t_begin=1), E_INVALID, b"t_begin 1 + Tc 5"),
    (dict(t_begin=-1), E_INVALID, b"t_begin -1"),
    (dict(H=2048, W=2048), E_UNSUPPORTED, b"2048 x 2048"),
    (dict(V=70000), E_UNSUPPORTED, b"V 70000"),
    (dict(Bc=70000), E_UNSUPPORTED, b"Bc 70000"),
])
def test_diag_refusals(L, kw, code, word):
    lib = L.load()
    assert diag(lib, **kw) == code
    assert word in lib.dlwp_last_error(), lib.dlwp_last_error()


def test_knob_and_workspace(L):
    lib = L.load()
    assert "ENS_BUCKET" in L.tuning_knobs()
    # per (sample, frame, variable) and pixel block four sums and M + 1 counts; the blocks are a function of H W only
    assert lib.dlwp_ens_diag_ws_floats(2, 5, 5, 3, 8, 16) == 2 * 5 * 3 * 1 * (5 + 5)
    assert lib.dlwp_ens_diag_ws_floats(1, 64, 1, 8, 32, 64) == 8 * 8 * (64 + 5)                  # 2048 pixels: 8 blocks of 256
    assert lib.dlwp_ens_diag_ws_floats(3, 64, 1, 8, 32, 64) == 3 * lib.dlwp_ens_diag_ws_floats(1, 64, 1, 8, 32, 64)
    assert lib.dlwp_ens_diag_ws_floats(1, 2, 1, 1, 721, 1440) == 254 * (2 + 5)                   # 16 pixels per thread: 254 blocks of 4096
    assert lib.dlwp_ens_diag_ws_floats(0, 5, 5, 3, 8, 16) == E_INVALID and b"Bc 0" in lib.dlwp_last_error()
    assert lib.dlwp_ens_diag_ws_floats(2, 1, 5, 3, 8, 16) == E_INVALID and b"M 1" in lib.dlwp_last_error()
    assert lib.dlwp_ens_diag_ws_floats(2, 65, 5, 3, 8, 16) == E_UNSUPPORTED and b"M 65" in lib.dlwp_last_error()
    assert lib.dlwp_ens_diag_ws_floats(2, 5, 5, 3, 4096, 4096) == E_UNSUPPORTED and b"4096 x 4096" in lib.dlwp_last_error()
    for value, m, code, word in [(7, 5, E_INVALID, b"ENS_BUCKET 7"), (-8, 5, E_INVALID, b"ENS_BUCKET -8"),
                                 (8, 9, E_UNSUPPORTED, b"ENS_BUCKET 8 cannot hold M 9")]:
        L.set_tuning("ENS_BUCKET", value)
        try:
            assert diag(lib, M=m, bs=m * 5 * 3 * 128) == code and word in lib.dlwp_last_error()
        finally:
            L.set_tuning("ENS_BUCKET", None)


def test_wrappers_refuse_on_the_host():
    from dlwp_benchmark_amd import ensemble as E, lib as L
    x = torch.zeros(2, 2, 3, 5, 7)
    with pytest.raises(ValueError, match="members = 0"):
        E.perturb_members(x, [0, 1], 0, 0.1, 1)
    with pytest.raises(ValueError, match="members = 65"):
        E.perturb_members(x, [0, 1], 65, 0.1, 1)
    with pytest.raises(ValueError, match="items must be 2 integers"):
        E.perturb_members(x, [0, 1, 2], 4, 0.1, 1)
    with pytest.raises(ValueError, match="items must be 2 integers"):
        E.perturb_members(x, [0.5, 1.0], 4, 0.1, 1)
    with pytest.raises(ValueError, match="items must lie"):
        E.perturb_members(x, [0, -1], 4, 0.1, 1)
    with pytest.raises(ValueError, match="one entry per variable"):
        E.perturb_members(x, [0, 1], 4, [0.1, 0.2], 1)
    with pytest.raises(ValueError, match="finite and not negative"):
        E.perturb_members(x, [0, 1], 4, [0.1, -0.2, 0.0], 1)
    with pytest.raises(ValueError, match="finite and not negative"):
        E.perturb_members(x, [0, 1], 4, float("inf"), 1)
    with pytest.raises(ValueError, match="needs a seed"):
        E.perturb_members(x, [0, 1], 4, 0.1, None)
    with pytest.raises(ValueError, match="64 unsigned bits"):
        E.perturb_members(x, [0, 1], 4, 0.1, 2 ** 64)
    with pytest.raises(ValueError, match="64 unsigned bits"):
        E.perturb_members(x, [0, 1], 4, 0.1, -1)
    with pytest.raises(ValueError, match="no axis of 4 variables"):
        E.perturb_members(x, [0, 1], 4, 0.1, 1, variables=4)
    with pytest.raises(ValueError, match=r"\[B, \.\.\., V, H, W\]"):
        E.perturb_members(x[0, 0], [0, 1, 2], 4, 0.1, 1)
    with pytest.raises(L.DlwpError):                                   # CPU tensors are refused, never computed on
        E.perturb_members(x, [0, 1], 4, 0.1, 1)
    assert E._layout(torch.zeros(2, 4, 3, 12, 2, 2), None) == (3, 48)              # [..., V, 12, n, n]
    assert E._layout(torch.zeros(2, 4, 12, 2, 2), None) == (4, 48)
    assert E._layout(torch.zeros(2, 4, 12, 2, 2), 12) == (12, 4)                   # ... unless the caller names the variable axis
    assert E._layout(x, None) == (3, 35)

    m, t = torch.zeros(2, 4, 3, 1, 4, 8), torch.zeros(2, 3, 1, 4, 8)
    with pytest.raises(ValueError, match="differ"):
        E.ensemble_diagnostics(m[:, :, :2], t)
    with pytest.raises(ValueError, match=r"\[B, M, T, V, H, W\]"):
        E.ensemble_diagnostics(m[0], t)
    with pytest.raises(ValueError, match="M = 1 members"):
        E.ensemble_diagnostics(m[:, :1], t)
    with pytest.raises(ValueError, match="outside the rollout"):
        E.ensemble_diagnostics(m, t, t_begin=2, T=4)
    with pytest.raises(ValueError, match="lats_deg must have 4"):
        E.ensemble_diagnostics(m, t, lats_deg=np.zeros(5))
    with pytest.raises(L.DlwpError):
        E.ensemble_diagnostics(m, t)
    part = {"sums": torch.zeros(1, 2, 1, 4), "ranks": torch.zeros(1, 2, 1, 5, dtype=torch.int32), "members": 4, "grid": (4, 8), "frames": 2}
    with pytest.raises(ValueError, match="different ensembles"):
        E.concat_ensemble([part, dict(part, members=5)])
    with pytest.raises(ValueError, match="one entry per variable"):
        E.ensemble_metrics(part, scale=[1.0, 2.0])
    both = E.concat_ensemble([part, part])
    assert tuple(both["sums"].shape) == (2, 2, 1, 4) and tuple(both["ranks"].shape) == (2, 2, 1, 5) and both["members"] == 4


def test_drivers_refuse_on_the_host():
    from dlwp_benchmark_amd import evaluate

    class Dataset:
        init_dates = np.array(["2017-01-01"], dtype="datetime64[h]")

    for forecast in ("persistence", "climatology"):
        with pytest.raises(ValueError, match="ensemble needs forecast='model'"):
            evaluate.evaluate_dlwp(None, Dataset(), 2, forecast=forecast, climatology=torch.zeros(12, 1, 4, 8), ensemble=4)
    with pytest.raises(ValueError, match="ensemble = 1 members"):
        evaluate.evaluate_dlwp(None, Dataset(), 2, ensemble=1)
    with pytest.raises(ValueError, match="needs a seed"):
        evaluate.evaluate_dlwp(None, Dataset(), 2, ensemble=4, ensemble_sigma=0.1)
    with pytest.raises(ValueError, match="ensemble = 65 members"):
        evaluate.evaluate_ns(None, [], 2, ensemble=65)
    with pytest.raises(ValueError, match="finite and not negative"):
        evaluate.evaluate_ns(None, [], 2, ensemble=4, ensemble_sigma=-1.0, ensemble_seed=1)
