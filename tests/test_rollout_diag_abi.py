"""Host-side refusals of dlwp_rollout_diag / dlwp_rollout_diag_ws_floats / dlwp_group_mean (csrc/rollout_diag.hip) and of their
wrappers in evaluate.py: every call here is rejected before anything touches a GPU, so the checks run on a CPU-only box."""
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


def diag(lib, **kw):
    """a valid lat-lon call (B 2, T 5, V 3, 8 x 16, clim with 12 maps, window [1, 4)) with the named arguments replaced"""
    a = dict(out=P, bs=5 * 3 * 128, ts=3 * 128, target=P, scale=P, shift=P, roww=P, clim=P, month=P, M=12, idx=None, w=None, n=0,
             Bc=2, Tc=5, V=3, H=8, W=16, t_begin=0, T=5, w0=1, w1=4, moments=P, zonal=P, wsum=P, ws=P)
    a.update(kw)
    return lib.dlwp_rollout_diag(a["out"], a["bs"], a["ts"], a["target"], a["scale"], a["shift"], a["roww"], a["clim"], a["month"], a["M"],
                                 a["idx"], a["w"], a["n"], a["Bc"], a["Tc"], a["V"], a["H"], a["W"], a["t_begin"], a["T"], a["w0"], a["w1"],
                                 a["moments"], a["zonal"], a["wsum"], a["ws"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(target=None), E_INVALID, b"target is NULL"),
    (dict(moments=None), E_INVALID, b"moments is NULL"),
    (dict(zonal=None), E_INVALID, b"zonal is NULL"),
    (dict(wsum=None), E_INVALID, b"wsum is NULL"),
    (dict(ws=None), E_INVALID, b"ws is NULL"),
    (dict(idx=P), E_INVALID, b"idx and w"),                    # half a table
    (dict(Bc=0), E_INVALID, b"Bc 0"),
    (dict(Tc=-1), E_INVALID, b"Tc -1"),
    (dict(V=0), E_INVALID, b"V 0"),
    (dict(H=0), E_INVALID, b"H 0"),
    (dict(W=0), E_INVALID, b"W 0"),
    (dict(T=0), E_INVALID, b"T 0"),
    (dict(idx=P, w=P, n=0), E_INVALID, b"nside"),
    (dict(bs=-1), E_INVALID, b"batch -1"),
    (dict(ts=-384), E_INVALID, b"time -384"),
    (dict(month=None), E_INVALID, b"clim and month"),
    (dict(clim=None), E_INVALID, b"clim and month"),
    (dict(M=0), E_INVALID, b"M 0"),
    (dict(out=None, clim=None, month=None), E_INVALID, b"out is NULL"),
    (dict(w0=-1), E_INVALID, b"window [-1, 4)"),
    (dict(w1=6), E_INVALID, b"window [1, 6)"),
    (dict(w0=4, w1=3), E_INVALID, b"window [4, 3)"),
    (dict(t_begin=1), E_INVALID, b"t_begin 1 + Tc 5"),
    (dict(t_begin=-1), E_INVALID, b"t_begin -1"),
    (dict(idx=P + 4, w=P, n=2), E_INVALID, b"aligned"),
    (dict(idx=P, w=P + 8, n=2), E_INVALID, b"aligned"),
    (dict(W=513), E_UNSUPPORTED, b"W 513"),
    (dict(V=70000), E_UNSUPPORTED, b"V 70000"),
    (dict(Bc=70000, T=5), E_UNSUPPORTED, b"Bc 70000"),
    (dict(idx=P, w=P, n=9000), E_UNSUPPORTED, b"n 9000"),
])
def test_rollout_diag_refusals(L, kw, code, word):
    lib = L.load()
    assert diag(lib, **kw) == code
    assert word in lib.dlwp_last_error(), lib.dlwp_last_error()


def test_forced_paths(L):
    lib = L.load()
    assert "DIAG_PATH" in L.tuning_knobs()
    L.set_tuning("DIAG_PATH", 1)
    try:        # HPX32: two planes of 12288 floats are 96 KiB
        assert diag(lib, idx=P, w=P, n=32) == E_UNSUPPORTED and b"LDS" in lib.dlwp_last_error()
    finally:
        L.set_tuning("DIAG_PATH", None)
    L.set_tuning("DIAG_PATH", 5)
    try:
        assert diag(lib) == E_INVALID and b"DIAG_PATH" in lib.dlwp_last_error()
    finally:
        L.set_tuning("DIAG_PATH", None)


def test_workspace_size(L):
    lib = L.load()
    # 32 x 64 lat-lon: one row per wave, 32 wave slots; HPX: two rows per wave, 16 slots; five partials per slot
    assert lib.dlwp_rollout_diag_ws_floats(2, 5, 3, 32, 64, 0) == 2 * 5 * 3 * 32 * 5
    assert lib.dlwp_rollout_diag_ws_floats(2, 5, 3, 32, 64, 1) == 2 * 5 * 3 * 16 * 5
    assert lib.dlwp_rollout_diag_ws_floats(2, 5, 3, 32, 256, 1) == 2 * 5 * 3 * 32 * 5            # wide rows: one row per wave
    assert lib.dlwp_rollout_diag_ws_floats(1, 1, 1, 5, 12, 0) == 8 * 5              # a partial row block still has four waves
    assert lib.dlwp_rollout_diag_ws_floats(0, 5, 3, 32, 64, 0) == E_INVALID and b"Bc 0" in lib.dlwp_last_error()
    assert lib.dlwp_rollout_diag_ws_floats(2, 5, 3, 32, 600, 0) == E_UNSUPPORTED and b"W 600" in lib.dlwp_last_error()


def test_group_mean_refusals(L):
    lib = L.load()
    assert lib.dlwp_group_mean(None, P, P, P, 4, 8, 12, None) == E_INVALID and b"frames is NULL" in lib.dlwp_last_error()
    assert lib.dlwp_group_mean(P, None, P, P, 4, 8, 12, None) == E_INVALID and b"group is NULL" in lib.dlwp_last_error()
    assert lib.dlwp_group_mean(P, P, None, P, 4, 8, 12, None) == E_INVALID and b"mean is NULL" in lib.dlwp_last_error()
    assert lib.dlwp_group_mean(P, P, P, None, 4, 8, 12, None) == E_INVALID and b"count is NULL" in lib.dlwp_last_error()
    assert lib.dlwp_group_mean(P, P, P, P, 0, 8, 12, None) == E_INVALID and b"N 0" in lib.dlwp_last_error()
    assert lib.dlwp_group_mean(P, P, P, P, 4, 0, 12, None) == E_INVALID and b"P 0" in lib.dlwp_last_error()
    assert lib.dlwp_group_mean(P, P, P, P, 4, 8, 0, None) == E_INVALID and b"G 0" in lib.dlwp_last_error()
    assert lib.dlwp_group_mean(P, P, P, P, 4, 8, 65, None) == E_UNSUPPORTED and b"G 65" in lib.dlwp_last_error()


def test_wrappers_refuse_on_the_host():
    from dlwp_benchmark_amd import evaluate, lib as L
    o, t = torch.zeros(2, 3, 1, 4, 8), torch.zeros(2, 3, 1, 4, 8)
    with pytest.raises(ValueError, match="differ"):
        evaluate.rollout_diagnostics(o[:, :2], t)
    with pytest.raises(ValueError, match="climatology"):
        evaluate.rollout_diagnostics(None, t)
    with pytest.raises(ValueError, match="go together"):
        evaluate.rollout_diagnostics(o, t, climatology=torch.zeros(12, 1, 4, 8))
    with pytest.raises(ValueError, match="outside the rollout"):
        evaluate.rollout_diagnostics(o, t, t_begin=2, T=4)
    with pytest.raises(ValueError, match="window"):
        evaluate.rollout_diagnostics(o, t, window=(2, 5))
    with pytest.raises(ValueError, match=r"0\.\.11"):
        evaluate.rollout_diagnostics(o, t, climatology=torch.zeros(12, 1, 4, 8), months=np.full((2, 3), 12))
    with pytest.raises(ValueError, match="integers"):
        evaluate.rollout_diagnostics(o, t, climatology=torch.zeros(12, 1, 4, 8), months=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="one entry per variable"):
        evaluate.rollout_diagnostics(o, t, scale=[1.0, 2.0])
    with pytest.raises(L.DlwpError):                                   # CPU tensors are refused, never computed on
        evaluate.rollout_diagnostics(o, t)
    with pytest.raises(ValueError, match=r"0\.\.11"):
        evaluate.monthly_climatology(torch.zeros(3, 4), np.array([0, 12, 1]))
    with pytest.raises(L.DlwpError):
        evaluate.monthly_climatology(torch.zeros(3, 4), np.array([0, 1, 1]))
    with pytest.raises(ValueError, match="forecast"):
        evaluate.evaluate_dlwp(None, None, 2, forecast="analog")
