"""Host-side refusals of dlwp_sphere_spectra / dlwp_plane_spectra, their _ws_floats (csrc/spectra.hip) and the wrappers in
dlwp_benchmark_amd/spectra.py: every call here is rejected before anything touches a GPU, so the checks run on a CPU-only box."""
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


def sphere(lib, **kw):
    """a valid lat-lon call (B 2, T 5, V 3, 8 x 16, L 8, M 8) with the named arguments replaced"""
    a = dict(out=P, bs=5 * 3 * 128, ts=3 * 128, target=P, F=P, Wf=P, idx=None, w=None, n=0, Bc=2, Tc=5, V=3, H=8, W=16, L=8, M=8,
             t_begin=0, T=5, power=P, cross=P, a00=P, ws=P)
    a.update(kw)
    return lib.dlwp_sphere_spectra(a["out"], a["bs"], a["ts"], a["target"], a["F"], a["Wf"], a["idx"], a["w"], a["n"], a["Bc"], a["Tc"],
                                   a["V"], a["H"], a["W"], a["L"], a["M"], a["t_begin"], a["T"], a["power"], a["cross"], a["a00"], a["ws"],
                                   None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(target=None), E_INVALID, b"target is NULL"),
    (dict(F=None), E_INVALID, b"F is NULL"),
    (dict(Wf=None), E_INVALID, b"Wf is NULL"),
    (dict(power=None), E_INVALID, b"power is NULL"),
    (dict(cross=None), E_INVALID, b"cross is NULL"),
    (dict(a00=None), E_INVALID, b"a00 is NULL"),
    (dict(ws=None), E_INVALID, b"ws is NULL"),
    (dict(idx=P), E_INVALID, b"idx and w"),                    # half a table
    (dict(w=P), E_INVALID, b"idx and w"),
    (dict(Bc=0), E_INVALID, b"Bc 0"),
    (dict(Tc=-1), E_INVALID, b"Tc -1"),
    (dict(V=0), E_INVALID, b"V 0"),
    (dict(H=0), E_INVALID, b"H 0"),
    (dict(W=0), E_INVALID, b"W 0"),
    (dict(L=0), E_INVALID, b"L 0"),
    (dict(M=0), E_INVALID, b"M 0"),
    (dict(T=0), E_INVALID, b"T 0"),
    (dict(L=9), E_INVALID, b"L 9 degrees above H 8"),
    (dict(M=9, L=8), E_INVALID, b"M 9 orders above W / 2 = 8"),
    (dict(H=257, L=8), E_UNSUPPORTED, b"H 257"),
    (dict(W=514), E_UNSUPPORTED, b"W 514"),
    (dict(idx=P, w=P, n=0), E_INVALID, b"nside"),
    (dict(idx=P, w=P, n=9000), E_UNSUPPORTED, b"n 9000"),
    (dict(idx=P + 4, w=P, n=2), E_INVALID, b"aligned"),
    (dict(idx=P, w=P + 8, n=2), E_INVALID, b"aligned"),
    (dict(bs=-1), E_INVALID, b"batch -1"),
    (dict(ts=-384), E_INVALID, b"time -384"),
    (dict(t_begin=1), E_INVALID, b"t_begin 1 + Tc 5"),
    (dict(t_begin=-1), E_INVALID, b"t_begin -1"),
    (dict(V=70000), E_UNSUPPORTED, b"V 70000"),
    (dict(Bc=70000), E_UNSUPPORTED, b"Bc 70000"),
])
def test_sphere_spectra_refusals(L, kw, code, word):
    lib = L.load()
    assert sphere(lib, **kw) == code
    assert word in lib.dlwp_last_error(), lib.dlwp_last_error()


def test_sphere_knobs_and_workspace(L):
    lib = L.load()
    knobs = L.tuning_knobs()
    assert "SPEC_MB" in knobs and "SPEC_RB" in knobs and "SPEC_HPX" in knobs
    # every order in one block: no fold, a token workspace; a forced block of 3 of 8 orders: three blocks of [3][L] sums per field
    assert lib.dlwp_sphere_spectra_ws_floats(2, 5, 3, 8, 16, 8, 8, 0) == 1
    assert lib.dlwp_sphere_spectra_ws_floats(2, 5, 3, 32, 64, 32, 32, 8) == 1
    L.set_tuning("SPEC_MB", 3)
    try:
        assert lib.dlwp_sphere_spectra_ws_floats(2, 5, 3, 8, 16, 8, 8, 0) == 2 * 5 * 3 * 3 * 3 * 8
    finally:
        L.set_tuning("SPEC_MB", None)
    # the largest grid: the tables of all 256 orders do not fit, the blocks shrink by themselves (at least 16 blocks)
    n = lib.dlwp_sphere_spectra_ws_floats(1, 1, 1, 256, 512, 256, 256, 0)
    assert n > 1 and n % (3 * 256) == 0 and n // (3 * 256) >= 16
    assert lib.dlwp_sphere_spectra_ws_floats(0, 5, 3, 8, 16, 8, 8, 0) == E_INVALID and b"Bc 0" in lib.dlwp_last_error()
    assert lib.dlwp_sphere_spectra_ws_floats(2, 5, 3, 8, 16, 9, 8, 0) == E_INVALID and b"L 9" in lib.dlwp_last_error()
    assert lib.dlwp_sphere_spectra_ws_floats(2, 5, 3, 8, 600, 8, 8, 0) == E_UNSUPPORTED and b"W 600" in lib.dlwp_last_error()
    assert lib.dlwp_sphere_spectra_ws_floats(2, 5, 3, 8, 16, 8, 8, -1) == E_INVALID and b"nside" in lib.dlwp_last_error()
    for knob, value, code, word in [("SPEC_HPX", 3, E_INVALID, b"SPEC_HPX 3"), ("SPEC_MB", -1, E_INVALID, b"SPEC_MB -1")]:
        L.set_tuning(knob, value)
        try:
            assert sphere(lib) == code and word in lib.dlwp_last_error()
        finally:
            L.set_tuning(knob, None)
    L.set_tuning("SPEC_HPX", 1)
    try:        # HPX32: two planes of 12288 floats are 96 KiB
        assert sphere(lib, idx=P, w=P, n=32) == E_UNSUPPORTED and b"LDS" in lib.dlwp_last_error()
    finally:
        L.set_tuning("SPEC_HPX", None)
    L.set_tuning("SPEC_MB", 256)
    L.set_tuning("SPEC_RB", 256)
    try:        # forced blocks that cannot fit are refused, not shrunk
        assert sphere(lib, H=256, W=512, L=256, M=256) == E_UNSUPPORTED and b"bytes of LDS" in lib.dlwp_last_error()
    finally:
        L.set_tuning("SPEC_MB", None)
        L.set_tuning("SPEC_RB", None)


def plane(lib, **kw):
    """a valid call (B 2, T 5, D 1, 12 x 20: 13 shells, 132 entries) with the named arguments replaced"""
    a = dict(plan=P, out=P, bs=5 * 240, ts=240, target=P, rowptr=P, entry=P, weight=P, K=13, nnz=132, Bc=2, Tc=5, D=1, H=12, W=20,
             t_begin=0, T=5, power=P, cross=P, ws=P)
    a.update(kw)
    return lib.dlwp_plane_spectra(a["plan"], a["out"], a["bs"], a["ts"], a["target"], a["rowptr"], a["entry"], a["weight"], a["K"],
                                  a["nnz"], a["Bc"], a["Tc"], a["D"], a["H"], a["W"], a["t_begin"], a["T"], a["power"], a["cross"], a["ws"],
                                  None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(plan=None), E_INVALID, b"plan is NULL"),
    (dict(target=None), E_INVALID, b"target is NULL"),
    (dict(rowptr=None), E_INVALID, b"rowptr is NULL"),
    (dict(entry=None), E_INVALID, b"entry is NULL"),
    (dict(weight=None), E_INVALID, b"weight is NULL"),
    (dict(power=None), E_INVALID, b"power is NULL"),
    (dict(cross=None), E_INVALID, b"cross is NULL"),
    (dict(ws=None), E_INVALID, b"ws is NULL"),
    (dict(Bc=0), E_INVALID, b"Bc 0"),
    (dict(Tc=0), E_INVALID, b"Tc 0"),
    (dict(D=-2), E_INVALID, b"D -2"),
    (dict(H=0), E_INVALID, b"H 0"),
    (dict(W=1), E_INVALID, b"W 1"),
    (dict(K=0), E_INVALID, b"K 0"),
    (dict(nnz=0), E_INVALID, b"nnz 0"),
    (dict(T=0), E_INVALID, b"T 0"),
    (dict(bs=-1), E_INVALID, b"batch -1"),
    (dict(ts=-240), E_INVALID, b"time -240"),
    (dict(t_begin=3), E_INVALID, b"t_begin 3 + Tc 5"),
    (dict(t_begin=-1), E_INVALID, b"t_begin -1"),
    (dict(Bc=70000, Tc=70000), E_UNSUPPORTED, b"fields"),
])
def test_plane_spectra_refusals(L, kw, code, word):
    lib = L.load()
    assert plane(lib, **kw) == code
    assert word in lib.dlwp_last_error(), lib.dlwp_last_error()


def test_plane_workspace(L):
    lib = L.load()
    assert lib.dlwp_plane_spectra_ws_floats(2, 5, 1, 12, 20) == 2 * (2 * 5 * 1) * 12 * 11 * 2
    assert lib.dlwp_plane_spectra_ws_floats(2, 5, 1, 9, 14) == 2 * 10 * 9 * 8 * 2
    assert lib.dlwp_plane_spectra_ws_floats(2, 0, 1, 12, 20) == E_INVALID and b"Tc 0" in lib.dlwp_last_error()
    assert lib.dlwp_plane_spectra_ws_floats(2, 5, 1, 12, 1) == E_INVALID and b"W 1" in lib.dlwp_last_error()


def test_wrappers_refuse_on_the_host():
    from dlwp_benchmark_amd import spectra, lib as L
    o, t = torch.zeros(2, 3, 1, 4, 8), torch.zeros(2, 3, 1, 4, 8)
    with pytest.raises(ValueError, match="differ"):
        spectra.sphere_spectra(o[:, :2], t)
    with pytest.raises(ValueError, match=r"\[B, T, V, H, W\]"):
        spectra.sphere_spectra(None, t[0])
    with pytest.raises(ValueError, match="outside the rollout"):
        spectra.sphere_spectra(o, t, t_begin=2, T=4)
    with pytest.raises(ValueError, match="grid must be"):
        spectra.sphere_spectra(o, t, grid="lobatto")
    with pytest.raises(ValueError, match="lmax = 5"):
        spectra.sphere_spectra(o, t, lmax=5)
    with pytest.raises(ValueError, match="300 x 8"):
        spectra.sphere_spectra(None, torch.zeros(1, 1, 1, 300, 8))
    with pytest.raises(L.DlwpError):                                   # CPU tensors are refused, never computed on
        spectra.sphere_spectra(o, t)
    with pytest.raises(ValueError, match="differ"):
        spectra.plane_spectra(o[:, :2], t)
    with pytest.raises(ValueError, match=r"\[B, T, D, H, W\]"):
        spectra.plane_spectra(None, t[0])
    with pytest.raises(ValueError, match="outside the rollout"):
        spectra.plane_spectra(o, t, t_begin=-1)
    with pytest.raises(L.DlwpError):
        spectra.plane_spectra(o, t)
    with pytest.raises(ValueError, match="n = 0"):
        spectra.fejer1_weights(0)
    with pytest.raises(ValueError, match="grid must be"):
        spectra.sphere_tables(8, 16, "lobatto")
    from dlwp_benchmark_amd import sht
    with pytest.raises(NotImplementedError):                           # sht's own refusal of other grid names is untouched
        sht.sht_tables(8, 16, 8, 8, "midpoint")
    assert np.isclose(spectra.fejer1_weights(7)[1].sum(), 2.0)
