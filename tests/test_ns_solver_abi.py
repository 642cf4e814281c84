"""dlwp_ns2d_grf / _spectral_terms / _advect / _cn_update on a CPU-only box: NULL operands and bad sizes are refused on the host
with a negative code and a message in dlwp_last_error() that names the argument; nothing is launched (every call below would
fault on its fake pointers otherwise)."""
import ctypes as C
import os

import pytest


@pytest.fixture(scope="module")
def h():
    from dlwp_benchmark_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


FAKE = 0x1000      # a non-NULL pointer value: validation must fail before it is ever dereferenced
F = C.c_float
NAN, INF = float("nan"), float("inf")


def err(h):
    return h.dlwp_last_error().decode()


def grf(h, seed=1, first=0, B=3, n=8, alpha=2.5, tau=7.0, sigma=1.0, H=FAKE):
    return h.dlwp_ns2d_grf(seed, first, B, n, F(alpha), F(tau), F(sigma), H, None)


def terms(h, w_h=FAKE, out=FAKE, B=3, n=8):
    return h.dlwp_ns2d_spectral_terms(w_h, out, B, n, None)


def advect(h, fields=FAKE, out=FAKE, B=3, n=8):
    return h.dlwp_ns2d_advect(fields, out, B, n, None)


def cn(h, w_h=FAKE, F_h=FAKE, f_h=FAKE, f_batched=0, B=3, n=8, dt=1e-2, visc=1e-3):
    return h.dlwp_ns2d_cn_update(w_h, F_h, f_h, f_batched, B, n, F(dt), F(visc), None)


def test_null_pointers_are_refused(h):
    assert grf(h, H=None) == -1 and "H is NULL" in err(h)
    for name in ("w_h", "out"):
        assert terms(h, **{name: None}) == -1 and f"{name} is NULL" in err(h)
    for name in ("fields", "out"):
        assert advect(h, **{name: None}) == -1 and f"{name} is NULL" in err(h)
    for name in ("w_h", "F_h", "f_h"):
        assert cn(h, **{name: None}) == -1 and f"{name} is NULL" in err(h)


@pytest.mark.parametrize("call", [grf, terms, advect, cn])
def test_bad_shapes_are_refused(h, call):
    for n in (7, 2, 0, -8):
        assert call(h, n=n) == -1
        assert f"n {n} must be even and at least 4" in err(h)
    for B in (0, -2):
        assert call(h, B=B) == -1
        assert f"B {B} must be at least 1" in err(h)
    assert call(h, B=2 ** 20, n=4096) == -3 and "too large" in err(h)


def test_grf_refuses_bad_samples_and_parameters(h):
    assert grf(h, first=2 ** 32 - 2, B=3) == -1 and "first_sample" in err(h)
    assert grf(h, first=-1) == -1 and "first_sample" in err(h)
    for name in ("alpha", "tau", "sigma"):
        for bad in (NAN, INF, -INF):
            assert grf(h, **{name: bad}) == -1
            assert name in err(h) and "finite" in err(h)


def test_cn_update_refuses_bad_steps(h):
    for dt in (0.0, -1e-3, NAN, INF):
        assert cn(h, dt=dt) == -1
        assert "dt" in err(h) and "positive" in err(h)
    for visc in (-1.0, NAN, INF):
        assert cn(h, visc=visc) == -1
        assert "visc" in err(h)


def test_misaligned_complex_arrays_are_refused(h):
    assert grf(h, H=FAKE + 4) == -1 and "8-byte aligned" in err(h)
    assert terms(h, out=FAKE + 4) == -1 and "8-byte aligned" in err(h)
    assert cn(h, F_h=FAKE + 4) == -1 and "8-byte aligned" in err(h)
