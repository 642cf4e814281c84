"""Host-side refusals of the remap entry points (csrc/hpx_remap.hip) and of hpx_remap.HEALPixRemap: every call here is rejected
before anything touches a GPU, so the checks run on a CPU-only box."""
import pytest


@pytest.fixture(scope="module")
def L():
    from dlwp_benchmark_amd import lib
    lib.load()
    return lib


def test_gather_refusals(L):
    lib, P = L.load(), 4096          # (a non-NULL, 16-byte aligned pointer value: never dereferenced, the calls are refused first)
    assert lib.dlwp_remap_gather4(P, 768, None, P, P, 2, 768, 2048, None) == -1 and b"NULL" in lib.dlwp_last_error()
    assert lib.dlwp_remap_gather4(P, 768, P, P, P, 0, 768, 2048, None) == -1 and b"positive" in lib.dlwp_last_error()
    assert lib.dlwp_remap_gather4(P, 768, P, P, P, 2, 768, 0, None) == -1
    assert lib.dlwp_remap_gather4(P, 700, P, P, P, 2, 768, 2048, None) == -1 and b"stride" in lib.dlwp_last_error()
    assert lib.dlwp_remap_gather4(P, 768, P + 4, P, P, 2, 768, 2048, None) == -1 and b"aligned" in lib.dlwp_last_error()
    L.set_tuning("REMAP_PATH", 1)
    try:
        assert lib.dlwp_remap_gather4(P, 49152, P, P, P, 1, 49152, 2048, None) == -3 and b"LDS" in lib.dlwp_last_error()
    finally:
        L.set_tuning("REMAP_PATH", None)
    L.set_tuning("REMAP_PATH", 7)
    try:
        assert lib.dlwp_remap_gather4(P, 768, P, P, P, 2, 768, 2048, None) == -1 and b"REMAP_PATH" in lib.dlwp_last_error()
    finally:
        L.set_tuning("REMAP_PATH", None)


def test_csr_and_moments_refusals(L):
    lib, P = L.load(), 4096
    assert lib.dlwp_remap_csr(P, None, P, P, P, 2, 2048, 768, 0, None) == -1 and b"NULL" in lib.dlwp_last_error()
    assert lib.dlwp_remap_csr(P, P, P, P, P, 0, 2048, 768, 0, None) == -1 and b"positive" in lib.dlwp_last_error()
    assert lib.dlwp_remap_csr(P, P, P, P, P, 2, 0, 768, 0, None) == -1
    assert lib.dlwp_hpx_error_moments(P, P, None, None, None, P, 1, 1, 8, 32, 64, P, None) == -1 and b"NULL" in lib.dlwp_last_error()
    assert lib.dlwp_hpx_error_moments(P, P, None, None, P, P, 0, 1, 8, 32, 64, P, None) == -1 and b"positive" in lib.dlwp_last_error()
    assert lib.dlwp_hpx_error_moments(P, P, None, None, P, P, 1, 1, 9000, 32, 64, P, None) == -3
    knobs = L.tuning_knobs()
    assert "REMAP_PATH" in knobs


def test_module_refuses_cpu_and_other_orders():
    import torch
    from dlwp_benchmark_amd import lib as L
    from dlwp_benchmark_amd.hpx_remap import HEALPixRemap, _planes
    with pytest.raises(NotImplementedError):
        HEALPixRemap(latitudes=32, longitudes=64, nside=8, order="bicubic", device="cuda")
    with pytest.raises(L.DlwpError):
        HEALPixRemap(latitudes=32, longitudes=64, nside=8, device="cpu")
    with pytest.raises(ValueError):
        HEALPixRemap(latitudes=32, longitudes=64)
    # plane views: dense planes behind one collapsible stride are read in place, anything else through a copy
    x = torch.zeros(6, 2, 32, 64)
    assert _planes(x, 2048)[1:] == (12, 2048) and _planes(x, 2048)[0] is x
    v = x[:, 1]
    assert _planes(v, 2048)[1:] == (6, 4096) and _planes(v, 2048)[0] is v
    for w in (x[:, :, ::2], x.permute(1, 0, 2, 3), x.expand(3, 6, 2, 32, 64)):
        src, planes, stride = _planes(w, w.shape[-1] * w.shape[-2])
        assert src.is_contiguous() and stride == w.shape[-1] * w.shape[-2] and planes == w.numel() // stride
