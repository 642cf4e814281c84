"""csrc/hpx_remap.hip on the MI355X: dlwp_remap_gather4 (both kernels, pinned through lib.kernel_accounting), its adjoint
dlwp_remap_csr, the autograd surface of hpx_remap.HEALPixRemap, the fused dlwp_hpx_error_moments behind evaluate.dlwp_metrics_hpx,
the host-side refusals, and the chain lat-lon record -> remap_fields -> WeatherBenchArrays -> ConvLSTMHPX -> dlwp_metrics_hpx.

Every source sits in a buffer followed by GUARD planes of NaN (a lane that reads past its plane tile shows as NaN), every result in
a buffer followed by GUARD planes of a sentinel bit pattern that must come back untouched.

Bounds (from the arithmetic, not from results).  Gather: four products and three additions of a convex combination, each rounded
once: |err| <= 7 * 2^-24 max|src| < 1e-6 max|src| against the float64 sum with the same float32-rounded weights.  Adjoint: a row of
len_r entries is len_r products and len_r additions in fp32, in whatever fixed order (eight ascending strided partial sums and a
three-level combine are shallower than one chain): |err_r| <= (len_r + 1) * 2^-24 * sum_e |val_e| * max|g|, asserted with a factor 2;
an accumulating call adds one more rounding of the result.  Two runs are bit-identical (fixed order, no atomics).  Fused moments: the tolerances tests/test_gpu_evaluate.py uses for the same reduction (rmse rtol 2e-5, acc atol 2e-5)."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import hpx_remap_ref as R
from oracle import eval_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 8), (2, 8, 16), (8, 32, 64)]
PLANES = [1, 3, 130]           # 130: more than one plane tile (16, 9 or 8 planes) and not a multiple of one
GUARD = 2
SENT = 0x4B1DFACE
U24 = 2.0 ** -24
E_INVALID, E_UNSUPPORTED = -1, -3


@contextlib.contextmanager
def knobs(**kw):
    from dlwp_benchmark_amd import lib as L
    try:
        for k, v in kw.items():
            L.set_tuning(k, v)
        yield
    finally:
        for k in kw:
            L.set_tuning(k, None)


def launched(fn):
    """the accounting names of one eager call"""
    from dlwp_benchmark_amd import lib as L
    with L.kernel_accounting() as acc:
        fn()
        torch.cuda.synchronize()
    return sorted(r["name"] for r in acc.rows)


@functools.lru_cache(maxsize=None)
def tables(direction, n, H, W):
    """(idx int32, w float32, (rowptr, col, val float32), n_in, n_out) of one direction: the float32-rounded weights the device holds"""
    from dlwp_benchmark_amd import hpx_geometry as G
    lats, lons = R.regular_grid(H, W)
    idx, w = (G.ll2hpx_table if direction == "ll2hpx" else G.hpx2ll_table)(lats, lons, n)
    n_in = H * W if direction == "ll2hpx" else 12 * n * n
    rowptr, col, val = G.transpose_csr(idx, w, n_in)
    return idx, w.astype(np.float32), (rowptr, col, val.astype(np.float32)), n_in, idx.shape[0]


def guarded_src(x, dev):
    """x [planes, n] float32 numpy -> the first `planes` rows of a device buffer whose GUARD further rows are NaN"""
    buf = torch.full((x.shape[0] + GUARD, x.shape[1]), float("nan"), device=dev)
    buf[:x.shape[0]] = torch.from_numpy(x).to(dev)
    return buf


def canary_dst(planes, n, dev):
    return torch.full((planes + GUARD, n), SENT, dtype=torch.int32, device=dev).view(torch.float32)


def check_canary(buf, planes):
    assert (buf[planes:].view(torch.int32) == SENT).all(), "the planes behind the result were written"
    assert not (buf[:planes].view(torch.int32) == SENT).any(), "part of the result was not written"


def dev_tables(direction, n, H, W, dev):
    idx, w32, (rowptr, col, val32), n_in, n_out = tables(direction, n, H, W)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    return up(idx), up(w32), up(rowptr), up(col), up(val32)


def run_gather(direction, n, H, W, src, planes, stride, dev):
    from dlwp_benchmark_amd import lib as L
    idx, w32, _, n_in, n_out = tables(direction, n, H, W)
    d_idx, d_w, _, _, _ = dev_tables(direction, n, H, W, dev)
    dst = canary_dst(planes, n_out, dev)
    names = launched(lambda: L.check(L.load().dlwp_remap_gather4(src.data_ptr(), stride, d_idx.data_ptr(), d_w.data_ptr(), dst.data_ptr(),
                                                                 planes, n_in, n_out, L.stream())))
    check_canary(dst, planes)
    return dst[:planes].cpu().numpy(), names


@pytest.mark.parametrize("path", ["auto", "direct"])
@pytest.mark.parametrize("planes", PLANES)
@pytest.mark.parametrize("n,H,W", SHAPES)
@pytest.mark.parametrize("direction", ["ll2hpx", "hpx2ll"])
def test_gather(cuda, direction, n, H, W, planes, path):
    idx, w32, _, n_in, n_out = tables(direction, n, H, W)
    x = np.random.default_rng(planes * 131 + n).standard_normal((planes, n_in)).astype(np.float32)
    src = guarded_src(x, cuda)
    with knobs(**({"REMAP_PATH": 2} if path == "direct" else {})):
        got, names = run_gather(direction, n, H, W, src, planes, n_in, cuda)
    assert names == ["remap_gather4_direct" if path == "direct" else "remap_gather4_lds"]
    ref = R.apply_table(idx, w32, x)
    err = np.abs(got - ref).max()
    print(f"{direction} n={n} {H}x{W} planes={planes} {path}: max |err| {err:.2e} (bound {1e-6 * np.abs(x).max():.2e})")
    assert err <= 1e-6 * np.abs(x).max()


def test_gather_forced_lds_equals_auto(cuda):
    idx, w32, _, n_in, n_out = tables("hpx2ll", 8, 32, 64)
    x = np.random.default_rng(7).standard_normal((5, n_in)).astype(np.float32)
    src = guarded_src(x, cuda)
    auto, names = run_gather("hpx2ll", 8, 32, 64, src, 5, n_in, cuda)
    with knobs(REMAP_PATH=1):
        forced, names1 = run_gather("hpx2ll", 8, 32, 64, src, 5, n_in, cuda)
    assert names == names1 == ["remap_gather4_lds"]
    np.testing.assert_array_equal(auto, forced)


@pytest.mark.parametrize("path", ["auto", "direct"])
@pytest.mark.parametrize("direction", ["ll2hpx", "hpx2ll"])
def test_gather_strided_source(cuda, direction, path):
    """x[:, 1] of a [B, 2, plane] tensor is read in place: plane stride 2 n_in; the other half is NaN"""
    n, H, W, B = 8, 32, 64, 19
    idx, w32, _, n_in, n_out = tables(direction, n, H, W)
    x = np.random.default_rng(11).standard_normal((B, n_in)).astype(np.float32)
    full = torch.full((B + GUARD, 2, n_in), float("nan"), device=cuda)
    full[:B, 1] = torch.from_numpy(x).to(cuda)
    view = full[:B, 1]
    with knobs(**({"REMAP_PATH": 2} if path == "direct" else {})):
        got, names = run_gather(direction, n, H, W, view, B, 2 * n_in, cuda)
    assert names == ["remap_gather4_direct" if path == "direct" else "remap_gather4_lds"]
    assert np.abs(got - R.apply_table(idx, w32, x)).max() <= 1e-6 * np.abs(x).max()


def test_gather_natural_direct_path(cuda):
    """HPX64 planes (192 KB) do not fit LDS: the dispatcher takes the direct kernel by itself"""
    n, H, W, planes = 64, 32, 64, 2
    idx, w32, _, n_in, n_out = tables("hpx2ll", n, H, W)
    x = np.random.default_rng(13).standard_normal((planes, n_in)).astype(np.float32)
    got, names = run_gather("hpx2ll", n, H, W, guarded_src(x, cuda), planes, n_in, cuda)
    assert names == ["remap_gather4_direct"]
    assert np.abs(got - R.apply_table(idx, w32, x)).max() <= 1e-6 * np.abs(x).max()


def adjoint_ref(direction, n, H, W, g):
    """float64 R^T g and the per-row bound of the module docstring (without the factor 2)"""
    _, _, (rowptr, col, val32), n_in, n_out = tables(direction, n, H, W)
    lens = np.diff(rowptr)
    rows = np.repeat(np.arange(n_in), lens)
    val = val32.astype(np.float64)
    bound = (lens + 1) * U24 * np.bincount(rows, weights=np.abs(val), minlength=n_in) * np.abs(g).max()
    g64 = np.asarray(g, dtype=np.float64)
    return np.stack([np.bincount(rows, weights=g64[p, col] * val, minlength=n_in) for p in range(g.shape[0])]), bound


def run_csr(direction, n, H, W, g, accumulate, dev, prefill=None):
    from dlwp_benchmark_amd import lib as L
    _, _, _, n_in, n_out = tables(direction, n, H, W)
    _, _, d_rowptr, d_col, d_val = dev_tables(direction, n, H, W, dev)
    planes = g.shape[0]
    src = guarded_src(g, dev)
    dst = canary_dst(planes, n_in, dev)
    if prefill is not None:
        dst[:planes] = torch.from_numpy(prefill).to(dev)
    names = launched(lambda: L.check(L.load().dlwp_remap_csr(src.data_ptr(), d_rowptr.data_ptr(), d_col.data_ptr(), d_val.data_ptr(),
                                                             dst.data_ptr(), planes, n_out, n_in, accumulate, L.stream())))
    assert names == ["remap_csr"]
    check_canary(dst, planes)
    return dst[:planes].cpu().numpy()


@pytest.mark.parametrize("planes", PLANES + [2])      # tiles of 1, 2 and (two lanes per row) 4 planes: every staged instantiation
@pytest.mark.parametrize("n,H,W", SHAPES)
@pytest.mark.parametrize("direction", ["ll2hpx", "hpx2ll"])
def test_adjoint(cuda, direction, n, H, W, planes):
    _, _, _, n_in, n_out = tables(direction, n, H, W)
    g = np.random.default_rng(planes * 17 + n).standard_normal((planes, n_out)).astype(np.float32)
    ref, bound = adjoint_ref(direction, n, H, W, g)
    got = run_csr(direction, n, H, W, g, 0, cuda)
    again = run_csr(direction, n, H, W, g, 0, cuda)
    np.testing.assert_array_equal(got.view(np.int32), again.view(np.int32))
    ratio = (np.abs(got - ref) / np.maximum(bound, 1e-300)).max()
    print(f"adjoint {direction} n={n} {H}x{W} planes={planes}: max err / bound {ratio:.3f} (allowed 2)")
    assert (np.abs(got - ref) <= 2 * bound).all()
    if planes == 3:                                                            # accumulate: dst += R^T g
        pre = np.random.default_rng(3).standard_normal((planes, n_in)).astype(np.float32)
        acc = run_csr(direction, n, H, W, g, 1, cuda, prefill=pre)
        assert (np.abs(acc - (pre + ref)) <= 2 * bound + 2 * U24 * np.abs(pre + ref).max()).all()


@pytest.mark.parametrize("H,W", [(32, 64), (256, 512)])
def test_adjoint_of_planes_beyond_lds(cuda, H, W):
    """the adjoint of ll2hpx at HPX64 reads 192 KB planes from global memory (the unstaged instantiations: rows of 96 entries on
    average from 32 x 64, of 1.5 from 256 x 512)"""
    n, planes = 64, 2
    _, _, _, n_in, n_out = tables("ll2hpx", n, H, W)
    g = np.random.default_rng(23).standard_normal((planes, n_out)).astype(np.float32)
    ref, bound = adjoint_ref("ll2hpx", n, H, W, g)
    got = run_csr("ll2hpx", n, H, W, g, 0, cuda)
    assert (np.abs(got - ref) <= 2 * bound).all()


@pytest.fixture(scope="module")
def remap8(cuda):
    from dlwp_benchmark_amd.hpx_remap import HEALPixRemap
    return HEALPixRemap(latitudes=32, longitudes=64, nside=8, device=cuda)


@pytest.mark.parametrize("lead", [(2, 3), (2, 1, 3), (2, 1, 2, 1, 3)])
@pytest.mark.parametrize("direction", ["ll2hpx", "hpx2ll"])
def test_autograd_and_leading_axes(cuda, remap8, direction, lead):
    idx, w32, _, n_in, n_out = tables(direction, 8, 32, 64)
    shape_in, shape_out = ((32, 64), (12, 8, 8)) if direction == "ll2hpx" else ((12, 8, 8), (32, 64))
    rng = np.random.default_rng(len(lead))
    x = rng.standard_normal(lead + shape_in).astype(np.float32)
    g = rng.standard_normal(lead + shape_out).astype(np.float32)
    xt = torch.from_numpy(x).to(cuda).requires_grad_(True)
    y = getattr(remap8, direction)(xt)
    assert tuple(y.shape) == lead + shape_out
    ref = R.apply_table(idx, w32, x.reshape(-1, n_in)).reshape(lead + shape_out)
    assert np.abs(y.detach().cpu().numpy() - ref).max() <= 1e-6 * np.abs(x).max()
    y.backward(torch.from_numpy(g).to(cuda))
    gref, bound = adjoint_ref(direction, 8, 32, 64, g.reshape(-1, n_out))
    assert (np.abs(xt.grad.cpu().numpy().reshape(-1, n_in) - gref) <= 2 * bound).all()


def test_strided_view_through_the_module(cuda, remap8):
    x = torch.randn(6, 2, 32, 64, device=cuda, generator=torch.Generator(device=cuda).manual_seed(3))
    np.testing.assert_array_equal(remap8.ll2hpx(x[:, 1]).cpu().numpy(), remap8.ll2hpx(x[:, 1].contiguous()).cpu().numpy())


def test_surface_refusals(cuda, remap8):
    from dlwp_benchmark_amd import lib as L
    from dlwp_benchmark_amd.hpx_remap import HEALPixRemap
    with pytest.raises(L.DlwpError):
        remap8.ll2hpx(torch.zeros(2, 32, 64))
    with pytest.raises(L.DlwpError):
        remap8.hpx2ll(torch.zeros(2, 12, 8, 8))
    with pytest.raises(ValueError):
        remap8.ll2hpx(torch.zeros(2, 16, 64, device=cuda))
    with pytest.raises(NotImplementedError):
        HEALPixRemap(latitudes=32, longitudes=64, nside=8, order="nearest-neighbor", device=cuda)
    with pytest.raises(ValueError):
        HEALPixRemap(latitudes=np.array([-80.0, -40.0, 10.0, 80.0]), longitudes=64, nside=2, device=cuda)
    named = HEALPixRemap(lats_deg=remap8.lats_deg, lons_deg=remap8.lons_deg, nside=8, device=cuda)
    assert torch.equal(named._hpx2ll.idx, remap8._hpx2ll.idx) and torch.equal(named._ll2hpx.w, remap8._ll2hpx.w)


# (B, T, V, n, H, W): the evaluation-like case; faces beyond LDS (two 48 KB planes: the unstaged instantiation); many groups, so that
# a workgroup runs over a batch range (2 + 1 of 3 samples) and the last 1024-point chunk is partial (8 x 16 = 128 points)
MOMENT_CASES = [(2, 3, 2, 8, 32, 64), (2, 1, 2, 32, 32, 64), (3, 20, 20, 2, 8, 16)]


@pytest.mark.parametrize("with_clim", [False, True])
@pytest.mark.parametrize("B,T,V,n,H,W", MOMENT_CASES)
def test_fused_moments(cuda, B, T, V, n, H, W, with_clim):
    from dlwp_benchmark_amd import evaluate
    from dlwp_benchmark_amd.hpx_remap import HEALPixRemap
    remap = HEALPixRemap(latitudes=H, longitudes=W, nside=n, device=cuda)
    g = torch.Generator().manual_seed(32)
    o, t = torch.randn(B, T, V, 12, n, n, generator=g), torch.randn(B, T, V, 12, n, n, generator=g)
    c = torch.randn(B, T, V, H, W, generator=g) if with_clim else None
    idx, w32, _, n_in, n_out = tables("hpx2ll", n, H, W)
    o_ll = R.apply_table(idx, w32, o.numpy().reshape(B, T, V, n_in)).reshape(B, T, V, H, W)
    t_ll = R.apply_table(idx, w32, t.numpy().reshape(B, T, V, n_in)).reshape(B, T, V, H, W)
    ref = eval_ref.dlwp_metrics(o_ll, t_ll, remap.lats_deg, None if c is None else c.numpy())
    od, td, cd = o.to(cuda), t.to(cuda), None if c is None else c.to(cuda)
    names = launched(lambda: evaluate.dlwp_metrics_hpx(od, td, remap, cd))
    assert names == ["hpx_error_moments"]
    got = evaluate.dlwp_metrics_hpx(od, td, remap, cd)
    two = evaluate.dlwp_metrics(remap.hpx2ll(od), remap.hpx2ll(td), remap.lats_deg, cd)
    assert set(got) == set(two) == ({"rmse", "acc"} if with_clim else {"rmse"})
    assert tuple(got["rmse"].shape) == (T, V)
    print(f"moments B={B} T={T} V={V} n={n}: rmse rel err {np.abs(got['rmse'].numpy() / ref['rmse'] - 1).max():.2e}")
    np.testing.assert_allclose(got["rmse"].numpy(), ref["rmse"], rtol=2e-5)
    np.testing.assert_allclose(got["rmse"].numpy(), two["rmse"].numpy(), rtol=2e-5)
    if with_clim:
        print(f"   acc abs err {np.abs(got['acc'].numpy() - ref['acc']).max():.2e}")
        np.testing.assert_allclose(got["acc"].numpy(), ref["acc"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(got["acc"].numpy(), two["acc"].numpy(), rtol=0, atol=2e-5)


def test_abi_refusals_launch_nothing(cuda):
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    d_idx, d_w, d_rowptr, d_col, d_val = dev_tables("hpx2ll", 8, 32, 64, cuda)
    src, dst, m = torch.zeros(2, 768, device=cuda), torch.zeros(2, 2048, device=cuda), torch.zeros(5, 1, device=cuda)
    big = torch.zeros(1, 49152, device=cuda)
    p = lambda t: t.data_ptr()      # noqa: E731
    rcs = []

    def calls():
        rcs.append(lib.dlwp_remap_gather4(p(src), 768, None, p(d_w), p(dst), 2, 768, 2048, L.stream()))            # NULL table
        rcs.append(lib.dlwp_remap_gather4(p(src), 768, p(d_idx), p(d_w), p(dst), 0, 768, 2048, L.stream()))        # planes = 0
        rcs.append(lib.dlwp_remap_gather4(p(src), 700, p(d_idx), p(d_w), p(dst), 2, 768, 2048, L.stream()))        # stride < n_in
        rcs.append(lib.dlwp_remap_csr(p(dst), None, p(d_col), p(d_val), p(src), 2, 2048, 768, 0, L.stream()))
        rcs.append(lib.dlwp_remap_csr(p(dst), p(d_rowptr), p(d_col), p(d_val), p(src), 0, 2048, 768, 0, L.stream()))
        rcs.append(lib.dlwp_hpx_error_moments(p(src), p(src), None, None, None, p(d_w), 1, 1, 8, 32, 64, p(m), L.stream()))
        rcs.append(lib.dlwp_hpx_error_moments(p(src), p(src), None, None, p(d_idx), p(d_w), 0, 1, 8, 32, 64, p(m), L.stream()))
        with knobs(REMAP_PATH=1):            # a forced LDS path at HPX64: 192 KB per plane
            rcs.append(lib.dlwp_remap_gather4(p(big), 49152, p(d_idx), p(d_w), p(dst), 1, 49152, 2048, L.stream()))

    assert launched(calls) == []
    assert rcs[:7] == [E_INVALID] * 7 and rcs[7] == E_UNSUPPORTED
    assert b"LDS" in lib.dlwp_last_error()


def test_lat_lon_record_to_hpx_model_to_score(cuda, remap8):
    from dlwp_benchmark_amd import dlwpbench, evaluate, wbdata
    fields, prognostic, prescribed, constants = wbdata.synthetic_fields(40, 32, 64)
    hpx = remap8.remap_fields(fields)
    assert hpx["t2m"].shape == (40, 12, 8, 8) and hpx["z"][500].shape == (40, 12, 8, 8) and hpx["lsm"].shape == (12, 8, 8)
    idx, w32, _, n_in, _ = tables("ll2hpx", 8, 32, 64)
    ref = R.apply_table(idx, w32, fields["t2m"].reshape(40, n_in)).reshape(40, 12, 8, 8)
    assert np.abs(hpx["t2m"] - ref).max() <= 1e-6 * np.abs(fields["t2m"]).max()
    L_, ctx = 5, 1
    ds = wbdata.WeatherBenchArrays(hpx, prognostic, prescribed, constants, sequence_length=L_, normalize=True, context_size=ctx, seed=0)
    const, presc, prog, target = wbdata.to_device_batch([ds[0], ds[1]], cuda)
    assert tuple(const.shape) == (2, 1, 4, 12, 8, 8) and tuple(presc.shape) == (2, L_, 1, 12, 8, 8)
    assert tuple(prog.shape) == (2, L_, 8, 12, 8, 8) and tuple(target.shape) == (2, L_ - ctx, 8, 12, 8, 8)
    torch.manual_seed(5)
    model = dlwpbench.ConvLSTMHPX(constant_channels=4, prescribed_channels=1, prognostic_channels=8, hidden_sizes=[8, 8],
                                  context_size=ctx).to(cuda)
    with torch.no_grad():
        out = model(const, presc, prog)
    assert out.shape == target.shape
    clim = torch.zeros(2, L_ - ctx, 8, 32, 64, device=cuda)
    res = evaluate.dlwp_metrics_hpx(out, target, remap8, clim)
    assert tuple(res["rmse"].shape) == tuple(res["acc"].shape) == (L_ - ctx, 8)
    assert torch.isfinite(res["rmse"]).all() and torch.isfinite(res["acc"]).all() and (res["rmse"] > 0).all()
