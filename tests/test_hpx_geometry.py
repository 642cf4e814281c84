"""dlwp_benchmark_amd/hpx_geometry.py on the CPU: the face layout against the project's HEALPix padding (tests/hpx_ref.py, pinned against
the reference), the pixel centres against the analytic ring structure, both remap tables against their defining properties and against
the smooth fields S of tests/hpx_remap_ref.py.  The reference's remap (reproject / astropy / healpy) cannot run here: parity unpinned
(environment).

Accuracy bounds: a float64 prototype of exactly these algorithms measured the largest absolute error over the nine fields of S as
hpx2ll 0.0240 (n = 8, 32 x 64) / 0.0118 (n = 16, 64 x 128) and ll2hpx 0.0069 / 0.0018; the tests allow 1.25 times that (floor and tie
choices that are equally valid), and 1e-12 on the constant field."""
import numpy as np
import pytest
import torch

import hpx_ref
import hpx_remap_ref as R
from dlwp_benchmark_amd import hpx_geometry as G

SHAPES = [(1, 4, 8), (2, 8, 16), (8, 32, 64)]


@pytest.mark.parametrize("n", [2, 4, 8])
def test_layout_is_consistent_with_the_healpix_padding(n):
    lat, lon = G.face_centres(n)
    v = torch.from_numpy(np.stack(R.unit_vectors(lat, lon), axis=1))          # [12, 3, n, n]
    p = hpx_ref.hpx_pad1(v).numpy()                                            # [12, 3, n + 2, n + 2]
    pix = np.sqrt(4 * np.pi / (12 * n * n))

    def angle(a, b):                                                           # [12, 3, k] each
        return np.arccos(np.clip((a * b).sum(1), -1.0, 1.0))

    worst = 0.0
    for edge, inner in ((p[:, :, 0, 1:-1], p[:, :, 1, 1:-1]), (p[:, :, -1, 1:-1], p[:, :, -2, 1:-1]),
                        (p[:, :, 1:-1, 0], p[:, :, 1:-1, 1]), (p[:, :, 1:-1, -1], p[:, :, 1:-1, -2])):
        worst = max(worst, float(angle(edge, inner).max()) / pix)
    print(f"n={n}: worst edge-to-interior angle {worst:.3f} pixel sizes")
    assert worst <= 1.5


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_centres(n):
    lat, lon = G.face_centres(n)
    assert lat.shape == lon.shape == (12, n, n)
    z = np.sin(np.deg2rad(lat))
    assert abs(z.sum()) < 1e-10
    jr, jp0, _, _ = G._face_rings(n)
    counts = np.bincount(jr.ravel(), minlength=4 * n)
    assert counts[0] == 0
    for i in range(1, 4 * n):
        assert counts[i] == 4 * min(i, n, 4 * n - i), i
    # every (ring, position) occurs once
    lut = G.ring_lookup(n)
    assert sorted(lut.tolist()) == list(range(12 * n * n))
    assert ((lon >= 0) & (lon < 360)).all()
    # the centre of mass of a face sits on its axis: lon 45 + 90 k for the polar faces, 90 k for the equatorial ones
    x, y, zz = R.unit_vectors(lat, lon)
    for f in range(12):
        k = f % 4
        want = 90.0 * k if 4 <= f < 8 else 45.0 + 90.0 * k
        got = np.rad2deg(np.arctan2(y[f].sum(), x[f].sum())) % 360.0
        assert abs((got - want + 180.0) % 360.0 - 180.0) < 1e-9, (f, got, want)


def test_centres_n1():
    lat, lon = G.face_centres(1)
    z = np.sin(np.deg2rad(lat)).ravel()
    np.testing.assert_allclose(z, [2 / 3] * 4 + [0.0] * 4 + [-2 / 3] * 4, atol=1e-15)
    np.testing.assert_allclose(lon.ravel(), [45, 135, 225, 315, 0, 90, 180, 270, 45, 135, 225, 315], atol=1e-12)


@pytest.mark.parametrize("n,H,W", SHAPES)
def test_table_properties(n, H, W):
    lats, lons = R.regular_grid(H, W)
    for name, (idx, w), n_in, n_out in (("ll2hpx", G.ll2hpx_table(lats, lons, n), H * W, 12 * n * n),
                                        ("hpx2ll", G.hpx2ll_table(lats, lons, n), 12 * n * n, H * W)):
        assert idx.dtype == np.int32 and w.dtype == np.float64 and idx.shape == w.shape == (n_out, 4), name
        assert (w >= 0).all(), name
        assert np.abs(w.sum(1) - 1).max() <= 1e-12, name
        assert idx.min() >= 0 and idx.max() < n_in, name
        if name == "hpx2ll":
            s = np.sort(idx, axis=1)
            assert (np.diff(s, axis=1) > 0).all(), "the four pixels of an hpx2ll row are distinct"


@pytest.mark.parametrize("n", [1, 2, 8])
def test_hpx2ll_at_the_pixel_centres_is_the_identity(n):
    lat, lon = G.face_centres(n)
    idx, w = G.hpx2ll_points(lat.ravel(), lon.ravel(), n)
    M = R.dense_table(idx, w, 12 * n * n)
    err = np.abs(M - np.eye(12 * n * n)).max()
    print(f"n={n}: |hpx2ll(centres) - I| = {err:.2e}")
    assert err <= 1e-9


@pytest.mark.parametrize("n,H,W", [(2, 8, 16), (8, 32, 64)])
def test_ll2hpx_reproduces_latitude(n, H, W):
    lats, lons = R.regular_grid(H, W)
    lat_c, _ = G.face_centres(n)
    assert np.abs(lat_c).max() <= abs(lats[-1])                               # no pixel is clamped at these shapes
    field = np.repeat(lats[:, None], W, axis=1).ravel()
    idx, w = G.ll2hpx_table(lats, lons, n)
    np.testing.assert_allclose(R.apply_table(idx, w, field), lat_c.ravel(), rtol=0, atol=1e-9)
    # descending latitudes: the same map applied to the row-flipped field
    rng = np.random.default_rng(5)
    x = rng.standard_normal((H, W))
    idx_d, w_d = G.ll2hpx_table(lats[::-1], lons, n)
    np.testing.assert_allclose(R.apply_table(idx_d, w_d, x[::-1].ravel()), R.apply_table(idx, w, x.ravel()), rtol=0, atol=1e-12)


def test_ll2hpx_clamps_poleward_pixels():
    lats, lons = R.regular_grid(4, 8)                                         # rows at +-22.5, +-67.5; HPX8 reaches 84.1
    idx, w = G.ll2hpx_table(lats, lons, 8)
    field = np.repeat(lats[:, None], 8, axis=1).ravel()
    lat_c = G.face_centres(8)[0].ravel()
    np.testing.assert_allclose(R.apply_table(idx, w, field), np.clip(lat_c, lats[0], lats[-1]), rtol=0, atol=1e-9)


@pytest.mark.parametrize("n,H,W,e_h2l,e_l2h", [(8, 32, 64, 0.0240, 0.0069), (16, 64, 128, 0.0118, 0.0018)])
def test_accuracy_on_smooth_fields(n, H, W, e_h2l, e_l2h):
    lats, lons = R.regular_grid(H, W)
    lat_c, lon_c = (a.ravel() for a in G.face_centres(n))
    s_hpx = R.S(lat_c, lon_c)                                                  # [9, 12 n^2]
    s_ll = R.S(np.repeat(lats, W), np.tile(lons, H))                           # [9, H W]
    idx, w = G.hpx2ll_table(lats, lons, n)
    err = np.abs(R.apply_table(idx, w, s_hpx) - s_ll)
    print(f"hpx2ll n={n} {H}x{W}: max |err| {err.max():.4f} (constant {err[0].max():.1e})")
    assert err[0].max() <= 1e-12 and err.max() <= 1.25 * e_h2l
    idx, w = G.ll2hpx_table(lats, lons, n)
    err = np.abs(R.apply_table(idx, w, s_ll) - s_hpx)
    print(f"ll2hpx n={n} {H}x{W}: max |err| {err.max():.4f} (constant {err[0].max():.1e})")
    assert err[0].max() <= 1e-12 and err.max() <= 1.25 * e_l2h


def test_transpose_csr():
    n, H, W = 2, 8, 16
    lats, lons = R.regular_grid(H, W)
    for (idx, w), n_in in ((G.hpx2ll_table(lats, lons, n), 12 * n * n), (G.ll2hpx_table(lats, lons, n), H * W)):
        w = w.copy()
        w[3, 1] = 0.0                                                          # a zero weight is dropped
        rowptr, col, val = G.transpose_csr(idx, w, n_in)
        assert rowptr.dtype == col.dtype == np.int32 and val.dtype == np.float64
        assert rowptr[0] == 0 and rowptr[-1] == len(col) == len(val) and (np.diff(rowptr) >= 0).all()
        assert (val != 0).all() and len(val) == np.count_nonzero(w)
        for r in range(n_in):
            assert (np.diff(col[rowptr[r]:rowptr[r + 1]]) >= 0).all()
        np.testing.assert_array_equal(R.dense_csr(rowptr, col, val, idx.shape[0]), R.dense_table(idx, w, n_in).T)


def test_polar_rows_are_long():
    lats, lons = R.regular_grid(32, 64)
    rowptr, _, _ = G.transpose_csr(*G.hpx2ll_table(lats, lons, 8), 768)
    lens = np.diff(rowptr)
    assert lens.max() >= 64 and lens.min() <= 8


def test_validation():
    lats, lons = R.regular_grid(8, 16)
    for fn in (G.ll2hpx_table,):
        with pytest.raises(ValueError, match="equally spaced"):
            fn(np.array([-80.0, -40.0, 10.0, 80.0]), lons, 2)
        with pytest.raises(ValueError, match="equally spaced"):
            fn(lats, np.concatenate((lons[:-1], [lons[-1] + 3.0])), 2)
        with pytest.raises(ValueError, match="360"):
            fn(lats, lons[:8], 2)
        with pytest.raises(ValueError, match="two"):
            fn(lats[:1], lons, 2)
    with pytest.raises(ValueError):
        G.face_centres(0)
    with pytest.raises(ValueError):
        G.transpose_csr(np.array([[0, 1, 2, 9]]), np.ones((1, 4)), 4)


def test_tables_at_nside_64_build_quickly():
    lats, lons = R.regular_grid(32, 64)
    idx, w = G.ll2hpx_table(lats, lons, 64)
    assert idx.shape == (12 * 64 * 64, 4)
    idx2, w2 = G.hpx2ll_table(lats, lons, 64)
    assert idx2.shape == (32 * 64, 4) and idx2.max() < 12 * 64 * 64
    rowptr, col, val = G.transpose_csr(idx, w, 32 * 64)
    assert rowptr[-1] == np.count_nonzero(w)
