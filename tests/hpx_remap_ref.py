"""Float64 numpy restatement of applying a 4-tap remap table, and the smooth test fields on the unit sphere (helper module for
tests/test_hpx_geometry.py and tests/test_gpu_hpx_remap.py, not a conftest)."""
import numpy as np


def apply_table(idx, w, x):
    """idx [n_out, 4] into the flattened trailing axis of x [..., n_in], w [n_out, 4] -> [..., n_out] float64"""
    x = np.asarray(x, dtype=np.float64)
    return (x[..., np.asarray(idx, dtype=np.int64)] * np.asarray(w, dtype=np.float64)).sum(-1)


def dense_table(idx, w, n_in):
    """the [n_out, n_in] float64 matrix of a table"""
    R = np.zeros((idx.shape[0], n_in))
    np.add.at(R, (np.repeat(np.arange(idx.shape[0]), idx.shape[1]), np.asarray(idx, dtype=np.int64).ravel()),
              np.asarray(w, dtype=np.float64).ravel())
    return R


def dense_csr(rowptr, col, val, n_cols):
    """the [rows, n_cols] float64 matrix of a CSR triple"""
    rows = len(rowptr) - 1
    M = np.zeros((rows, n_cols))
    np.add.at(M, (np.repeat(np.arange(rows), np.diff(rowptr)), np.asarray(col, dtype=np.int64)), np.asarray(val, dtype=np.float64))
    return M


def unit_vectors(lat_deg, lon_deg):
    lat, lon = np.deg2rad(np.asarray(lat_deg, dtype=np.float64)), np.deg2rad(np.asarray(lon_deg, dtype=np.float64))
    return np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)


def S(lat_deg, lon_deg):
    """[9, ...]: 1, x, y, z, xy, z^2 - 1/3, xz, (5 z^3 - 3 z) / 2, x^2 - y^2 at the given points of the unit sphere"""
    x, y, z = unit_vectors(lat_deg, lon_deg)
    return np.stack([np.ones_like(x), x, y, z, x * y, z * z - 1.0 / 3.0, x * z, (5 * z ** 3 - 3 * z) / 2, x * x - y * y])


def regular_grid(H, W):
    """the grid integer H / W stand for: lat = -90 + 90/H + i 180/H, lon = j 360/W"""
    return -90.0 + 90.0 / H + np.arange(H) * (180.0 / H), np.arange(W) * (360.0 / W)
