"""HEALPix geometry for the lat-lon <-> HEALPix remap tables (host, numpy, float64, vectorised: no loop over pixels or grid points).

Written from the HEALPix definitions (Gorski et al. 2005: 12 base faces, nested face coordinates, rings of constant latitude); the
reference builds the same maps offline through reproject / astropy / healpy (data/processing/healpix_mapping.py), none of which is
available here, so PARITY WITH THE REFERENCE'S REMAP IS UNPINNED (environment).  The geometry is anchored analytically and against the
project's own `padding="healpix"` neighbour table (tests/test_hpx_geometry.py), which is pinned against the reference.

Face layout.  Element [f, h, w] of a [12, n, n] tensor is the pixel of base face f with nested coordinates ix = n-1-h, iy = n-1-w: the
north corner of a face is its top-left element (what the reference's hpx1d2hpx3d -- hpx3d[f, x, y], then a flip of both axes -- produces,
and the only one of the four candidate layouts under which every padded edge cell of the HEALPix padding lies next to its interior
neighbour on the sphere).

Rings.  Ring jr = 1 .. 4n-1 (north to south) has 4 nr pixels, nr = min(jr, n, 4n - jr), at height z(jr) and azimuths
phi_j = (j + shift/2) 2 pi / (4 nr), j = 0 .. 4nr-1, shift = 1 in the caps and 1 - ((jr - n) & 1) in the equatorial belt.
"""
import numpy as np

JRLL = np.array([2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4], dtype=np.int64)
JPLL = np.array([1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7], dtype=np.int64)


def _ring_tables(n):
    """per ring jr = 1 .. 4n-1 (array index jr - 1): nr, z, shift, and the offset of the ring's first pixel in ring order"""
    jr = np.arange(1, 4 * n, dtype=np.int64)
    north, south = jr < n, jr > 3 * n
    nr = np.where(north, jr, np.where(south, 4 * n - jr, n))
    cap = nr.astype(np.float64) ** 2 / (3.0 * n * n)
    z = np.where(north, 1.0 - cap, np.where(south, cap - 1.0, (2 * n - jr) * 2.0 / (3.0 * n)))
    ks = np.where(north | south, 0, (jr - n) & 1)
    start = np.concatenate(([0], np.cumsum(4 * nr)[:-1]))
    return nr, z, 1 - ks, start


def _face_rings(n):
    """ring number jr (1-based) and position in the ring jp - 1 (0-based) of every array element [12, n, n]"""
    f, h, w = np.meshgrid(np.arange(12), np.arange(n), np.arange(n), indexing="ij")
    ix, iy = n - 1 - h, n - 1 - w
    jr = JRLL[f] * n - ix - iy - 1
    north, south = jr < n, jr > 3 * n
    nr = np.where(north, jr, np.where(south, 4 * n - jr, n))
    ks = np.where(north | south, 0, (jr - n) & 1)
    jp = (JPLL[f] * nr + ix - iy + 1 + ks) // 2
    jp = np.where(jp > 4 * nr, jp - 4 * nr, jp)
    jp = np.where(jp < 1, jp + 4 * nr, jp)
    return jr, jp - 1, nr, ks


def face_centres(n):
    """-> (lat_deg, lon_deg), each [12, n, n] float64: the centre of every pixel in the face layout; lon east positive in [0, 360)"""
    n = int(n)
    if n < 1:
        raise ValueError("nside must be at least 1")
    jr, jp0, nr, ks = _face_rings(n)
    _, zr, _, _ = _ring_tables(n)
    z = zr[jr - 1]
    phi = (jp0 + 1 - (ks + 1) / 2.0) * (np.pi / (2.0 * nr))
    return np.rad2deg(np.arcsin(z)), np.rad2deg(phi) % 360.0


def ring_lookup(n):
    """int64 [12 n^2]: flat face-layout index f n^2 + h n + w of the pixel at (ring, position), rings concatenated north to south"""
    jr, jp0, _, _ = _face_rings(n)
    _, _, _, start = _ring_tables(n)
    lut = np.full(12 * n * n, -1, dtype=np.int64)
    lut[(start[jr - 1] + jp0).ravel()] = np.arange(12 * n * n)
    assert (lut >= 0).all()
    return lut


def _regular_axis(v, what):
    v = np.asarray(v, dtype=np.float64).ravel()
    if v.size < 2:
        raise ValueError(f"{what}: at least two grid values are needed")
    d = np.diff(v)
    if d[0] == 0 or not np.allclose(d, d[0], rtol=0, atol=1e-9 * max(1.0, abs(d[0]))):
        raise ValueError(f"{what} are not equally spaced")
    return v, float((v[-1] - v[0]) / (v.size - 1))


def _check_grid(lats_deg, lons_deg):
    lats, dlat = _regular_axis(lats_deg, "latitudes")
    lons, dlon = _regular_axis(lons_deg, "longitudes")
    if abs(abs(dlon) * lons.size - 360.0) > 1e-6:
        raise ValueError(f"longitudes do not cover 360 degrees ({lons.size} columns of {abs(dlon)} degrees)")
    return lats, dlat, lons, dlon


def ll2hpx_table(lats_deg, lons_deg, n):
    """Bilinear interpolation of a regular lat-lon grid at every HEALPix pixel centre.

    lats_deg [H] (ascending or descending, equally spaced, H >= 2), lons_deg [W] (equally spaced, W columns covering 360 degrees)
    -> idx int32 [12 n^2, 4] (flat h W + w indices), w float64 [12 n^2, 4]; rows in the face layout order f n^2 + h n + w.
    Longitude wraps periodically; the latitude coordinate is clamped to the first and last row (pixels poleward of the outermost
    row take that row's longitude-interpolated value).  ValueError for unequal spacing, partial longitude coverage, H < 2.

    Deviations from the reference (HEALPixRemap.ll2hpx through reproject): (1) reproject does not wrap longitude and leaves NaN
    where a tap falls outside the image -- this table defines every pixel; (2) the reference's WCS carries a one-degree longitude
    offset (CRVAL1 180 against 179) which is not reproduced."""
    lats, dlat, lons, dlon = _check_grid(lats_deg, lons_deg)
    H, W = lats.size, lons.size
    lat_c, lon_c = (a.ravel() for a in face_centres(n))
    fi = np.clip((lat_c - lats[0]) / dlat, 0.0, H - 1.0)
    i0 = np.minimum(np.floor(fi).astype(np.int64), H - 2)
    wy = fi - i0
    fj = ((lon_c - lons[0]) / dlon) % W
    j0 = np.floor(fj).astype(np.int64)
    wx = fj - j0
    j0 %= W
    j1 = (j0 + 1) % W
    idx = np.stack([i0 * W + j0, i0 * W + j1, (i0 + 1) * W + j0, (i0 + 1) * W + j1], axis=1).astype(np.int32)
    w = np.stack([(1 - wy) * (1 - wx), (1 - wy) * wx, wy * (1 - wx), wy * wx], axis=1)
    return idx, w


def _in_ring(phi, nr4, shift):
    """the two pixels of a ring of nr4 pixels around azimuth phi and the weight of the second"""
    t = phi / (2.0 * np.pi / nr4) - shift / 2.0
    i1 = np.floor(t)
    w1 = t - i1
    i1 = i1.astype(np.int64)
    return i1 % nr4, (i1 + 1) % nr4, w1


def hpx2ll_points(lat_deg, lon_deg, n):
    """The standard HEALPix bilinear interpolation (get_interp_weights) at arbitrary points: lat_deg, lon_deg [P]
    -> idx int64 [P, 4] (face-layout indices), w float64 [P, 4].

    Between two rings the two nearest pixels of each are weighted linearly in azimuth and the rings linearly in colatitude; above
    the first (below the last) ring the four pixels of that ring share (1 - wt) / 4 each on top of wt times the in-ring weights,
    wt = theta / theta_1 (mirrored in the south)."""
    n = int(n)
    lat = np.asarray(lat_deg, dtype=np.float64).ravel()
    phi = np.deg2rad(np.asarray(lon_deg, dtype=np.float64).ravel()) % (2.0 * np.pi)
    theta = np.pi / 2.0 - np.deg2rad(lat)
    nr, zr, shift, start = _ring_tables(n)
    lut = ring_lookup(n)
    theta_r = np.arccos(zr)
    nrings = 4 * n - 1
    ir1 = np.searchsorted(theta_r, theta, side="right")    # number of rings with z_ring >= z = the last such ring (1-based), 0: none
    north, south = ir1 == 0, ir1 == nrings
    ra = np.clip(ir1, 1, nrings) - 1                       # array index of the upper ring (of ring 1 above the first ring)
    rb = np.clip(ir1 + 1, 1, nrings) - 1                   # ... of the lower ring (of the last ring below it)
    a1, a2, wa = _in_ring(phi, 4 * nr[ra], shift[ra])
    b1, b2, wb = _in_ring(phi, 4 * nr[rb], shift[rb])
    th1, th2 = theta_r[ra], theta_r[rb]
    with np.errstate(invalid="ignore", divide="ignore"):
        wt = np.where(north, theta / th2, np.where(south, (theta - th1) / (np.pi - th1), (theta - th1) / (th2 - th1)))
    wt = np.clip(wt, 0.0, 1.0)
    pa1, pa2 = lut[start[ra] + a1], lut[start[ra] + a2]
    pb1, pb2 = lut[start[rb] + b1], lut[start[rb] + b2]
    idx = np.stack([pa1, pa2, pb1, pb2], axis=1)
    w = np.stack([(1 - wt) * (1 - wa), (1 - wt) * wa, wt * (1 - wb), wt * wb], axis=1)
    if north.any():        # ring 1 (= rb there): its pair, and the two pixels opposite
        m = north
        q = (1 - wt[m]) / 4
        idx[m] = np.stack([pb1[m], pb2[m], lut[start[rb[m]] + (b1[m] + 2) % 4], lut[start[rb[m]] + (b2[m] + 2) % 4]], axis=1)
        w[m] = np.stack([wt[m] * (1 - wb[m]) + q, wt[m] * wb[m] + q, q, q], axis=1)
    if south.any():        # the last ring (= ra there), mirrored
        m = south
        q = wt[m] / 4
        idx[m] = np.stack([pa1[m], pa2[m], lut[start[ra[m]] + (a1[m] + 2) % 4], lut[start[ra[m]] + (a2[m] + 2) % 4]], axis=1)
        w[m] = np.stack([(1 - wt[m]) * (1 - wa[m]) + q, (1 - wt[m]) * wa[m] + q, q, q], axis=1)
    return idx, w


def hpx2ll_table(lats_deg, lons_deg, n):
    """HEALPix bilinear interpolation at every point of a lat-lon grid: lats_deg [H], lons_deg [W]
    -> idx int32 [H W, 4] (face-layout indices f n^2 + h n + w), w float64 [H W, 4]; rows in the order h W + w."""
    lats = np.asarray(lats_deg, dtype=np.float64).ravel()
    lons = np.asarray(lons_deg, dtype=np.float64).ravel()
    if lats.size < 1 or lons.size < 1:
        raise ValueError("hpx2ll_table: empty grid")
    idx, w = hpx2ll_points(np.repeat(lats, lons.size), np.tile(lons, lats.size), n)
    return idx.astype(np.int32), w


def transpose_csr(idx, w, n_in):
    """The transpose of a 4-tap table as CSR over its n_in inputs: rowptr int32 [n_in + 1], col int32 [nnz] (ascending within a row),
    val float64 [nnz]; zero weights are dropped.  Row lengths are very uneven (HPX8 on 32 x 64: 96 readers of a polar pixel, 4 of an
    equatorial one)."""
    idx, w = np.asarray(idx), np.asarray(w, dtype=np.float64)
    rows = idx.ravel().astype(np.int64)
    cols = np.repeat(np.arange(idx.shape[0], dtype=np.int64), idx.shape[1])
    vals = w.ravel()
    keep = vals != 0
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    if rows.size and (rows.min() < 0 or rows.max() >= n_in):
        raise ValueError("transpose_csr: table index outside [0, n_in)")
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    rowptr = np.zeros(n_in + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_in), out=rowptr[1:])
    return rowptr.astype(np.int32), cols.astype(np.int32), vals
