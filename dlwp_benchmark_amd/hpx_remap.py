"""Lat-lon <-> HEALPix remap on libdlwpmi (csrc/hpx_remap.hip): the reference's offline `HEALPixRemap`
(src/dlwpbench/data/processing/healpix_mapping.py:328-399) as two table gathers on the GPU.

The tables come from `hpx_geometry` (float64 on the host, uploaded once as int32 / float32); `ll2hpx` and `hpx2ll` apply them to any
number of leading axes in one launch and are differentiable (the backward is the transposed table as a CSR gather, summed in a fixed
order).  Parity with the reference's remap is unpinned (environment): reproject / astropy / healpy are not available, see
hpx_geometry's docstring and docs/kernels/remap.md for the anchoring and for the two deliberate deviations.
"""
import numpy as np
import torch

from . import hpx_geometry as G
from . import lib as L


def _check_table(idx, w, n_in, what):
    if idx.ndim != 2 or idx.shape[1] != 4 or w.shape != idx.shape:
        raise ValueError(f"{what}: tables must be [n_out, 4]")
    if idx.min() < 0 or idx.max() >= n_in:
        raise ValueError(f"{what}: index outside [0, {n_in})")
    if not np.isfinite(w).all():
        raise ValueError(f"{what}: non-finite weight")


def _check_csr(rowptr, col, val, n_rows, n_cols, what):
    if len(rowptr) != n_rows + 1 or rowptr[0] != 0 or (np.diff(rowptr) < 0).any() or rowptr[-1] != len(col) or len(col) != len(val):
        raise ValueError(f"{what}: rowptr is not a monotone offset table of its entries")
    if len(col) and (col.min() < 0 or col.max() >= n_cols):
        raise ValueError(f"{what}: column outside [0, {n_cols})")


class _Table:
    """one direction: the gather table and its transpose on the device"""

    def __init__(self, idx, w, n_in, device, what):
        _check_table(idx, w, n_in, what)
        rowptr, col, val = G.transpose_csr(idx, w, n_in)
        _check_csr(rowptr, col, val, n_in, idx.shape[0], what + " (transpose)")
        self.n_in, self.n_out = int(n_in), int(idx.shape[0])
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device)      # noqa: E731
        self.idx, self.w = up(idx, torch.int32), up(w, torch.float32)
        self.rowptr, self.col, self.val = up(rowptr, torch.int32), up(col, torch.int32), up(val, torch.float32)
        if len(col) == 0:                                     # (cannot happen for an interpolation table: keeps the pointers non-NULL)
            self.col, self.val = torch.zeros(1, dtype=torch.int32, device=device), torch.zeros(1, device=device)


def _planes(x, n_in):
    """(tensor to keep alive, planes, plane stride in floats): x [..., n_in-element dense planes] read in place where the leading axes
    collapse to one stride, through a contiguous copy otherwise"""
    planes = x.numel() // n_in
    if x.is_contiguous():
        return x, planes, n_in
    sizes, strides = list(x.shape), list(x.stride())
    # trailing axes that make up a plane
    k, run = len(sizes), 1
    while k > 0 and run < n_in:
        k -= 1
        if sizes[k] != 1 and strides[k] != run:
            return x.contiguous(), planes, n_in
        run *= sizes[k]
    lead = [(s, st) for s, st in zip(sizes[:k], strides[:k]) if s != 1]
    if run != n_in or not lead:
        return x.contiguous(), planes, n_in
    for (s0, st0), (s1, st1) in zip(lead, lead[1:]):
        if st0 != st1 * s1:
            return x.contiguous(), planes, n_in
    stride = lead[-1][1]
    if stride < n_in:
        return x.contiguous(), planes, n_in
    return x, planes, stride


def _gather(x, tab, out_shape):
    if not x.is_cuda:
        raise L.DlwpError("libdlwpmi needs CUDA/HIP tensors (no CPU fallback)")
    if x.dtype != torch.float32:
        raise L.DlwpError(f"the remap kernels take float32 tensors, not {x.dtype}")
    y = torch.empty(out_shape, device=x.device, dtype=torch.float32)
    if y.numel() == 0:
        return y
    src, planes, stride = _planes(x, tab.n_in)
    L.check(L.load().dlwp_remap_gather4(src.data_ptr(), stride, L.ptr(tab.idx), L.ptr(tab.w), L.ptr(y), planes, tab.n_in, tab.n_out,
                                        L.stream()))
    return y


def _adjoint(g, tab, in_shape):
    """R^T g: g [..., n_out planes] -> in_shape"""
    gx = torch.empty(in_shape, device=g.device, dtype=torch.float32)
    if gx.numel() == 0:
        return gx
    gc = g.contiguous()
    L.check(L.load().dlwp_remap_csr(L.ptr(gc), L.ptr(tab.rowptr), L.ptr(tab.col), L.ptr(tab.val), L.ptr(gx), gc.numel() // tab.n_out,
                                    tab.n_out, tab.n_in, 0, L.stream()))
    return gx


class _Remap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, tab, k_in, tail_out):
        ctx.tab, ctx.in_shape = tab, x.shape
        return _gather(x, tab, x.shape[:x.dim() - k_in] + tuple(tail_out))

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        return _adjoint(g, ctx.tab, ctx.in_shape), None, None, None


class HEALPixRemap:
    """`HEALPixRemap(latitudes, longitudes, nside, order="bilinear")` of the reference, on the GPU.

    latitudes / longitudes (or lats_deg / lons_deg): the grid's coordinates in degrees, or integers H / W for the grid
    lat = -90 + 90/H + i 180/H, lon = j 360/W (`wbdata.synthetic_fields`, WeatherBench 5.625 degrees).  Only `order="bilinear"`
    exists (NotImplementedError otherwise).  The constructor builds and validates both tables and both transposes and uploads them.

    ll2hpx(x): [..., H, W] -> [..., 12, n, n];  hpx2ll(x): [..., 12, n, n] -> [..., H, W].  fp32 CUDA tensors with any number of
    leading axes; views whose planes are dense are read in place; differentiable; CPU tensors raise DlwpError.
    remap_fields(fields): a `wbdata` fields mapping with every trailing [lat, lon] replaced by [12, n, n]."""

    def __init__(self, latitudes=None, longitudes=None, nside=None, order="bilinear", device=None, lats_deg=None, lons_deg=None,
                 **kwargs):
        if order != "bilinear":
            raise NotImplementedError(f"HEALPixRemap: only order='bilinear' is built, not {order!r}")
        lats = latitudes if latitudes is not None else lats_deg
        lons = longitudes if longitudes is not None else lons_deg
        if lats is None or lons is None or nside is None:
            raise ValueError("HEALPixRemap needs latitudes, longitudes and nside")
        if np.ndim(lats) == 0:
            H = int(lats)
            lats = -90.0 + 90.0 / H + np.arange(H) * (180.0 / H)
        if np.ndim(lons) == 0:
            W = int(lons)
            lons = np.arange(W) * (360.0 / W)
        self.lats_deg, self.lons_deg = np.asarray(lats, dtype=np.float64), np.asarray(lons, dtype=np.float64)
        self.nside = int(nside)
        self.H, self.W, self.npix = self.lats_deg.size, self.lons_deg.size, 12 * self.nside * self.nside
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise L.DlwpError("libdlwpmi needs CUDA/HIP tensors (no CPU fallback)")
        self._ll2hpx = _Table(*G.ll2hpx_table(self.lats_deg, self.lons_deg, self.nside), self.H * self.W, self.device, "ll2hpx")
        self._hpx2ll = _Table(*G.hpx2ll_table(self.lats_deg, self.lons_deg, self.nside), self.npix, self.device, "hpx2ll")

    def ll2hpx(self, x):
        if x.dim() < 2 or tuple(x.shape[-2:]) != (self.H, self.W):
            raise ValueError(f"ll2hpx takes [..., {self.H}, {self.W}], not {tuple(x.shape)}")
        return _Remap.apply(x, self._ll2hpx, 2, (12, self.nside, self.nside))

    def hpx2ll(self, x):
        if x.dim() < 3 or tuple(x.shape[-3:]) != (12, self.nside, self.nside):
            raise ValueError(f"hpx2ll takes [..., 12, {self.nside}, {self.nside}], not {tuple(x.shape)}")
        return _Remap.apply(x, self._hpx2ll, 3, (self.H, self.W))

    def remap_fields(self, fields, max_planes=4096):
        """{name: array [..., lat, lon]} / {name: {level: array}} -> the same mapping on the HEALPix mesh (numpy float32), through
        the GPU in batches of at most `max_planes` maps"""
        def one(a):
            a = np.asarray(a, dtype=np.float32)
            if a.ndim < 2 or a.shape[-2:] != (self.H, self.W):
                raise ValueError(f"remap_fields: array of shape {a.shape} does not end in [{self.H}, {self.W}]")
            flat = np.ascontiguousarray(a).reshape(-1, self.H, self.W)
            out = np.empty((flat.shape[0], 12, self.nside, self.nside), dtype=np.float32)
            for s in range(0, flat.shape[0], max_planes):
                out[s:s + max_planes] = self.ll2hpx(torch.from_numpy(flat[s:s + max_planes]).to(self.device)).cpu().numpy()
            return out.reshape(a.shape[:-2] + (12, self.nside, self.nside))
        return {k: ({l: one(a) for l, a in v.items()} if isinstance(v, dict) else one(v)) for k, v in fields.items()}
