"""Power spectra of forecasts and targets per lead time (csrc/spectra.hip): at which scales is a forecast still right, and how
quickly does it blur?  The complement of the grid-point scores of evaluate.py; the reference has no spectra, so the definitions
below are the contract (restated in float64 in tests/spectra_ref.py).

Sphere (`sphere_spectra`).  With colatitude nodes theta_k, quadrature weights w_k and the orthonormal associated Legendre functions
P~_l^m of sht.legpoly, the analysis is that of sht.RealSHT,
    a_lm = sum_k w_k P~_l^m(cos theta_k) (2 pi / W) sum_n x[k, n] exp(-2 pi i m n / W),        0 <= m < M = min(L, W // 2)
(the Nyquist order is left out), and per (sample, lead time, variable, degree l), c_0 = 1 and c_m = 2 otherwise:
    power  P_l = (1 / 4 pi) sum_m c_m |a_lm|^2        of output and target: sum_l P_l is the mean of f^2 over the sphere
    cross  C_l = (1 / 4 pi) sum_m c_m Re(a_lm^out conj a_lm^tgt)
    a00    Re a_00 = sqrt(4 pi) mean(f): a per-variable shift moves degree 0 only, so the host applies it here.
Everything on the device is in NORMALISED units (no z500 offset inside an fp32 sum, csrc/rollout_diag.hip's rule);
`spectral_metrics` brings the tables to physical units in float64.

Grids.  "midpoint" is the benchmark's latitude axis (evaluate.regular_latitudes: lat_k = -90 + d / 2 + d k, south first) with Fejer's
first-rule weights (`fejer1_weights`).  That rule integrates polynomials in cos(theta) up to degree H - 1 only: the analysis recovers
a field band-limited to degrees < H / 2 to rounding (5e-15 in float64 at 8 x 16 and 32 x 64), and degrees >= H / 2 are
QUADRATURE-APPROXIMATE -- a field with power up to degree H - 1 aliases (coefficient error 0.9 at H = 8, 0.5 to 1.4 at H = 32).  On
"legendre-gauss" nodes all H degrees are exact (2e-14); "equiangular" is sht's Clenshaw-Curtis grid.  Both are north first, as
sht.sht_tables builds them.  The tables are operands of the kernel, which never evaluates a sine or a recurrence.

Plane (`plane_spectra`).  For doubly periodic fields [.., H, W] with u = rfft2(f) (norm "backward"):
    E(k) = sum c |u|^2 / (H W)^2 over the half-spectrum entries with rint(sqrt(kx^2 + ky^2)) = k,       K = max k + 1 shells,
c = 1 on the self-conjugate columns kx = 0 and 2 kx = W and 2 otherwise, so sum_k E(k) = mean(f^2); the cross-spectrum likewise.

Both functions continue a `state` over time chunks the way evaluate.rollout_diagnostics does, and chunks in time and batch give the
bits of one call.
"""
import math

import numpy as np
import torch

from . import lib as L
from . import sht

GRIDS = ("midpoint", "legendre-gauss", "equiangular")
_TABLES = {}
_SHELLS = {}


def fejer1_weights(n):
    """(theta [n], w [n]) float64: the nodes theta_j = (j + 1/2) pi / n and the weights of Fejer's first rule for the integral over
    cos(theta) in [-1, 1] (sum 2, all positive; exact for polynomials up to degree n - 1)."""
    n = int(n)
    if n < 1:
        raise ValueError(f"fejer1_weights: n = {n} must be positive")
    theta = (np.arange(n) + 0.5) * np.pi / n
    k = np.arange(1, n // 2 + 1)
    s = (np.cos(2.0 * np.outer(theta, k)) / (4.0 * k * k - 1.0)).sum(axis=1)
    return theta, 2.0 / n * (1.0 - 2.0 * s)


def sphere_tables_host(H, W, grid="midpoint", lmax=None):
    """(F [2 M, W], Wf [M, L, H]) in float64 with L = lmax or H and M = min(L, W // 2); rows in the grid's own order."""
    H, W = int(H), int(W)
    Lm = H if lmax is None else int(lmax)
    if grid not in GRIDS:
        raise ValueError(f"grid must be one of {GRIDS}, not {grid!r}")
    if not 1 <= Lm <= H:
        raise ValueError(f"lmax = {Lm} must lie in 1..H = {H}")
    if W < 2:
        raise ValueError(f"W = {W} must be at least 2")
    M = min(Lm, W // 2)
    if grid == "midpoint":
        theta, w = fejer1_weights(H)
        x = np.cos(theta)[::-1].copy()                        # south first: x_k = sin(lat_k), lat_k = -90 + d / 2 + d k
        Wf = sht.legpoly(M, Lm, x) * w[::-1][None, None, :]
        ang = 2.0 * np.pi * np.outer(np.arange(M), np.arange(W)) / W
        F = np.empty((2 * M, W))
        F[0::2] = 2.0 * np.pi / W * np.cos(ang)
        F[1::2] = -2.0 * np.pi / W * np.sin(ang)
    else:
        F, Wf, _, _ = sht.sht_tables(H, W, Lm, M, grid)
    return np.ascontiguousarray(F), np.ascontiguousarray(Wf)


def sphere_tables(H, W, grid="midpoint", lmax=None, device=None):
    """{"F", "Wf"} as fp32 tensors on `device` (rounded once from float64) with "L", "M", "H", "W", "grid"; cached."""
    key = (int(H), int(W), grid, None if lmax is None else int(lmax), str(device))
    tab = _TABLES.get(key)
    if tab is None:
        F, Wf = sphere_tables_host(H, W, grid, lmax)
        tab = {"F": torch.from_numpy(F).float().contiguous().to(device), "Wf": torch.from_numpy(Wf).float().contiguous().to(device),
               "L": Wf.shape[1], "M": Wf.shape[0], "H": int(H), "W": int(W), "grid": grid}
        _TABLES[key] = tab
    return tab


def plane_shells_host(H, W):
    """(rowptr [K + 1], entry [nnz], weight [nnz], K): per shell k the half-spectrum entries (index ky (W // 2 + 1) + kx, ascending)
    with rint(sqrt(kx^2 + ky^2)) = k and their weights c (1 on the columns kx = 0 and 2 kx = W, else 2)."""
    H, W = int(H), int(W)
    ky = np.rint(np.fft.fftfreq(H, 1.0 / H)).astype(np.int64)
    kx = np.arange(W // 2 + 1, dtype=np.int64)
    shell = np.rint(np.sqrt((ky[:, None] ** 2 + kx[None, :] ** 2).astype(np.float64))).astype(np.int64).reshape(-1)
    c = np.broadcast_to(np.where((kx == 0) | (2 * kx == W), 1.0, 2.0)[None, :], (H, W // 2 + 1)).reshape(-1)
    K = int(shell.max()) + 1
    order = np.argsort(shell, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(shell, minlength=K))])
    return rowptr.astype(np.int32), order.astype(np.int32), c[order].astype(np.float32), K


def _plane_shells(H, W, device):
    key = (int(H), int(W), str(device))
    tab = _SHELLS.get(key)
    if tab is None:
        rowptr, entry, weight, K = plane_shells_host(H, W)
        tab = {"rowptr": torch.from_numpy(rowptr).to(device), "entry": torch.from_numpy(entry).to(device),
               "weight": torch.from_numpy(weight).to(device), "K": K, "nnz": int(entry.size)}
        _SHELLS[key] = tab
    return tab


def _in_place(outputs):
    """(tensor, batch stride, time stride): `outputs` read in place when its trailing axes are dense and no stride is negative."""
    o = outputs
    dense = [int(np.prod(o.shape[k + 1:])) for k in range(2, o.dim())]
    if list(o.stride()[2:]) != dense or min(o.stride()[:2]) < 0:
        o = o.contiguous()
    return o, o.stride()[0], o.stride()[1]


def _chunk(Tc, t_begin, T):
    T = Tc if T is None else int(T)
    t_begin = int(t_begin)
    if t_begin < 0 or t_begin + Tc > T:
        raise ValueError(f"chunk [{t_begin}, {t_begin + Tc}) is outside the rollout of {T} frames")
    return t_begin, T


def sphere_spectra(outputs, targets, *, grid="midpoint", lmax=None, remap=None, state=None, t_begin=0, T=None):
    """One chunk of a rollout through dlwp_sphere_spectra.

    outputs   [Bc, Tc, V, H, W] (with `remap`: [Bc, Tc, V, 12, n, n], analysed on the remap's H x W grid) NORMALISED, on the GPU; batch
              and time strides are free (an expanded view is read in place).  None: the targets alone (power[0] and cross are zero).
    targets   the same shape.
    grid / lmax  see the module docstring; L = lmax or H degrees, M = min(L, W // 2) orders.
    state     the dictionary a previous time chunk of the SAME samples returned; t_begin / T as evaluate.rollout_diagnostics.

    Returns {"power" [2, Bc, T, V, L], "cross" [Bc, T, V, L], "a00" [2, Bc, T, V], "kind": "sphere", "grid", "frames"} on the GPU."""
    if targets.dim() < 5:
        raise ValueError(f"targets must be [B, T, V, H, W] (with a remap: [B, T, V, 12, n, n]), not {tuple(targets.shape)}")
    Bc, Tc, V = targets.shape[:3]
    if remap is not None:
        H, W, plane = remap.H, remap.W, (12, remap.nside, remap.nside)
    else:
        plane = tuple(targets.shape[3:])
        if len(plane) != 2:
            raise ValueError(f"targets must be [B, T, V, H, W], not {tuple(targets.shape)}")
        H, W = plane
    if tuple(targets.shape[3:]) != plane:
        raise ValueError(f"targets must be [B, T, V, {', '.join(map(str, plane))}], not {tuple(targets.shape)}")
    if outputs is not None and tuple(outputs.shape) != tuple(targets.shape):
        raise ValueError(f"outputs {tuple(outputs.shape)} and targets {tuple(targets.shape)} differ")
    if H > 256 or W > 512:
        raise ValueError(f"the grid {H} x {W} is above 256 x 512")
    t_begin, T = _chunk(Tc, t_begin, T)
    if grid not in GRIDS:
        raise ValueError(f"grid must be one of {GRIDS}, not {grid!r}")
    Lm = H if lmax is None else int(lmax)
    if not 1 <= Lm <= H:
        raise ValueError(f"lmax = {Lm} must lie in 1..H = {H}")
    if not targets.is_cuda or (outputs is not None and not outputs.is_cuda):
        raise L.DlwpError("libdlwpmi needs CUDA/HIP tensors (no CPU fallback)")
    dev = targets.device
    tab = sphere_tables(H, W, grid, lmax, dev)
    M = tab["M"]
    t = targets.contiguous()
    o, bs, ts = (None, 0, 0) if outputs is None else _in_place(outputs)
    if state is None:
        state = {"power": torch.zeros(2, Bc, T, V, Lm, device=dev), "cross": torch.zeros(Bc, T, V, Lm, device=dev),
                 "a00": torch.zeros(2, Bc, T, V, device=dev), "kind": "sphere", "grid": grid, "frames": 0}
    elif state.get("kind") != "sphere" or tuple(state["power"].shape) != (2, Bc, T, V, Lm) or state["grid"] != grid:
        raise ValueError("state belongs to another rollout (kind, shape or grid differ)")
    lib = L.load()
    nside = remap.nside if remap is not None else 0
    ws = L.workspace(lib.dlwp_sphere_spectra_ws_floats, Bc, Tc, V, H, W, Lm, M, nside, device=dev)
    hp = remap._hpx2ll if remap is not None else None
    L.check(lib.dlwp_sphere_spectra(None if o is None else o.data_ptr(), bs, ts, L.ptr(t), L.ptr(tab["F"]), L.ptr(tab["Wf"]),
                                    L.ptr(hp.idx) if hp else None, L.ptr(hp.w) if hp else None, nside, Bc, Tc, V, H, W, Lm, M, t_begin, T,
                                    L.ptr(state["power"]), L.ptr(state["cross"]), L.ptr(state["a00"]), L.ptr(ws), L.stream()))
    state["frames"] += Tc
    return state


def plane_spectra(outputs, targets, *, state=None, t_begin=0, T=None):
    """One chunk of a rollout of doubly periodic fields through dlwp_plane_spectra: outputs (or None) / targets [Bc, Tc, D, H, W] on the
    GPU, strides as `sphere_spectra`.  Returns {"power" [2, Bc, T, D, K], "cross" [Bc, T, D, K], "kind": "plane", "frames"}."""
    if targets.dim() != 5:
        raise ValueError(f"targets must be [B, T, D, H, W], not {tuple(targets.shape)}")
    if outputs is not None and tuple(outputs.shape) != tuple(targets.shape):
        raise ValueError(f"outputs {tuple(outputs.shape)} and targets {tuple(targets.shape)} differ")
    Bc, Tc, D, H, W = targets.shape
    if W < 2:
        raise ValueError(f"targets {tuple(targets.shape)}: W must be at least 2")
    t_begin, T = _chunk(Tc, t_begin, T)
    if not targets.is_cuda or (outputs is not None and not outputs.is_cuda):
        raise L.DlwpError("libdlwpmi needs CUDA/HIP tensors (no CPU fallback)")
    from . import fft
    dev = targets.device
    sh = _plane_shells(H, W, dev)
    K = sh["K"]
    t = targets.contiguous()
    o, bs, ts = (None, 0, 0) if outputs is None else _in_place(outputs)
    if state is None:
        state = {"power": torch.zeros(2, Bc, T, D, K, device=dev), "cross": torch.zeros(Bc, T, D, K, device=dev), "kind": "plane",
                 "frames": 0}
    elif state.get("kind") != "plane" or tuple(state["power"].shape) != (2, Bc, T, D, K):
        raise ValueError("state belongs to another rollout (kind or shape differ)")
    lib = L.load()
    ws = L.workspace(lib.dlwp_plane_spectra_ws_floats, Bc, Tc, D, H, W, device=dev)
    L.check(lib.dlwp_plane_spectra(fft._plan(H, W), None if o is None else o.data_ptr(), bs, ts, L.ptr(t), L.ptr(sh["rowptr"]),
                                   L.ptr(sh["entry"]), L.ptr(sh["weight"]), K, sh["nnz"], Bc, Tc, D, H, W, t_begin, T,
                                   L.ptr(state["power"]), L.ptr(state["cross"]), L.ptr(ws), L.stream()))
    state["frames"] += Tc
    return state


def concat_spectra(parts):
    """The tables of batch chunks (each a finished `sphere_spectra` / `plane_spectra` state) joined along the sample axis, on the host."""
    first = parts[0]
    out = {"power": torch.cat([p["power"].cpu() for p in parts], 1), "cross": torch.cat([p["cross"].cpu() for p in parts], 0),
           "kind": first["kind"], "frames": first["frames"]}
    if "a00" in first:
        out["a00"] = torch.cat([p["a00"].cpu() for p in parts], 1)
        out["grid"] = first["grid"]
    return out


def _derived(po, pt, cr):
    """the per-(.., degree) quantities from mean powers and cross-spectrum; 0 / 0 is nan"""
    ratio = po / pt
    below = ratio < 0.5
    first = torch.where(below.any(dim=-1), below.to(torch.int64).argmax(dim=-1), torch.full(below.shape[:-1], below.shape[-1], dtype=torch.int64))
    return {"power_out": po, "power_tgt": pt, "ratio": ratio, "error": po + pt - 2.0 * cr, "coherence": cr / torch.sqrt(po * pt),
            "half_power_degree": first}


def spectral_metrics(diag, scale=None, shift=None, window=None):
    """From the tables of `sphere_spectra` / `plane_spectra` (or `concat_spectra`), in float64 on the host, folded over the samples in
    index order: per (lead time, variable, degree or shell) the mean "power_out" / "power_tgt", their "ratio", the "error" power
    P_out + P_tgt - 2 cross (the power of output - target), the "coherence" cross / sqrt(P_out P_tgt) and, per (lead time,
    variable), "half_power_degree": the first degree at which the ratio falls below 1/2 (the number of degrees when none does).
    scale / shift per variable: the powers become physical, x scale^2 for every degree, degree 0 from a00 as
    (scale a00 + shift sqrt(4 pi))^2 / 4 pi (sphere tables only).  window = (w0, w1): "window" holds the same quantities from the
    powers averaged over the frames w0 .. w1 - 1."""
    p, c = diag["power"].double().cpu().clone(), diag["cross"].double().cpu().clone()
    B, T, V = c.shape[:3]
    if scale is not None or shift is not None:
        sc = torch.ones(V, dtype=torch.float64) if scale is None else torch.as_tensor(scale, dtype=torch.float64).reshape(-1)
        sh = torch.zeros(V, dtype=torch.float64) if shift is None else torch.as_tensor(shift, dtype=torch.float64).reshape(-1)
        if sc.numel() != V or sh.numel() != V:
            raise ValueError(f"scale / shift must have one entry per variable ({V}), not {sc.numel()} / {sh.numel()}")
        p *= (sc * sc)[None, None, None, :, None]
        c *= (sc * sc)[None, None, :, None]
        if bool((sh != 0).any()) or "a00" in diag:
            if "a00" not in diag:
                raise ValueError("a shift needs the a00 table of sphere_spectra")
            a = diag["a00"].double().cpu() * sc[None, None, None, :] + sh[None, None, None, :] * math.sqrt(4.0 * math.pi)
            p[..., 0] = a * a / (4.0 * math.pi)
            c[..., 0] = a[0] * a[1] / (4.0 * math.pi)
    pm, cm = torch.zeros_like(p[:, 0]), torch.zeros_like(c[0])
    for b in range(B):                                        # samples in index order
        pm += p[:, b]
        cm += c[b]
    pm, cm = pm / B, cm / B
    res = _derived(pm[0], pm[1], cm)
    if window is not None:
        w0, w1 = int(window[0]), int(window[1])
        if not 0 <= w0 < w1 <= T:
            raise ValueError(f"window [{w0}, {w1}) is outside [0, {T}] or empty")
        res["window"] = _derived(pm[0, w0:w1].mean(dim=0), pm[1, w0:w1].mean(dim=0), cm[w0:w1].mean(dim=0))
    return res
