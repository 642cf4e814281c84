"""Evaluation rollout and metrics on libdlwpmi.

nsbench (scripts/evaluate.py:26-85, 232-257): forward rollout without gradients over the test batches, then RMSE overall /
in teacher forcing / in closed loop and the accumulated error "Frob".  The reference slices its xarray dataset by
*label* -- `sel(time=slice(0, tf))`, `sel(time=slice(tf, T))` on the coordinate 0..T-1 (:109) -- so the teacher-forcing
window is [0, tf] inclusive and the closed-loop window [tf, T-1]: step tf belongs to both.  Reproduced as is.

dlwpbench (scripts/evaluate.py:494-546): latitude-weighted RMSE per (lead time, variable), w = cos(lat) / mean(cos(lat))
(Rasp et al. 2020 eq. 2), and the anomaly correlation coefficient against a climatology (eq. A1).

All reductions run in one kernel (dlwp_error_moments); only the [5, G] moment table reaches the host.  Models on the HEALPix mesh
are scored on lat-lon like the reference's (scripts/evaluate.py:71-109, 215-220 project outputs and targets first): dlwp_metrics_hpx
runs the same reduction with the HEALPix -> lat-lon interpolation inside the kernel (dlwp_hpx_error_moments, hpx_remap.HEALPixRemap).

Long rollouts (scripts/evaluate.py:548-588 and scripts/build_baselines.py): `rollout_diagnostics` reads a chunk of NORMALISED
outputs and targets once (dlwp_rollout_diag: de-normalisation, the monthly climatology selected per frame and, for HPX models, the
interpolation to lat-lon all happen inside the kernel) and leaves three small tables -- per-sample moments, zonal means and the sum
over a window of lead times -- from which `diag_metrics` (the dictionary of `dlwp_metrics`) and `physical_soundness` are finished on
the host in float64.  `evaluate_dlwp` is the driver beside `evaluate_ns`; `persistence_forecast` and `forecast="climatology"` are
the two baselines, `monthly_climatology` (dlwp_group_mean) the climatology itself.

Ensembles (`ensemble=M` of both drivers, off by default): the initial state is perturbed into M seeded members, the members run
through the model folded into the batch axis and are scored as a distribution -- CRPS, spread-skill ratio, rank histogram
(dlwp_benchmark_amd/ensemble.py); every deterministic key is computed from member 0.
"""
import math

import numpy as np
import torch

from . import lib as L


def error_moments(outputs, targets, climatology=None, row_weights=None):
    """outputs / targets / climatology [B, G, H, W] on the GPU -> moments [5, G] (see dlwpmi.h)."""
    B, G, H, W = outputs.shape
    m = torch.zeros(5, G, device=outputs.device)
    # the contiguous copies stay bound to locals until the launch is enqueued: a temporary freed between two ptr() calls
    # could hand its block to the next .contiguous() and alias both arguments
    o, t = outputs.contiguous(), targets.contiguous()
    c = climatology.contiguous() if climatology is not None else None
    w = row_weights.contiguous() if row_weights is not None else None
    L.check(L.load().dlwp_error_moments(L.ptr(o), L.ptr(t), L.ptr(c), L.ptr(w), B, G, H, W, L.ptr(m), L.stream()))
    return m


def ns_metrics(outputs, targets, teacher_forcing_steps):
    """outputs / targets [B, T, D, H, W] -> dict(rmse, rmse_tf, rmse_cl, frob, frob_tf, frob_cl) as Python floats."""
    B, T, D, H, W = outputs.shape
    m = error_moments(outputs.reshape(B, T, D * H, W), targets.reshape(B, T, D * H, W)).double().cpu()
    n = B * D * H * W                                 # elements per time step
    tf = int(teacher_forcing_steps)
    win = {"": (0, T), "_tf": (0, min(tf + 1, T)), "_cl": (min(tf, T), T)}    # label-inclusive slices, see module docstring
    out = {}
    for tag, (a, b) in win.items():
        cnt = max(b - a, 0) * n
        out["rmse" + tag] = math.sqrt(m[0, a:b].sum().item() / cnt) if cnt else float("nan")
        out["frob" + tag] = (m[1, a:b] / n).sum().item()
    return out


def _ensemble_args(ensemble, sigma, seed):
    """(M, sigma, seed) of the drivers' ensemble keywords, validated before the first batch"""
    from . import ensemble as E
    M = int(ensemble)
    if not 2 <= M <= E.MAX_MEMBERS:
        raise ValueError(f"ensemble = {M} members must lie in 2..{E.MAX_MEMBERS}")
    sg = np.asarray(sigma, dtype=np.float64).reshape(-1)
    if not (np.isfinite(sg).all() and (sg >= 0).all()):
        raise ValueError(f"ensemble_sigma {sg.tolist()} must be finite and not negative")
    return M, (float(sg[0]) if sg.size == 1 else sg), E._check_seed(float(sg.max()), seed)


def _host_tables(d):
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}


@torch.no_grad()
def evaluate_ns(model, batches, teacher_forcing_steps, spectra=False, ensemble=None, ensemble_sigma=0.0, ensemble_seed=None,
                ensemble_control=True):
    """evaluate_model (:26-85) without the NetCDF detour: rollout every (x, y) batch, accumulate the moments on device.
    spectra=True adds "spectra": `spectra.spectral_metrics` of the shell-binned spectra E(k) of outputs and targets
    (`spectra.plane_spectra`) and the raw tables under "tables".
    ensemble=M adds "ensemble": the input x of every sample is perturbed into M members (`ensemble.perturb_members` with
    `ensemble_sigma`, `ensemble_seed`, `ensemble_control`; the item is the running sample index over `batches`), the members run
    through the model folded into the batch axis, and `ensemble.ensemble_metrics` of their rollouts is reported per lead time
    (unweighted, no scale), the raw tables under "tables".  Every other key is computed from member 0."""
    tot, shape, sparts, eparts, seen = None, None, [], [], 0
    if ensemble is not None:
        from . import ensemble as E
        M, sigma, seed = _ensemble_args(ensemble, ensemble_sigma, ensemble_seed)
    for x, y in batches:
        if ensemble is not None:
            Bx = x.shape[0]
            xm = E.perturb_members(x, np.arange(seen, seen + Bx), M, sigma, seed, control=ensemble_control, variables=x.shape[-3])
            seen += Bx
            ym = model(xm.reshape(Bx * M, *x.shape[1:]), teacher_forcing_steps)
            ym = ym.reshape(Bx, M, *ym.shape[1:])
            eparts.append(_host_tables(E.ensemble_diagnostics(ym, y)))
            y_hat = ym[:, 0]
        else:
            y_hat = model(x, teacher_forcing_steps)
        B, T, D, H, W = y_hat.shape
        if spectra:
            from . import spectra as S
            sparts.append({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in S.plane_spectra(y_hat, y).items()})
        m = error_moments(y_hat.reshape(B, T, D * H, W), y.reshape(B, T, D * H, W))
        tot = m if tot is None else tot + m
        shape = (shape[0] + B, T, D, H, W) if shape else (B, T, D, H, W)
    B, T, D, H, W = shape
    n, tf, m = B * D * H * W, int(teacher_forcing_steps), tot.double().cpu()
    out = {}
    for tag, (a, b) in {"": (0, T), "_tf": (0, min(tf + 1, T)), "_cl": (min(tf, T), T)}.items():
        cnt = max(b - a, 0) * n
        out["rmse" + tag] = math.sqrt(m[0, a:b].sum().item() / cnt) if cnt else float("nan")
        out["frob" + tag] = (m[1, a:b] / n).sum().item()
    if spectra:
        from . import spectra as S
        tables = S.concat_spectra(sparts)
        out["spectra"] = S.spectral_metrics(tables)
        out["spectra"]["tables"] = tables
    if ensemble is not None:
        tables = E.concat_ensemble(eparts)
        out["ensemble"] = E.ensemble_metrics(tables)
        out["ensemble"]["tables"] = tables
    return out


def lat_weights(lats_deg, device=None):
    lats = torch.deg2rad(torch.as_tensor(lats_deg, dtype=torch.float64))
    w = torch.cos(lats) / torch.cos(lats).mean()
    return w.float().to(device) if device is not None else w.float()


def dlwp_metrics(outputs, targets, lats_deg, climatology=None):
    """outputs / targets (/ climatology) [B, T, V, H, W] -> rmse [T, V] (and acc [T, V]) tensors on the host."""
    B, T, V, H, W = outputs.shape
    w = lat_weights(lats_deg, outputs.device)
    clim = climatology.reshape(B, T * V, H, W) if climatology is not None else None
    m = error_moments(outputs.reshape(B, T * V, H, W), targets.reshape(B, T * V, H, W), clim, w).double().cpu()
    res = {"rmse": torch.sqrt(m[0] / (B * H * W)).reshape(T, V)}
    if climatology is not None:
        res["acc"] = (m[2] / torch.sqrt(m[3] * m[4])).reshape(T, V)
    return res


def hpx_error_moments(outputs, targets, remap, climatology=None, row_weights=None):
    """outputs / targets [B, G, 12, n, n] on the GPU, climatology [B, G, H, W] on the remap's lat-lon grid -> moments [5, G] of
    hpx2ll(outputs), hpx2ll(targets): the interpolation runs inside the reduction kernel (dlwp_hpx_error_moments)."""
    B, G, F, n, n2 = outputs.shape
    if (F, n, n2) != (12, remap.nside, remap.nside) or targets.shape != outputs.shape:
        raise ValueError(f"outputs / targets must be [B, G, 12, {remap.nside}, {remap.nside}], not {tuple(outputs.shape)} / {tuple(targets.shape)}")
    if climatology is not None and tuple(climatology.shape) != (B, G, remap.H, remap.W):
        raise ValueError(f"climatology must be [{B}, {G}, {remap.H}, {remap.W}], not {tuple(climatology.shape)}")
    m = torch.zeros(5, G, device=outputs.device)
    o, t = outputs.contiguous(), targets.contiguous()      # (bound to locals until the launch is enqueued, see error_moments)
    c = climatology.contiguous() if climatology is not None else None
    w = row_weights.contiguous() if row_weights is not None else None
    tab = remap._hpx2ll
    L.check(L.load().dlwp_hpx_error_moments(L.ptr(o), L.ptr(t), L.ptr(c), L.ptr(w), L.ptr(tab.idx), L.ptr(tab.w), B, G, remap.nside,
                                            remap.H, remap.W, L.ptr(m), L.stream()))
    return m


def dlwp_metrics_hpx(outputs, targets, remap, climatology=None):
    """`dlwp_metrics` for models on the HEALPix mesh, scored on the lat-lon grid of `remap` (an hpx_remap.HEALPixRemap) as the
    reference scores its HPX models (scripts/evaluate.py:71-109, 215-220 project to lat-lon first): outputs / targets
    [B, T, V, 12, n, n], climatology [B, T, V, H, W] on lat-lon -> rmse [T, V] (and acc [T, V]) tensors on the host."""
    B, T, V = outputs.shape[:3]
    H, W = remap.H, remap.W
    w = lat_weights(remap.lats_deg, outputs.device)
    clim = climatology.reshape(B, T * V, H, W) if climatology is not None else None
    m = hpx_error_moments(outputs.reshape(B, T * V, *outputs.shape[3:]), targets.reshape(B, T * V, *targets.shape[3:]), remap, clim,
                          w).double().cpu()
    res = {"rmse": torch.sqrt(m[0] / (B * H * W)).reshape(T, V)}
    if climatology is not None:
        res["acc"] = (m[2] / torch.sqrt(m[3] * m[4])).reshape(T, V)
    return res


# ---- long-rollout diagnostics (csrc/rollout_diag.hip) ------------------------------------------------------------------------------
def forecast_months(init_dates, T, timedelta_hours):
    """int32 [B, T], 0 = January: the month of init date + lead time, lead i being (i + 1) * timedelta after the init date -- the
    `time` coordinate build_dataset writes (scripts/evaluate.py:263-269) added to `sample` as build_baselines.py:66 does."""
    d = np.asarray(init_dates).astype("datetime64[h]")
    lead = (np.arange(int(T), dtype=np.int64) + 1) * int(timedelta_hours)
    valid = d[:, None] + lead[None, :].astype("timedelta64[h]")
    return (valid.astype("datetime64[M]").astype(np.int64) % 12).astype(np.int32)


def lead_window(day_from, day_to, timedelta_hours, T):
    """(w0, w1): the frames of `sel(time=slice(Timedelta(day_from, "d"), Timedelta(day_to, "d")))` (scripts/evaluate.py:584) as a
    half-open index range; the slice is by label and includes both ends, frame i carries the label (i + 1) * timedelta."""
    dt = float(timedelta_hours)
    w0 = max(math.ceil(day_from * 24 / dt) - 1, 0)           # first i with (i + 1) dt >= day_from * 24 h
    w1 = min(math.floor(day_to * 24 / dt), int(T))           # one past the last i with (i + 1) dt <= day_to * 24 h
    return (min(w0, w1), w1)


def persistence_forecast(inits, T):
    """inits [B, V, ...] -> the persistence forecast [B, T, V, ...] (build_baselines.py:23-28) as an expanded VIEW: time stride 0,
    which dlwp_rollout_diag reads in place."""
    return inits.unsqueeze(1).expand(inits.shape[0], int(T), *inits.shape[1:])


def monthly_climatology(fields, months, groups=12):
    """fields [N, ...] on the GPU, months [N] integers in 0..groups-1 -> (mean [groups, ...], count [groups] int32): the
    `groupby(time.dt.month).mean()` of build_baselines.py:62 (dlwp_group_mean; an empty group gives a zero map and count 0)."""
    m = np.asarray(months.cpu() if torch.is_tensor(months) else months)
    N = fields.shape[0]
    if m.shape != (N,) or not np.issubdtype(m.dtype, np.integer):
        raise ValueError(f"months must be {N} integers, not {m.dtype} {m.shape}")
    if N and (m.min() < 0 or m.max() >= groups):
        raise ValueError(f"months must lie in 0..{groups - 1}, found {int(m.min())}..{int(m.max())}")
    f = fields.contiguous()
    P = f.numel() // N
    g = torch.from_numpy(m.astype(np.int32)).to(f.device)
    mean = torch.empty((groups,) + tuple(f.shape[1:]), device=f.device)
    count = torch.empty(groups, dtype=torch.int32, device=f.device)
    L.check(L.load().dlwp_group_mean(L.ptr(f), L.ptr(g), L.ptr(mean), L.ptr(count), N, P, groups, L.stream()))
    return mean, count


def _per_variable(x, V, device, name):
    if x is None:
        return None
    t = torch.as_tensor(x, dtype=torch.float32).reshape(-1).to(device).contiguous()
    if t.numel() != V:
        raise ValueError(f"{name} must have one entry per variable ({V}), not {t.numel()}")
    return t


def rollout_diagnostics(outputs, targets, *, scale=None, shift=None, lats_deg=None, remap=None, climatology=None, months=None,
                        window=None, state=None, t_begin=0, T=None):
    """One chunk of a rollout through dlwp_rollout_diag.

    outputs   [Bc, Tc, V, H, W] (with `remap`: [Bc, Tc, V, 12, n, n]) NORMALISED model outputs on the GPU; batch and time strides are
              free (an expanded view such as `persistence_forecast` is read in place), the trailing axes are made dense if they
              are not.  None: the forecast is the climatology.
    targets   the same shape, normalised.
    scale / shift  per variable, physical = x * scale + shift (None: identity).
    lats_deg  latitudes of the lat-lon rows for the cos(lat) weights of the moments (None: unweighted).
    remap     an hpx_remap.HEALPixRemap: outputs / targets are HEALPix planes scored on its lat-lon grid.
    climatology [M, V, H, W] in physical units with months [Bc, Tc] (integers in 0..M-1, checked here on the host).
    window    (w0, w1) global frame indices whose sum is kept per pixel (None: no window).
    state     the dictionary a previous time chunk of the SAME samples returned: its tables are continued.
    t_begin / T  global index of the chunk's first frame and the whole rollout's length (default: the chunk is the rollout).

    Returns {"moments" [Bc, T, V, 5], "zonal" [2, Bc, T, V, H], "wsum" [2, Bc, V, H, W] (normalised sums), "scale", "shift", "window",
    "frames" (chunk frames seen so far)} on the GPU.  Chunks in time and in batch give the bits of one call."""
    Bc, Tc, V = targets.shape[:3]
    dev = targets.device
    if remap is not None:
        H, W, plane = remap.H, remap.W, (12, remap.nside, remap.nside)
    else:
        H, W = targets.shape[3:]
        plane = (H, W)
    if tuple(targets.shape[3:]) != plane:
        raise ValueError(f"targets must be [B, T, V, {', '.join(map(str, plane))}], not {tuple(targets.shape)}")
    if outputs is not None and tuple(outputs.shape) != tuple(targets.shape):
        raise ValueError(f"outputs {tuple(outputs.shape)} and targets {tuple(targets.shape)} differ")
    if outputs is None and climatology is None:
        raise ValueError("outputs=None means the climatology forecast: give a climatology")
    if (climatology is None) != (months is None):
        raise ValueError("climatology and months go together")
    T = Tc if T is None else int(T)
    t_begin = int(t_begin)
    if t_begin < 0 or t_begin + Tc > T:
        raise ValueError(f"chunk [{t_begin}, {t_begin + Tc}) is outside the rollout of {T} frames")
    w0, w1 = (0, 0) if window is None else (int(window[0]), int(window[1]))
    if not 0 <= w0 <= w1 <= T:
        raise ValueError(f"window [{w0}, {w1}) is outside [0, {T}]")
    t = targets.contiguous()
    o, bs, ts = None, 0, 0
    if outputs is not None:
        o = outputs
        dense = [int(np.prod(o.shape[k + 1:])) for k in range(2, o.dim())]
        if list(o.stride()[2:]) != dense or min(o.stride()[:2]) < 0:
            o = o.contiguous()
        bs, ts = o.stride()[:2]
    sc, sh = _per_variable(scale, V, dev, "scale"), _per_variable(shift, V, dev, "shift")
    roww = lat_weights(lats_deg, dev).contiguous() if lats_deg is not None else None
    if roww is not None and roww.numel() != H:
        raise ValueError(f"lats_deg must have {H} entries, not {roww.numel()}")
    clim, mon, M = None, None, 0
    if climatology is not None:
        M = climatology.shape[0]
        if tuple(climatology.shape) != (M, V, H, W):
            raise ValueError(f"climatology must be [M, {V}, {H}, {W}], not {tuple(climatology.shape)}")
        m = np.asarray(months.cpu() if torch.is_tensor(months) else months)
        if m.shape != (Bc, Tc) or not np.issubdtype(m.dtype, np.integer):
            raise ValueError(f"months must be [{Bc}, {Tc}] integers, not {m.dtype} {m.shape}")
        if m.min() < 0 or m.max() >= M:
            raise ValueError(f"months must lie in 0..{M - 1}, found {int(m.min())}..{int(m.max())}")
        clim, mon = climatology.contiguous(), torch.from_numpy(np.ascontiguousarray(m.astype(np.int32))).to(dev)
    if not targets.is_cuda or (outputs is not None and not outputs.is_cuda):
        raise L.DlwpError("libdlwpmi needs CUDA/HIP tensors (no CPU fallback)")
    if state is None:
        state = {"moments": torch.zeros(Bc, T, V, 5, device=dev), "zonal": torch.zeros(2, Bc, T, V, H, device=dev),
                 "wsum": torch.zeros(2, Bc, V, H, W, device=dev), "window": (w0, w1), "frames": 0}
    elif (tuple(state["moments"].shape) != (Bc, T, V, 5) or tuple(state["wsum"].shape) != (2, Bc, V, H, W)
          or state["window"] != (w0, w1)):
        raise ValueError("state belongs to another rollout (shape or window differ)")
    lib = L.load()
    n_ws = lib.dlwp_rollout_diag_ws_floats(Bc, Tc, V, H, W, int(remap is not None))
    if n_ws < 0:
        L.check(int(n_ws))
    ws = torch.empty(n_ws, device=dev)
    tab = remap._hpx2ll if remap is not None else None
    L.check(lib.dlwp_rollout_diag(None if o is None else o.data_ptr(), bs, ts, L.ptr(t), L.ptr(sc), L.ptr(sh), L.ptr(roww), L.ptr(clim),
                                  L.ptr(mon), M, L.ptr(tab.idx) if tab else None, L.ptr(tab.w) if tab else None,
                                  remap.nside if remap is not None else 0, Bc, Tc, V, H, W, t_begin, T, w0, w1,
                                  L.ptr(state["moments"]), L.ptr(state["zonal"]), L.ptr(state["wsum"]), L.ptr(ws), L.stream()))
    state["scale"], state["shift"], state["frames"] = sc, sh, state["frames"] + Tc
    return state


def concat_diagnostics(parts):
    """The tables of batch chunks (each a finished `rollout_diagnostics` state) joined along the sample axis, on the host."""
    first = parts[0]
    out = {"moments": torch.cat([p["moments"].cpu() for p in parts], 0), "zonal": torch.cat([p["zonal"].cpu() for p in parts], 1),
           "wsum": torch.cat([p["wsum"].cpu() for p in parts], 1), "window": first["window"],
           "scale": None if first["scale"] is None else first["scale"].cpu(),
           "shift": None if first["shift"] is None else first["shift"].cpu(), "frames": first["frames"]}
    return out


def diag_metrics(diag):
    """The dictionary of `dlwp_metrics` -- rmse [T, V] (and acc [T, V] when a climatology was given: any of its moments nonzero) --
    from the per-sample moment table, folded over the samples in index order in float64 on the host."""
    m = diag["moments"].double().cpu()
    B, T, V, _ = m.shape
    H, W = diag["wsum"].shape[-2:]
    tot = torch.zeros(T, V, 5, dtype=torch.float64)
    for b in range(B):
        tot += m[b]
    res = {"rmse": torch.sqrt(tot[..., 0] / (B * H * W))}
    if bool((tot[..., 3] != 0).any() or (tot[..., 4] != 0).any()):
        res["acc"] = tot[..., 2] / torch.sqrt(tot[..., 3] * tot[..., 4])
    return res


def latitude_band(lats_deg, lo, hi):
    """Row mask of xarray's `sel(lat=slice(lo, hi))`: by label, both ends included."""
    lats = np.asarray(lats_deg, dtype=np.float64)
    return (lats >= lo) & (lats <= hi)


def physical_soundness(diag, lats_deg, window_len):
    """scripts/evaluate.py:551-588 from the tables of `rollout_diagnostics`, per variable ([V] float64 tensors): the RMSE of the time-
    and longitude-mean fields over (sample, lat) -- globally, on the trade-wind bands slice(-20, -10) U slice(10, 20) and on the
    south-westerlies band slice(-55, -45) (label slices on `lats_deg`, both ends included) -- and the RMSE of the window-mean fields
    over (sample, lat, lon); all means unweighted, as the reference's.  `window_len` = w1 - w0 frames."""
    z = diag["zonal"].double().cpu()                          # [2, B, T, V, H]
    d = z[0].mean(dim=1) - z[1].mean(dim=1)                   # [B, V, H]
    lats = np.asarray(lats_deg, dtype=np.float64)
    if lats.shape != (z.shape[-1],):
        raise ValueError(f"lats_deg must have {z.shape[-1]} entries")
    trade = torch.from_numpy(latitude_band(lats, -20, -10) | latitude_band(lats, 10, 20))
    south = torch.from_numpy(latitude_band(lats, -55, -45))

    def rmse(x):
        return torch.sqrt((x ** 2).mean(dim=(0, 2)))

    w = diag["wsum"].double().cpu()                           # [2, B, V, H, W], normalised sums
    sc = torch.ones(w.shape[2], dtype=torch.float64) if diag.get("scale") is None else diag["scale"].double().cpu()
    dw = (w[0] - w[1]) / float(window_len) * sc[None, :, None, None] if window_len else torch.full_like(w[0], float("nan"))
    return {"rmse_global": rmse(d), "rmse_trade_winds": rmse(d[:, :, trade]), "rmse_south_westerlies": rmse(d[:, :, south]),
            "rmse_window": torch.sqrt((dw ** 2).mean(dim=(0, 2, 3)))}


def dataset_scale_shift(dataset):
    """(scale, shift) per prognostic channel from the dataset's z-score table, in the order scripts/evaluate.py:198-213 walks the
    channels (levels of a variable first); (None, None) for a dataset that does not normalise."""
    if not dataset.normalize:
        return None, None
    scale, shift = [], []
    for p, levels in dataset.prognostic_variable_names_and_levels.items():
        for st in ([dataset.stats[p]["level"][l] for l in levels] if levels else [dataset.stats[p]]):
            scale.append(float(st["std"]))
            shift.append(float(st["mean"]))
    return scale, shift


def regular_latitudes(H):
    """The `lat` coordinate build_dataset writes (scripts/evaluate.py:270): -90 + d / 2 + d k, d = 180 / H (5.625 for 32 rows)."""
    d = 180.0 / H
    return -90.0 + d / 2 + d * np.arange(H)


@torch.no_grad()
def evaluate_dlwp(model, dataset, batch_size, *, forecast="model", remap=None, climatology=None, window_days=(334, 365), lats_deg=None,
                  device=None, spectra=False, spectra_grid="midpoint", ensemble=None, ensemble_sigma=0.0, ensemble_seed=None,
                  ensemble_control=True):
    """evaluate_model + compute_metrics (scripts/evaluate.py:112-234, 494-588) without the NetCDF detour, batch by batch, with nothing
    but the diagnostic tables leaving the device.

    dataset   a wbdata.WeatherBenchArrays on its `init_dates` branch; constants / prescribed that are NaN are passed as None
              (:180-189); scale and shift come from its z-score table (`dataset_scale_shift`).
    forecast  "model" (model(constants, prescribed, prognostic)), "persistence" (the first prognostic frame held, build_baselines.py:
              23-28) or "climatology" (needs `climatology`; the model is not called).
    remap     an hpx_remap.HEALPixRemap for the models on the HEALPix mesh: scored on its lat-lon grid.
    climatology [12, V, H, W] monthly maps in physical units (`monthly_climatology`): enables the ACC.
    spectra   True: also the power per spherical-harmonic degree of outputs and targets (`spectra.sphere_spectra` on `spectra_grid`,
              for HPX models on the remap's lat-lon grid): "spectra" holds `spectra.spectral_metrics` in physical units, over all lead
              times and over the window, and the raw tables under "tables".
    ensemble  M (2..64; forecast="model" only): `prognostic` of every sample is perturbed into M members (`ensemble.perturb_members`
              with `ensemble_sigma` -- a scalar or one value per prognostic channel, normalised units --, `ensemble_seed` and
              `ensemble_control`; the item is the dataset index, so a member does not depend on the batch size), the members run
              through the model folded into the batch axis (B M samples, constants and prescribed repeated), and "ensemble" holds
              `ensemble.ensemble_metrics` in physical units with the raw tables under "tables".  Every other key is computed from
              member 0 (the unperturbed forecast under `ensemble_control`).
    Returns rmse [T, V] (acc [T, V]), rmse_global / rmse_trade_winds / rmse_south_westerlies / rmse_window [V], "window", "diag"."""
    if forecast not in ("model", "persistence", "climatology"):
        raise ValueError(f"forecast must be 'model', 'persistence' or 'climatology', not {forecast!r}")
    if forecast == "climatology" and climatology is None:
        raise ValueError("forecast='climatology' needs the climatology")
    if dataset.init_dates is None:
        raise ValueError("evaluate_dlwp iterates the dataset's init_dates branch: construct it with init_dates")
    if ensemble is not None:
        if forecast != "model":
            raise ValueError(f"ensemble needs forecast='model': the {forecast} forecast has no members")
        from . import ensemble as E
        M, sigma, seed = _ensemble_args(ensemble, ensemble_sigma, ensemble_seed)
    from . import wbdata
    device = device if device is not None else (climatology.device if climatology is not None else next(model.parameters()).device)
    scale, shift = dataset_scale_shift(dataset)
    parts, sparts, eparts, lats, window = [], [], [], None, None
    for i0 in range(0, len(dataset), int(batch_size)):
        items = list(range(i0, min(i0 + int(batch_size), len(dataset))))
        constants, prescribed, prognostic, target = wbdata.to_device_batch([dataset[i] for i in items], device)
        constants = None if constants is None or bool(constants.isnan().any()) else constants
        prescribed = None if prescribed is None or bool(prescribed.isnan().any()) else prescribed
        T = target.shape[1]
        members = None
        if ensemble is not None:
            B = prognostic.shape[0]
            pm = E.perturb_members(prognostic, np.asarray(items), M, sigma, seed, control=ensemble_control, variables=prognostic.shape[2])
            fold = lambda a: None if a is None else a.repeat_interleave(M, dim=0)      # noqa: E731
            members = model(constants=fold(constants), prescribed=fold(prescribed), prognostic=pm.reshape(B * M, *prognostic.shape[1:]))
            members = members.reshape(B, M, *members.shape[1:])
            out = members[:, 0]
        elif forecast == "model":
            out = model(constants=constants, prescribed=prescribed, prognostic=prognostic)
        elif forecast == "persistence":
            out = persistence_forecast(prognostic[:, 0], T)
        else:
            out = None
        if lats is None:
            H = remap.H if remap is not None else target.shape[-2]
            lats = np.asarray(remap.lats_deg if remap is not None else (lats_deg if lats_deg is not None else regular_latitudes(H)))
            window = lead_window(window_days[0], window_days[1], dataset.timedelta, T)
        months = forecast_months(dataset.init_dates[items], T, dataset.timedelta) if climatology is not None else None
        d = rollout_diagnostics(out, target, scale=scale, shift=shift, lats_deg=lats, remap=remap, climatology=climatology,
                                months=months, window=window)
        parts.append({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()})
        if members is not None:
            eparts.append(_host_tables(E.ensemble_diagnostics(members, target, lats_deg=lats, remap=remap)))
        if spectra:
            from . import spectra as S
            sp = S.sphere_spectra(out, target, grid=spectra_grid, remap=remap)
            sparts.append({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sp.items()})
    diag = concat_diagnostics(parts)
    res = diag_metrics(diag)
    res.update(physical_soundness(diag, lats, window[1] - window[0]))
    res["window"], res["diag"] = window, diag
    if spectra:
        from . import spectra as S
        tables = S.concat_spectra(sparts)
        res["spectra"] = S.spectral_metrics(tables, scale=scale, shift=shift, window=window if window[1] > window[0] else None)
        res["spectra"]["tables"] = tables
    if ensemble is not None:
        tables = E.concat_ensemble(eparts)
        res["ensemble"] = E.ensemble_metrics(tables, scale=scale)
        res["ensemble"]["tables"] = tables
    return res
