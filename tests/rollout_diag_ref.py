"""TEST INFRASTRUCTURE ONLY -- float64 numpy restatement of the dlwpbench long-rollout evaluation, for tests/test_*rollout_diag*.py.

Restated (not copied) from the reference, with xarray's label-based selection spelled out in numpy indices because xarray is not in
this image (PARITY UNPINNED for that reading; the arithmetic itself is elementary):
    denormalise         <- src/dlwpbench/scripts/evaluate.py:197-213   x * std + mean per prognostic channel
    lat_coordinate      <- :270                                        -90 + 5.625 / 2 + 5.625 k  (180 / H in general)
    time_labels_hours   <- :263-264                                    timedelta_range(start = dt, periods = T, freq = dt): (i + 1) dt
    rmse_acc            <- :514-546                                    latitude-weighted RMSE and ACC per (lead time, variable)
    physical_soundness  <- :551-588                                    RMSE of time- and longitude-mean fields (global, trade winds,
                                                                       south westerlies) and of the month 11-12 time-mean fields
    persistence         <- scripts/build_baselines.py:23-28            the initial condition broadcast over the lead times
    monthly_climatology <- :52-62                                      groupby(time.dt.month).mean()
    climatology_forecast<- :63-67                                      the monthly map of (sample + time).month per frame
All inputs and results are float64; arrays are [sample, time, variable, lat, lon].
"""
import warnings

import numpy as np


def denormalise(x, scale, shift):
    x = np.asarray(x, dtype=np.float64)
    if scale is None:
        return x
    s = np.asarray(scale, dtype=np.float64).reshape(1, 1, -1, 1, 1)
    m = np.asarray(shift, dtype=np.float64).reshape(1, 1, -1, 1, 1)
    return x * s + m


def lat_coordinate(H):
    d = 180.0 / H
    return -90.0 + d / 2 + d * np.arange(H)                                   # :270 with deg = 5.625 for H = 32


def time_labels_hours(T, timedelta_hours):
    return (np.arange(T) + 1) * float(timedelta_hours)                        # :263-264


def label_slice(coord, lo, hi):
    """indices of `sel(coord=slice(lo, hi))` on an ascending coordinate: both ends included"""
    coord = np.asarray(coord, dtype=np.float64)
    return np.nonzero((coord >= lo) & (coord <= hi))[0]


def rmse_acc(outputs, targets, lats_deg, climatology=None):
    """:514-546.  lats_deg None: unweighted (all weights 1)."""
    o, t = np.asarray(outputs, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    if lats_deg is None:
        w = np.ones((1, 1, 1, o.shape[3], 1))
    else:
        lr = np.deg2rad(np.asarray(lats_deg, dtype=np.float64))               # :516-518
        w = (np.cos(lr) / np.mean(np.cos(lr)))[None, None, None, :, None]
    res = {"rmse": np.sqrt((w * (o - t) ** 2).mean(axis=(0, 3, 4)))}          # :527-528
    if climatology is not None:
        c = np.asarray(climatology, dtype=np.float64)
        oc, tc = o - c, t - c                                                 # :539-540
        nom = (w * oc * tc).mean(axis=(0, 3, 4))
        den = np.sqrt((w * oc ** 2).mean(axis=(0, 3, 4)) * (w * tc ** 2).mean(axis=(0, 3, 4)))
        res["acc"] = nom / den                                                # :541-545
    return res


def physical_soundness(outputs, targets, lats_deg, timedelta_hours, day_from=334, day_to=365):
    """:551-588 per variable ([V] arrays)."""
    o, t = np.asarray(outputs, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    lats = np.asarray(lats_deg, dtype=np.float64)
    avg_tar, avg_out = t.mean(axis=(1, 4)), o.mean(axis=(1, 4))               # :555-556  [sample, variable, lat]
    d = avg_out - avg_tar
    trade = np.concatenate([label_slice(lats, -20, -10), label_slice(lats, 10, 20)])      # :563-564
    south = label_slice(lats, -55, -45)                                       # :571-572
    frames = label_slice(time_labels_hours(o.shape[1], timedelta_hours), day_from * 24.0, day_to * 24.0)      # :584-585
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)                       # a band or a window without members: nan, as xarray gives
        res = {"rmse_global": np.sqrt((d ** 2).mean(axis=(0, 2))),                          # :557
               "rmse_trade_winds": np.sqrt((d[:, :, trade] ** 2).mean(axis=(0, 2))),        # :565
               "rmse_south_westerlies": np.sqrt((d[:, :, south] ** 2).mean(axis=(0, 2)))}   # :573
        dw = o[:, frames].mean(axis=1) - t[:, frames].mean(axis=1)
        res["rmse_window"] = np.sqrt((dw ** 2).mean(axis=(0, 2, 3)))          # :586
    res["window_frames"] = frames
    return res


def persistence(inits, T):
    """build_baselines.py:23-28: inits [sample, variable, lat, lon] -> [sample, T, variable, lat, lon]"""
    x = np.asarray(inits, dtype=np.float64)
    return np.broadcast_to(x[:, None], (x.shape[0], T) + x.shape[1:]).copy()


def monthly_climatology(fields, months, groups=12):
    """build_baselines.py:62: fields [time, ...], months [time] in 0..groups-1 -> (mean [groups, ...] with zero rows for empty groups,
    count [groups])"""
    f, m = np.asarray(fields, dtype=np.float64), np.asarray(months)
    mean, count = np.zeros((groups,) + f.shape[1:]), np.zeros(groups, dtype=np.int64)
    for g in range(groups):
        sel = m == g
        count[g] = sel.sum()
        if count[g]:
            mean[g] = f[sel].mean(axis=0)
    return mean, count


def forecast_months(init_dates, T, timedelta_hours):
    """build_baselines.py:66 with the `time` coordinate of scripts/evaluate.py:263-264: month (0 = January) of init + (i + 1) dt"""
    out = np.zeros((len(init_dates), T), dtype=np.int64)
    for s, d in enumerate(np.asarray(init_dates).astype("datetime64[h]")):
        for i in range(T):
            valid = d + np.timedelta64(int((i + 1) * timedelta_hours), "h")
            out[s, i] = int(str(valid.astype("datetime64[M]"))[5:7]) - 1
    return out


def climatology_forecast(clim, months):
    """build_baselines.py:63-67: clim [12, variable, lat, lon], months [sample, T] -> [sample, T, variable, lat, lon]"""
    return np.asarray(clim, dtype=np.float64)[np.asarray(months)]
