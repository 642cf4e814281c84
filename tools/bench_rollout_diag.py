#!/usr/bin/env python3
"""Time of the long-rollout diagnostics launch (csrc/rollout_diag.hip: dlwp_rollout_diag + its moment fold) beside the same tables
computed from the pieces the library had before it, and beside the HBM roof of its algorithmic bytes, in one run.

Shape: the benchmark's one-year rollout, T = 1460 frames (365 days at 6 h), V = 8 variables, scored on 32 x 64, at a batch that fits
(--batch, default 8: 0.77 GB per lat-lon tensor); once with lat-lon planes and once with HPX8 planes interpolated in the kernel.
Window = lead_window(334, 365, 6, 1460) = frames 1335..1459.  Per mesh one JSON line:

    fused        dlwp_rollout_diag on pre-uploaded operands (normalised outputs / targets, scale / shift, monthly climatology [12, V, H, W],
                 months [B, T], row weights) -> moments [B, T, V, 5], zonal [2, B, T, V, H], wsum [2, B, V, H, W]
    composition  the parent commit's route to the same tables: torch de-normalise of outputs and targets, the expanded climatology
                 clim[months] [B, T, V, H, W], (HPX: HEALPixRemap.hpx2ll of both tensors first,) evaluate.error_moments
                 (dlwp_error_moments; its table is already folded over the batch), torch means over longitude and over the window
    roof         algorithmic bytes (one read of outputs and targets) / HBM bandwidth, at the 8 TB/s datasheet figure and at the
                 6.3 TB/s a float4 copy reaches

Method: device events around windows of back-to-back calls, every window at least --window seconds long (the repetition count is
found first), 3 warm-up calls each, the two routes alternating over --windows windows; reported are the median microseconds per call
and the spread over the windows.

    python tools/bench_rollout_diag.py [--batch 8] [--frames 1460] [--window 0.3] [--windows 5] [--out profiles/rollout_diag.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF_SPEC_TBS, ROOF_COPY_TBS = 8.0, 6.3


def window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def compare(ours, base, window, windows):
    """alternating windows -> (median us ours, [min, max], median us baseline, [min, max])"""
    reps = []
    for fn in (ours, base):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps.append(max(3, int(window * 1e6 / max(window_us(fn, 3), 1e-3))))
    t = ([], [])
    for _ in range(windows):
        for k, fn in enumerate((ours, base)):
            t[k].append(window_us(fn, reps[k]))
    return [(statistics.median(x), [round(min(x), 1), round(max(x), 1)]) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1460)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rollout_diag: no GPU (timings on the CPU would say nothing)")
    from dlwp_benchmark_amd import evaluate, hpx_remap
    from dlwp_benchmark_amd import lib as L
    dev = torch.device("cuda:0")
    lib = L.load()
    B, T, V, H, W, n = args.batch, args.frames, 8, 32, 64, 8
    w0, w1 = evaluate.lead_window(334, 365, 6, T)
    gen = torch.Generator(device=dev).manual_seed(0)
    scale = torch.tensor([15.6, 21.2, 5.5, 4.8, 5087.0, 3349.0, 2133.0, 1070.0], device=dev)
    shift = torch.tensor([274.5, 278.4, -0.09, 0.22, 89400.0, 54108.0, 28925.0, 738.5], device=dev)
    sc5, sh5 = scale.view(1, 1, V, 1, 1), shift.view(1, 1, V, 1, 1)
    clim = shift.view(1, V, 1, 1) + scale.view(1, V, 1, 1) * 0.5 * torch.randn(12, V, H, W, device=dev, generator=gen)
    months_h = evaluate.forecast_months(np.datetime64("2017-01-01T00", "h") + np.timedelta64(84, "h") * np.arange(B), T, 6)
    months = torch.from_numpy(months_h).to(dev)
    months_l = months.long()
    rm = hpx_remap.HEALPixRemap(latitudes=H, longitudes=W, nside=n, device=dev)
    roww = evaluate.lat_weights(rm.lats_deg, dev).contiguous()
    lines = []
    for mesh in ("latlon", "hpx8"):
        plane = (H, W) if mesh == "latlon" else (12, n, n)
        npix = int(np.prod(plane))
        o = torch.randn((B, T, V) + plane, device=dev, generator=gen)
        t = torch.randn((B, T, V) + plane, device=dev, generator=gen)
        moments, zonal = torch.zeros(B, T, V, 5, device=dev), torch.zeros(2, B, T, V, H, device=dev)
        wsum = torch.zeros(2, B, V, H, W, device=dev)
        ws = torch.empty(lib.dlwp_rollout_diag_ws_floats(B, T, V, H, W, int(mesh != "latlon")), device=dev)
        idx, w = (rm._hpx2ll.idx, rm._hpx2ll.w) if mesh != "latlon" else (None, None)

        def fused():
            L.check(lib.dlwp_rollout_diag(L.ptr(o), T * V * npix, V * npix, L.ptr(t), L.ptr(scale), L.ptr(shift), L.ptr(roww), L.ptr(clim),
                                          L.ptr(months), 12, L.ptr(idx), L.ptr(w), n if idx is not None else 0, B, T, V, H, W, 0, T, w0, w1,
                                          L.ptr(moments), L.ptr(zonal), L.ptr(wsum), L.ptr(ws), L.stream()))

        def composition():
            ol, tl = (o, t) if mesh == "latlon" else (rm.hpx2ll(o), rm.hpx2ll(t))
            op, tp = ol * sc5 + sh5, tl * sc5 + sh5
            c = clim[months_l]
            m = evaluate.error_moments(op.reshape(B, T * V, H, W), tp.reshape(B, T * V, H, W), c.reshape(B, T * V, H, W), roww)
            z = torch.stack([op.mean(-1), tp.mean(-1)])
            wm = torch.stack([op[:, w0:w1].mean(1), tp[:, w0:w1].mean(1)])
            return m, z, wm

        with L.kernel_accounting() as acc:
            fused()
            torch.cuda.synchronize()
        kernels = {r["name"]: {"ms": round(r["ms"], 4), "algorithmic_bytes": r["bytes"]} for r in acc.rows}
        # the two routes agree (the composition sums in physical units: compare loosely, this is a benchmark's sanity check)
        with torch.no_grad():
            m_ref, z_ref, wm_ref = composition()
            wsum.zero_()
            fused()
            torch.cuda.synchronize()
            rel = lambda a, b: float((a - b).abs().max() / b.abs().max())      # noqa: E731
            agree = {"moments": rel(moments.sum(0).permute(2, 0, 1).reshape(5, T * V), m_ref), "zonal": rel(zonal, z_ref),
                     "window_mean": rel(wsum / (w1 - w0) * sc5[0].unsqueeze(0) + sh5[0].unsqueeze(0), wm_ref)}
            del m_ref, z_ref, wm_ref
            (us, spread), (bus, bspread) = compare(fused, composition, args.window, args.windows)
        nbytes = 4.0 * B * T * V * npix * 2
        line = {"mesh": mesh, "shape": f"B {B}, T {T}, V {V}, {H}x{W}" + (f", HPX{n}" if mesh != "latlon" else ""), "window": [w0, w1],
                "fused_us": round(us, 1), "fused_us_min_max": spread, "composition_us": round(bus, 1), "composition_us_min_max": bspread,
                "composition_over_fused": round(bus / us, 2), "algorithmic_bytes": nbytes,
                "roof_us_at_8TBs": round(nbytes / ROOF_SPEC_TBS / 1e6, 1), "roof_us_at_6.3TBs": round(nbytes / ROOF_COPY_TBS / 1e6, 1),
                "fraction_of_8TBs": round(nbytes / us / 1e6 / ROOF_SPEC_TBS, 4), "fraction_of_6.3TBs": round(nbytes / us / 1e6 / ROOF_COPY_TBS, 4),
                "kernels_one_call": kernels, "max_rel_difference_to_composition": agree}
        lines.append(line)
        print(json.dumps(line), flush=True)
        del o, t, moments, zonal, wsum, ws
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
