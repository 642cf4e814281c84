#!/usr/bin/env python3
"""Time of the HEALPix <-> lat-lon remap kernels (csrc/hpx_remap.hip) beside the torch expression of the same tables, in one run.

Shapes: HPX8 <-> 32 x 64 with planes = 16 * 57 * 8 (the reference's evaluation: batch 16, 57 lead times, 8 variables;
scripts/evaluate.py projects that many maps one by one on the CPU), and HPX64 <-> 32 x 64 with a few planes (the direct path).
Per shape and operation one JSON line:

    hpx2ll / ll2hpx   dlwp_remap_gather4                     baseline (x[..., idx] * w).sum(-1)
    adjoint_*         dlwp_remap_csr                          baseline torch autograd's backward of that expression
    moments           dlwp_hpx_error_moments (fused)          baseline hpx2ll of outputs and targets + evaluate.error_moments

Method: device events around windows of back-to-back launches, every window at least --window seconds long (the repetition count
is found first), 3 warm-up launches per operation, the library and the baseline alternating over --windows windows; reported are the
median microseconds per launch, the spread over the windows, algorithmic GB/s (4 planes (n_in + n_out) bytes for the remaps, the two
HEALPix tensors and the climatology for the moments), the fraction of the 8 TB/s HBM roof and the ratio to the baseline.  The parent
commit has no kernel to compare with.

    python tools/bench_hpx_remap.py [--window 0.2] [--windows 5] [--out profiles/hpx_remap.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF_TBS = 8.0


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
    return [(statistics.median(x), [round(min(x), 2), round(max(x), 2)]) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hpx_remap: no GPU (timings on the CPU would say nothing)")
    from dlwp_benchmark_amd import evaluate, hpx_remap
    from dlwp_benchmark_amd import lib as L
    dev = torch.device("cuda:0")
    lines = []

    def report(shape, op, kernel, nbytes, res):
        (us, spread), (bus, bspread) = res
        line = {"shape": shape, "op": op, "kernel": kernel, "us": round(us, 2), "us_min_max": spread,
                "algorithmic_GBs": round(nbytes / us / 1e3, 1), "fraction_of_8TBs": round(nbytes / us / 1e6 / ROOF_TBS, 4),
                "baseline_us": round(bus, 2), "baseline_us_min_max": bspread, "baseline_over_ours": round(bus / us, 2)}
        lines.append(line)
        print(json.dumps(line), flush=True)

    for n, planes in ((8, 16 * 57 * 8), (64, 8)):
        H, W = 32, 64
        rm = hpx_remap.HEALPixRemap(latitudes=H, longitudes=W, nside=n, device=dev)
        npix, shape = 12 * n * n, f"HPX{n} <-> {H}x{W}, planes {planes}"
        x_h = torch.randn(planes, 12, n, n, device=dev)
        x_l = torch.randn(planes, H, W, device=dev)
        nbytes = 4.0 * planes * (npix + H * W)
        for op, x, tab, fn in (("hpx2ll", x_h, rm._hpx2ll, rm.hpx2ll), ("ll2hpx", x_l, rm._ll2hpx, rm.ll2hpx)):
            idx, w = tab.idx.long(), tab.w
            xf = x.reshape(planes, -1)
            with L.kernel_accounting() as acc:
                fn(x)
                torch.cuda.synchronize()
            kernel = "+".join(r["name"] for r in acc.rows)
            with torch.no_grad():
                report(shape, op, kernel, nbytes, compare(lambda: fn(x), lambda: (xf[:, idx] * w).sum(-1), args.window, args.windows))
            # the adjoint: R^T g
            g = torch.randn(planes, tab.n_out, device=dev)
            xr = xf.detach().clone().requires_grad_(True)
            y = (xr[:, idx] * w).sum(-1)
            report(shape, "adjoint_" + op, "remap_csr", nbytes,
                   compare(lambda: hpx_remap._adjoint(g, tab, (planes, tab.n_in)),
                           lambda: torch.autograd.grad(y, xr, g, retain_graph=True), args.window, args.windows))
            del y, xr, g
        if n == 8:
            B, G = 16, 57 * 8
            o, t = torch.randn(B, G, 12, n, n, device=dev), torch.randn(B, G, 12, n, n, device=dev)
            c = torch.randn(B, G, H, W, device=dev)
            wts = evaluate.lat_weights(rm.lats_deg, dev)
            with torch.no_grad():
                report(shape, "moments", "hpx_error_moments", 4.0 * B * G * (2 * npix + H * W),
                       compare(lambda: evaluate.hpx_error_moments(o, t, rm, c, wts),
                               lambda: evaluate.error_moments(rm.hpx2ll(o), rm.hpx2ll(t), c, wts), args.window, args.windows))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
