#!/usr/bin/env python3
"""Time of the ensemble score kernel (csrc/ensemble.hip: dlwp_ens_diag) beside a torch composition of the same sums and beside the
HBM roof of its algorithmic bytes, in one run.

Shapes: the dlwpbench grid 32 x 64 with V = 8 (B --batch, T --frames) and Navier-Stokes planes of 64 x 64 with D = 1 (B 16, T 50),
each for M = 4, 16 and 64 members.  Per case one JSON line:

    kernel       ensemble.ensemble_diagnostics (tables pre-allocated in the state): dlwp_ens_diag and its fold launch
    composition  torch on the same device: mean / var over the member axis, mean |x_i - y|, the pair term from torch.sort and the
                 order-statistics weights (the cheapest torch form: no [M, M, ...] tensor), the ranks from (x < y).sum and
                 torch.bincount
    roof         one read of the M member fields and the target at the 8 TB/s datasheet figure and at the 6.3 TB/s a float4 copy
                 reaches

Method: device events around windows of back-to-back calls, every window at least --window seconds long (the repetition count is
found first), 3 warm-up calls each, the two routes alternating over --windows windows; median microseconds and [min, max].

    python tools/bench_ensemble.py [--batch 4] [--frames 8] [--window 0.3] [--windows 5] [--out profiles/ensemble.json]
"""
import argparse
import json
import os
import statistics
import sys

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
    """alternating windows -> (median us ours, [min, max]), (median us baseline, [min, max])"""
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
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ensemble: no GPU (timings on the CPU would say nothing)")
    from dlwp_benchmark_amd import ensemble as E, evaluate
    from dlwp_benchmark_amd import lib as L
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for case, (B, T, V, H, W), weighted in (("dlwpbench", (args.batch, args.frames, 8, 32, 64), True), ("nsbench", (16, 50, 1, 64, 64), False)):
        lats = evaluate.regular_latitudes(H) if weighted else None
        w = evaluate.lat_weights(lats, dev).reshape(H, 1) if weighted else torch.ones(H, 1, device=dev)
        for M in (4, 16, 64):
            x = torch.randn(B, M, T, V, H, W, device=dev, generator=gen)
            y = torch.randn(B, T, V, H, W, device=dev, generator=gen)
            nf = B * T * V
            coef = (2.0 * torch.arange(M, device=dev) - M + 1).reshape(1, M, 1, 1, 1, 1)
            field = (torch.arange(nf, device=dev) * (M + 1)).reshape(B, T, V, 1, 1)
            state = {"st": None}

            def kernel():
                st = E.ensemble_diagnostics(x, y, lats_deg=lats, state=state["st"])
                st["frames"] = 0
                state["st"] = st
                return st

            def composition():
                d = x.mean(1) - y
                s0 = (w * d * d).sum((-1, -2))
                s1 = (w * x.var(1, unbiased=True)).sum((-1, -2))
                s2 = (w * (x - y[:, None]).abs().mean(1)).sum((-1, -2))
                s3 = (w * (torch.sort(x, dim=1).values * coef).sum(1)).sum((-1, -2)) / (M * (M - 1))
                below = (x < y[:, None]).sum(1)
                ranks = torch.bincount((field + below).reshape(-1), minlength=nf * (M + 1)).reshape(B, T, V, M + 1)
                return torch.stack([s0, s1, s2, s3], -1), ranks

            with L.kernel_accounting() as acc:
                st = kernel()
                torch.cuda.synchronize()
            kern = {r["name"]: {"calls": r["calls"], "ms": round(r["ms"], 4)} for r in acc.rows}
            with torch.no_grad():
                sums, ranks = composition()
                agree = {"sums": float(((st["sums"] - sums).abs() / sums.abs()).max()), "ranks_equal": bool(torch.equal(st["ranks"].long(), ranks))}
                del sums, ranks
                (us, spread), (bus, bspread) = compare(kernel, composition, args.window, args.windows)
            nbytes = 4.0 * nf * H * W * (M + 1)
            line = {"case": case, "shape": f"B {B}, M {M}, T {T}, V {V}, {H}x{W}", "kernel_us": round(us, 1), "kernel_us_min_max": spread,
                    "composition_us": round(bus, 1), "composition_us_min_max": bspread, "composition_over_kernel": round(bus / us, 2),
                    "algorithmic_bytes": nbytes, "roof_us_at_8TBs": round(nbytes / ROOF_SPEC_TBS / 1e6, 1),
                    "roof_us_at_6.3TBs": round(nbytes / ROOF_COPY_TBS / 1e6, 1), "fraction_of_8TBs": round(nbytes / us / 1e6 / ROOF_SPEC_TBS, 4),
                    "fraction_of_6.3TBs": round(nbytes / us / 1e6 / ROOF_COPY_TBS, 4), "kernels_one_pass": kern,
                    "difference_to_composition": agree}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del x, y, state
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
