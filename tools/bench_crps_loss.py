#!/usr/bin/env python3
"""Time and peak memory of the fused CRPS loss (csrc/ensemble.hip: dlwp_crps_loss_fwd_bwd, loss + gradient in one call) beside the
torch composition of the same loss, in one run.

Shapes: the dlwpbench grid 32 x 64 with V 8, T 4, B 4 for M = 4 and 16 members, and one 721 x 1440 plane (V 1, T 1, B 1) for M = 8;
cos(lat) row weights in every case.  Per case one JSON line:

    fused        ensemble.crps_loss_and_grad: the loss kernel, its fold launch and the wrapper
    composition  torch on the same device, forward + backward through autograd: mean |x_i - y|, the pair term from the broadcast
                 [B, M, M, T, V, H, W] tensor of |x_i - x_j|, the weighted mean; gradient with respect to the members
    peak bytes   torch.cuda.max_memory_allocated over one call of each route, above what is allocated before it

Method: device events around windows of back-to-back calls, every window at least --window seconds long (the repetition count is
found first), 3 warm-up calls each, the two routes alternating over --windows windows; median microseconds and [min, max].  No
ratio is expected in advance: the comparison is between two routes on the same commit.

    python tools/bench_crps_loss.py [--window 0.3] [--windows 5] [--out profiles/crps_loss.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((4, 4, 4, 8, 32, 64), (4, 16, 4, 8, 32, 64), (1, 8, 1, 1, 721, 1440))      # B, M, T, V, H, W


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_crps_loss: no GPU (timings on the CPU would say nothing)")
    from dlwp_benchmark_amd import ensemble as E, evaluate
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for B, M, T, V, H, W in CASES:
        lats = evaluate.regular_latitudes(H)
        w = evaluate.lat_weights(lats, dev).reshape(H, 1)
        x = torch.randn(B, M, T, V, H, W, device=dev, generator=gen).requires_grad_(True)
        y = torch.randn(B, T, V, H, W, device=dev, generator=gen)

        def fused():
            return E.crps_loss_and_grad(x, y, lats_deg=lats)

        def composition():
            mae = (x - y[:, None]).abs().mean(1)
            pair = (x[:, :, None] - x[:, None, :]).abs().sum((1, 2)) / (2 * M * (M - 1))
            loss = (w * (mae - pair)).mean()
            (g,) = torch.autograd.grad(loss, x)
            return loss.detach(), g

        (lf, gf), (lc, gc) = fused(), composition()
        agree = {"loss": float((lf - lc).abs() / lc.abs()), "grad_max_abs": float((gf - gc).abs().max()), "grad_scale": float(gc.abs().max())}
        del lf, gf, lc, gc
        peaks = {"fused": peak_bytes(fused), "composition": peak_bytes(composition)}
        (us, spread), (bus, bspread) = compare(fused, composition, args.window, args.windows)
        line = {"shape": f"B {B}, M {M}, T {T}, V {V}, {H}x{W}", "fused_us": round(us, 1), "fused_us_min_max": spread,
                "composition_us": round(bus, 1), "composition_us_min_max": bspread, "composition_over_fused": round(bus / us, 2),
                "peak_bytes_fused": peaks["fused"], "peak_bytes_composition": peaks["composition"],
                "algorithmic_bytes": 4.0 * B * T * V * H * W * (2 * M + 1), "difference_to_composition": agree}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del x, y
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
