#!/usr/bin/env python3
"""Time steps per second of the two GPU Navier-Stokes solvers of nsdata.py in one process: navier_stokes_2d_hip (the transforms on
the library's FFT kernels, the point-wise algebra in torch) and navier_stokes_2d_device (the point-wise algebra on the kernels of
csrc/ns_solver.hip as well), at (n, B) = (64, 50) and (256, 50).

Method: a solver is one call that sets up (buffers, the two initial transforms), steps and records one frame, so the steps are timed
by difference.  Per repeat and per solver: a call of --warmup steps, then a call of --warmup + --steps steps, each under a host
clock that ends in a synchronise; steps/s = --steps / (long - short).  The set-up, the warm-up steps and the recorded frame are in
both calls and cancel: what remains is --steps steps that follow --warmup warm-up steps.  The whole-call rate of the long call
(set-up included) is reported beside it.  The two solvers alternate over --repeats repeats; reported are the medians and the
ranges.  Launches per step: kernels seen by torch.profiler in a call of 3 steps minus those of a call of 1 step, halved (every kernel, torch's
included), and the library's own launches from its accounting (lib.kernel_accounting) counted the same way.  One JSON line per
shape; the two solvers' last frames are compared as a sanity check.

    python tools/bench_nsdata.py [--steps 200] [--warmup 20] [--repeats 5] [--out profiles/nsdata.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, VISC = 1e-3, 1e-3
SHAPES = ((64, 50), (256, 50))


def run(solver, w0, f, steps):
    sol, _ = solver(w0, f, VISC, T=steps * DT - 0.5 * DT, delta_t=DT, record_steps=1)      # ceil(T / dt) = steps
    torch.cuda.synchronize()
    return sol


def timed(solver, w0, f, steps):
    t0 = time.perf_counter()
    run(solver, w0, f, steps)
    return time.perf_counter() - t0


def steps_per_s(solver, w0, f, steps, warmup):
    """(steps/s of `steps` steps behind `warmup` warm-up steps, steps/s of the whole long call)"""
    short, long = timed(solver, w0, f, warmup), timed(solver, w0, f, warmup + steps)
    return steps / (long - short), (warmup + steps) / long


def profiler_kernels(solver, w0, f, steps):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        run(solver, w0, f, steps)
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return sum(1 for k in names if not k.lower().startswith(("memcpy", "memset")))


def library_kernels(L, solver, w0, f, steps):
    with L.kernel_accounting() as acc:
        run(solver, w0, f, steps)
    return sum(r["calls"] for r in acc.rows)


def launches_per_step(count):
    """kernels a step adds to a call (the set-up and the recorded frame cancel)"""
    return (count(3) - count(1)) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_nsdata: no GPU (timings on the CPU would say nothing)")
    from dlwp_benchmark_amd import lib as L
    from dlwp_benchmark_amd import nsdata
    dev = torch.device("cuda:0")
    solvers = {"torch": nsdata.navier_stokes_2d_hip, "kernels": nsdata.navier_stokes_2d_device}
    lines = []
    for n, B in SHAPES:
        w0 = nsdata.GaussianRF(n, alpha=2.5, tau=7.0, device=dev, rng="philox", seed=1).sample(B)
        f = nsdata.forcing(n, device=dev)
        last = {k: run(s, w0, f, args.warmup) for k, s in solvers.items()}
        agree = float((last["kernels"] - last["torch"]).abs().max() / last["torch"].abs().max())
        rates, calls = {k: [] for k in solvers}, {k: [] for k in solvers}
        for _ in range(args.repeats):
            for k, s in solvers.items():
                per_step, per_call = steps_per_s(s, w0, f, args.steps, args.warmup)
                rates[k].append(per_step), calls[k].append(per_call)
        line = {"n": n, "B": B, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
        for k, s in solvers.items():
            line[k + "_steps_per_s"] = round(statistics.median(rates[k]), 1)
            line[k + "_steps_per_s_min_max"] = [round(min(rates[k]), 1), round(max(rates[k]), 1)]
            line[k + "_us_per_step"] = round(1e6 / statistics.median(rates[k]), 2)
            line[k + "_whole_call_steps_per_s"] = round(statistics.median(calls[k]), 1)
            line[k + "_library_launches_per_step"] = launches_per_step(lambda c, s=s: library_kernels(L, s, w0, f, c))
            try:
                seen = launches_per_step(lambda c, s=s: profiler_kernels(s, w0, f, c))
                line[k + "_launches_per_step"] = seen if seen > 0 else None      # no device events: not measured
            except Exception as e:      # a profiler without device tracing: the count is then not measured, the timings stand
                line[k + "_launches_per_step"] = None
                line["profiler_error"] = f"{type(e).__name__}: {e}"
        line["kernels_over_torch"] = round(line["kernels_steps_per_s"] / line["torch_steps_per_s"], 2)
        line["max_rel_difference_after_warmup_steps"] = agree
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
