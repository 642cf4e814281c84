#!/usr/bin/env python3
"""Training-step time of the nsbench ConvLSTM at the published protocol: B 4, 64 x 64, sequence 50, teacher forcing 10, fp32,
Adam; widths 2 x 16 (the shipped config), 4 x 57 ("1M") and 4 x 162 ("4M") of src/nsbench/scripts/train_commands.txt.

Per width one JSON line: the graphed step (train_engine.GraphedTrainStep, 3 warm-up steps, median of >= 10), samples/s, the
per-kernel accounting of ONE eager step (lib.kernel_accounting: name, calls, ms, TFLOP/s, fraction of the 157.3 TFLOP/s fp32
matrix roof and of 8 TB/s), the same step of the plain-torch helper model (tests/convlstm_ref.py) on the host CPU with 16
threads, and -- where torch's own convolution runs on the card -- the helper on the GPU ("what a user gets without this
library"; a failure there is reported in the line, nothing is retried).

    python tools/bench_convlstm.py [--widths 2x16,4x57,4x162] [--steps 10] [--out profiles/convlstm_step.json] [--append]

`--mesh healpix` times `dlwpbench.ConvLSTMHPX` instead, and `--mesh equirectangular` `dlwpbench.ConvLSTM` beside it, at the
reference's training protocol (src/dlwpbench/configs/training/default.yaml: batch 16, sequence 5; model/convlstm.yaml: 4
constant, 1 prescribed, 8 prognostic channels, context 1): widths 2 x 16 (the shipped config) and 4 x 228 (the published
"16M"), face sizes 8 and 32 with 16 spheres per batch, the equirectangular grid 32 x 64 with 16 samples.  One JSON line per
width and grid with the graphed step and the per-kernel accounting of one eager step; the helper models are not timed here.

    python tools/bench_convlstm.py --mesh healpix [--widths 2x16,4x228] [--faces 8,32] --out profiles/convlstm_hpx_step.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROOF_TFLOPS, ROOF_TBS = 157.3, 8.0
B, H, W, SEQ, TF = 4, 64, 64, 50, 10


def helper_step_seconds(params, x, y, device, reps):
    """forward + backward + Adam of the helper model; median seconds per step"""
    import convlstm_ref as R
    p = {k: v.detach().clone().to(device).requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)
    x, y = x.to(device), y.to(device)
    times = []
    for i in range(reps + 1):
        if device.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(R.ns_forward(p, x, TF), y)
        loss.backward()
        opt.step()
        if device.type == "cuda":
            torch.cuda.synchronize()
        if i:                                   # the first step warms allocators and kernel caches
            times.append(time.perf_counter() - t0)
    return statistics.median(times)


DLWP_B, DLWP_SEQ, DLWP_CH = 16, 5, dict(constant_channels=4, prescribed_channels=1, prognostic_channels=8, context_size=1)


def accounting_rows(acc):
    total_ms = sum(r["ms"] for r in acc.rows)
    rows = [{"name": r["name"], "calls": r["calls"], "ms": round(r["ms"], 3), "tflops": round(r["flops"] / (r["ms"] * 1e9), 2) if r["ms"] else 0.0,
             "fraction_of_fp32_matrix_roof": round(r["flops"] / (r["ms"] * 1e9) / ROOF_TFLOPS, 4) if r["ms"] else 0.0,
             "fraction_of_8TBs": round(r["bytes"] / (r["ms"] * 1e9) / ROOF_TBS, 4) if r["ms"] else 0.0,
             "share_of_kernel_time": round(r["ms"] / total_ms, 4)} for r in acc.rows]
    return rows, total_ms


def timed_steps(step, warmup, steps):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(max(steps, 10)):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times) * 1e3, len(times)


def dlwp_lines(a, dev, lines):
    """the dlwpbench ConvLSTM on either mesh: one line per width and grid"""
    from dlwp_benchmark_amd import dlwpbench, lib as L
    from dlwp_benchmark_amd.train_engine import GraphedTrainStep
    hpx = a.mesh == "healpix"
    grids = [(12, int(f), int(f)) for f in a.faces.split(",")] if hpx else [(32, 64)]
    for spec in (a.widths or "2x16,4x228").split(","):
        n, h = (int(v) for v in spec.split("x"))
        for grid in grids:
            torch.manual_seed(0)
            g = torch.Generator().manual_seed(1)
            r = lambda t, c: torch.randn(DLWP_B, t, c, *grid, generator=g).to(dev)      # noqa: E731
            kw = {"constants": r(1, DLWP_CH["constant_channels"]), "prescribed": r(DLWP_SEQ, DLWP_CH["prescribed_channels"]),
                  "prognostic": r(DLWP_SEQ, DLWP_CH["prognostic_channels"])}
            yd = r(DLWP_SEQ - DLWP_CH["context_size"], DLWP_CH["prognostic_channels"])
            cls = dlwpbench.ConvLSTMHPX if hpx else dlwpbench.ConvLSTM
            model = cls(batch_size=DLWP_B, hidden_sizes=[h] * n, height=grid[-2], width=grid[-1], device=dev, **DLWP_CH).train()
            line = {"model": f"dlwpbench.{cls.__name__} {n} x {h}", "mesh": a.mesh, "parameters": sum(p.numel() for p in model.parameters()),
                    "batch": DLWP_B, "grid": list(grid), "pixels_per_sample": int(torch.tensor(grid).prod()), "sequence": DLWP_SEQ,
                    "context_size": DLWP_CH["context_size"], "precision": "fp32"}
            for _ in range(2):
                model.zero_grad(set_to_none=True)
                with L.kernel_accounting() as acc:
                    torch.nn.functional.mse_loss(model(**kw), yd).backward()
                    torch.cuda.synchronize()
            line["eager_step_kernels"], total_ms = accounting_rows(acc)
            line["eager_step_kernel_ms"] = round(total_ms, 3)
            model.zero_grad(set_to_none=True)
            step = GraphedTrainStep(model, kw, yd, lr=1e-3)
            ms, ntimed = timed_steps(step, a.warmup, a.steps)
            line.update({"step_ms": round(ms, 3), "samples_per_s": round(DLWP_B / ms * 1e3, 2), "steps_timed": ntimed,
                         "us_per_pixel_frame": round(ms * 1e3 / (DLWP_B * line["pixels_per_sample"] * DLWP_SEQ), 5),
                         "loss": float(step.loss.item())})
            del step, model
            lines.append(line)
            print(json.dumps(line), flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(lines, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="ns", choices=["ns", "healpix", "equirectangular"],
                    help="ns: the nsbench model (default); healpix / equirectangular: dlwpbench.ConvLSTMHPX / dlwpbench.ConvLSTM")
    ap.add_argument("--faces", default="8,32", help="--mesh healpix: face sizes")
    ap.add_argument("--widths", default=None, help="LAYERSxWIDTH,...; default 2x16,4x57,4x162 (ns) or 2x16,4x228 (dlwpbench)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convlstm_step.json"))
    ap.add_argument("--append", action="store_true", help="keep the lines already in --out (one width per invocation)")
    a = ap.parse_args()
    from dlwp_benchmark_amd import lib as L, nsbench
    from dlwp_benchmark_amd.train_engine import GraphedTrainStep
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    lines = []
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            lines = json.load(f)
    if a.mesh != "ns":
        return dlwp_lines(a, dev, lines)
    for spec in (a.widths or "2x16,4x57,4x162").split(","):
        n, h = (int(v) for v in spec.split("x"))
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(1)
        u = torch.randn(B, SEQ + 1, 1, H, W, generator=g)
        x, y = u[:, :-1].contiguous(), u[:, 1:].contiguous()
        model = nsbench.ConvLSTM(batch_size=B, input_size=1, hidden_sizes=[h] * n, height=H, width=W, device=dev).train()
        params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        line = {"model": f"nsbench.ConvLSTM {n} x {h}", "parameters": sum(v.numel() for v in params.values()), "batch": B,
                "grid": [H, W], "sequence": SEQ, "teacher_forcing_steps": TF, "precision": "fp32"}
        # ---- one eager step under the accounting
        xd, yd = x.to(dev), y.to(dev)
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            with L.kernel_accounting() as acc:
                torch.nn.functional.mse_loss(model(xd, TF), yd).backward()
                torch.cuda.synchronize()
        line["eager_step_kernels"], total_ms = accounting_rows(acc)
        line["eager_step_kernel_ms"] = round(total_ms, 3)
        model.zero_grad(set_to_none=True)
        # ---- the graphed step
        step = GraphedTrainStep(model, {"x": xd}, yd, lr=1e-3, call=lambda m, kw: m(kw["x"], TF))
        ms, ntimed = timed_steps(step, a.warmup, a.steps)
        line.update({"step_ms": round(ms, 3), "samples_per_s": round(B / ms * 1e3, 2), "steps_timed": ntimed,
                     "loss": float(step.loss.item())})
        del step
        # ---- the helper on the host CPU (16 threads) and, if torch's convolution runs there, on the card
        cpu_s = helper_step_seconds(params, x, y, torch.device("cpu"), a.cpu_reps)
        line.update({"cpu_helper_step_ms": round(cpu_s * 1e3, 1), "cpu_helper_samples_per_s": round(B / cpu_s, 3), "cpu_threads": 16,
                     "speedup_over_cpu_helper": round(cpu_s * 1e3 / ms, 1)})
        line["torch_gpu_helper"] = "not reached"
        lines.append(line)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:                    # kept even if torch's own convolution stalls below
            json.dump(lines, f, indent=1)
        try:
            gpu_s = helper_step_seconds(params, x, y, dev, 3)
            del line["torch_gpu_helper"]
            line.update({"torch_gpu_helper_step_ms": round(gpu_s * 1e3, 2), "torch_gpu_helper_samples_per_s": round(B / gpu_s, 2)})
        except Exception as e:      # noqa: BLE001 -- reported, not retried
            line["torch_gpu_helper"] = f"did not run: {type(e).__name__}: {str(e)[:200]}"
        print(json.dumps(line), flush=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
