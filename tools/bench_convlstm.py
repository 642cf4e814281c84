#!/usr/bin/env python3
"""Training-step time of the nsbench ConvLSTM at the published protocol: B 4, 64 x 64, sequence 50, teacher forcing 10, fp32,
Adam; widths 2 x 16 (the shipped config), 4 x 57 ("1M") and 4 x 162 ("4M") of src/nsbench/scripts/train_commands.txt.

Per width one JSON line: the graphed step (train_engine.GraphedTrainStep, 3 warm-up steps, median of >= 10), samples/s, the
per-kernel accounting of ONE eager step (lib.kernel_accounting: name, calls, ms, TFLOP/s, fraction of the 157.3 TFLOP/s fp32
matrix roof and of 8 TB/s), the same step of the plain-torch helper model (tests/convlstm_ref.py) on the host CPU with 16
threads, and -- where torch's own convolution runs on the card -- the helper on the GPU ("what a user gets without this
library"; a failure there is reported in the line, nothing is retried).

    python tools/bench_convlstm.py [--widths 2x16,4x57,4x162] [--steps 10] [--out profiles/convlstm_step.json] [--append]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="2x16,4x57,4x162")
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
    for spec in a.widths.split(","):
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
        total_ms = sum(r["ms"] for r in acc.rows)
        line["eager_step_kernels"] = [
            {"name": r["name"], "calls": r["calls"], "ms": round(r["ms"], 3), "tflops": round(r["flops"] / (r["ms"] * 1e9), 2) if r["ms"] else 0.0,
             "fraction_of_fp32_matrix_roof": round(r["flops"] / (r["ms"] * 1e9) / ROOF_TFLOPS, 4) if r["ms"] else 0.0,
             "fraction_of_8TBs": round(r["bytes"] / (r["ms"] * 1e9) / ROOF_TBS, 4) if r["ms"] else 0.0,
             "share_of_kernel_time": round(r["ms"] / total_ms, 4)} for r in acc.rows]
        line["eager_step_kernel_ms"] = round(total_ms, 3)
        model.zero_grad(set_to_none=True)
        # ---- the graphed step
        step = GraphedTrainStep(model, {"x": xd}, yd, lr=1e-3, call=lambda m, kw: m(kw["x"], TF))
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        times = []
        for _ in range(max(a.steps, 10)):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        ms = statistics.median(times) * 1e3
        line.update({"step_ms": round(ms, 3), "samples_per_s": round(B / ms * 1e3, 2), "steps_timed": len(times),
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
