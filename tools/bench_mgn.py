#!/usr/bin/env python3
"""Training-step time of the two MeshGraphNet baselines, fp32, Adam:

* nsbench, the published command (src/nsbench/scripts/train_commands.txt): `grid_2d`, hidden 32, processor_size 2, 64 x 64,
  B 1, sequence 50, context_size 10, teacher forcing 10;
* dlwpbench `d116`: `delaunay` on 32 x 64, hidden 116, processor_size 4, context_size 1, 4 constant / 1 prescribed /
  8 prognostic channels, B 1, two lead times.

Per workload one JSON line: the graphed step (train_engine.GraphedTrainStep, 3 warm-up steps, median of >= 10, each step
bracketed by a device synchronisation), samples/s, the per-kernel accounting of ONE eager step (lib.kernel_accounting: name,
calls, ms, TFLOP/s, fraction of the 157.3 TFLOP/s fp32 matrix roof and of 8 TB/s, share of the kernel time), the same step of the
plain-torch helper model (tests/mgn_ref.py: index_select / index_add_ / F.linear / F.layer_norm) on the same card ("what a user
gets without this library"; a failure there is reported in the line, nothing is retried) and on the host CPU with 16 threads.

    python tools/bench_mgn.py [--only nsbench|dlwpbench] [--steps 10] [--out profiles/mgn_step.json] [--append]
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


def workloads():
    import mgn_ref as R
    ns = R._ns("grid_2d", 64, 64, True, 10, 2, R._widths(32))
    dl = R._dlwp("delaunay", 32, 64, True, 4, 1, 8, 1, 4, R._widths(116))
    return {"nsbench": ("ns", ns, (1, 50, 64, 64), dict(teacher_forcing_steps=10)),
            "dlwpbench": ("dlwp", dl, (1, 3, 32, 64), {})}


def helper_step_seconds(kind, cfg, roll, params, inputs, target, device, reps):
    """forward + backward + Adam of the helper model; median seconds per step"""
    import mgn_ref as R
    p = {k: v.detach().clone().to(device).requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)
    mesh = tuple(t.to(device) for t in R.build_mesh(kind, cfg))
    inp = {k: v.to(device) for k, v in inputs.items()}
    y = target.to(device)
    net = lambda x_t: R.network(p, x_t, mesh, cfg.get("message_passing_steps", 1), cfg.get("aggregation", "sum"))      # noqa: E731
    times = []
    for i in range(reps + 1):
        if device.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        if kind == "ns":
            out = R.ns_forward(p, inp["x"], roll["teacher_forcing_steps"], cfg["context_size"], net)
        else:
            out = R.dlwp_forward(p, inp.get("constants"), inp.get("prescribed"), inp["prognostic"], cfg["context_size"], net)
        torch.nn.functional.mse_loss(out, y).backward()
        opt.step()
        if device.type == "cuda":
            torch.cuda.synchronize()
        if i:                                   # the first step warms allocators and kernel caches
            times.append(time.perf_counter() - t0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="nsbench,dlwpbench")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mgn_step.json"))
    ap.add_argument("--append", action="store_true", help="keep the lines already in --out (one workload per invocation)")
    a = ap.parse_args()
    import mgn_ref as R
    from dlwp_benchmark_amd import dlwpbench, lib as L, nsbench
    from dlwp_benchmark_amd.train_engine import GraphedTrainStep
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    lines = []
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            lines = json.load(f)
    for app in a.only.split(","):
        kind, cfg, shape, roll = workloads()[app]
        B = shape[0]
        torch.manual_seed(0)
        inputs, target = R.make_inputs(kind, cfg, shape, torch.Generator().manual_seed(1))
        model = (nsbench if kind == "ns" else dlwpbench).MeshGraphNet(device=dev, **cfg).train()
        params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        line = {"model": f"{app}.MeshGraphNet", "config": {k: v for k, v in cfg.items()}, "parameters": sum(v.numel() for v in params.values()),
                "batch": B, "frames": shape[1], "grid": list(shape[2:]), "nodes": model.graph.num_nodes, "edges": model.graph.num_edges,
                "rollout": roll, "precision": "fp32"}
        ind = {k: v.to(dev) for k, v in inputs.items()}
        yd = target.to(dev)
        if kind == "ns":
            call = lambda m, kw: m(kw["x"], roll["teacher_forcing_steps"])      # noqa: E731
        else:
            call = lambda m, kw: m(constants=kw.get("constants"), prescribed=kw.get("prescribed"), prognostic=kw["prognostic"])      # noqa: E731
        # ---- one eager step under the accounting
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            with L.kernel_accounting() as acc:
                torch.nn.functional.mse_loss(call(model, ind), yd).backward()
                torch.cuda.synchronize()
        total_ms = sum(r["ms"] for r in acc.rows)
        line["eager_step_kernels"] = [
            {"name": r["name"], "calls": r["calls"], "ms": round(r["ms"], 3), "tflops": round(r["flops"] / (r["ms"] * 1e9), 3) if r["ms"] else 0.0,
             "fraction_of_fp32_matrix_roof": round(r["flops"] / (r["ms"] * 1e9) / ROOF_TFLOPS, 4) if r["ms"] else 0.0,
             "fraction_of_8TBs": round(r["bytes"] / (r["ms"] * 1e9) / ROOF_TBS, 4) if r["ms"] else 0.0,
             "share_of_kernel_time": round(r["ms"] / total_ms, 4)} for r in acc.rows]
        line["eager_step_kernel_ms"] = round(total_ms, 3)
        line["eager_step_launches"] = sum(r["calls"] for r in acc.rows)
        model.zero_grad(set_to_none=True)
        # ---- the graphed step
        step = GraphedTrainStep(model, ind, yd, lr=1e-3, call=call)
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
        line.update({"step_ms": round(ms, 3), "step_ms_min": round(min(times) * 1e3, 3), "step_ms_max": round(max(times) * 1e3, 3),
                     "samples_per_s": round(B / ms * 1e3, 2), "steps_timed": len(times), "loss": float(step.loss.item())})
        del step
        line["torch_gpu_helper"] = "not reached"
        lines.append(line)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
        try:
            gpu_s = helper_step_seconds(kind, cfg, roll, params, inputs, target, dev, 3)
            del line["torch_gpu_helper"]
            line.update({"torch_gpu_helper_step_ms": round(gpu_s * 1e3, 2), "torch_gpu_helper_samples_per_s": round(B / gpu_s, 2),
                         "speedup_over_torch_gpu_helper": round(gpu_s * 1e3 / ms, 2)})
        except Exception as e:      # noqa: BLE001 -- reported, not retried
            line["torch_gpu_helper"] = f"did not run: {type(e).__name__}: {str(e)[:200]}"
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
        cpu_s = helper_step_seconds(kind, cfg, roll, params, inputs, target, torch.device("cpu"), a.cpu_reps)
        line.update({"cpu_helper_step_ms": round(cpu_s * 1e3, 1), "cpu_helper_samples_per_s": round(B / cpu_s, 3), "cpu_threads": 16,
                     "speedup_over_cpu_helper": round(cpu_s * 1e3 / ms, 1)})
        print(json.dumps(line), flush=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
