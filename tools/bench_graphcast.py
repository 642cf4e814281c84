#!/usr/bin/env python3
"""Training-step time of the nsbench GraphCast baseline, fp32, Adam: the published `dp34` command
(src/nsbench/scripts/train_commands.txt: hidden_dim_processor 34, encoders and decoder 32, processor_layers 4, two hidden layers
per MLP, nhop [2], 64 x 64, B 1, sequence 50, context_size 10, teacher forcing 10).

One JSON line: the graphed step (train_engine.GraphedTrainStep, 3 warm-up steps, median of >= 10, each step bracketed by a device
synchronisation), samples/s, the per-kernel accounting of ONE eager step (lib.kernel_accounting), the same step of the
plain-torch helper model (tests/graphcast_ref.py) on the same card ("what a user gets without this library"; a failure there is
reported in the line, nothing is retried), and -- in the same run -- the fused backward launch of a later Linear,
`dlwp_graph_dgrad_mul`, against what it replaces, `dlwp_conv1x1_dgrad` followed by a torch multiply, on 20480 x 34 and
20480 x 116 (the edge rows of this mesh at the published widths 34 and 116): 5 x 200 back-to-back launches between two events
after 20 warm-up launches, median microseconds per launch; the operands (<= 10 MB each) stay in the 256 MB last-level cache, as
they do inside a step.

    python tools/bench_graphcast.py [--steps 10] [--out profiles/graphcast_step.json]

`--model dlwp`: the dlwpbench GraphCastNet instead, at its shipped config (tests/golden/shipped_graphcast_dlwp_model_config.json:
hidden_dim 512, 16 processor layers, 32 x 64 grid) on a level-3 icosphere file this tool writes itself (the reference ships none),
B 1, 3 frames (context 1: two lead times).  Same line -- graphed step, accounting of one eager step, the plain-torch helper
(tests/graphcast_dlwp_ref.py, fp32) on the same card -- without the dgrad_mul comparison; default output
profiles/graphcast_dlwp_step.json.
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


def workload():
    import graphcast_ref as R
    return R._cfg(64, 64, [2], 10, 4, 34, 32, 32, 32), (1, 50), dict(teacher_forcing_steps=10)


def helper_step_seconds(cfg, roll, params, x, target, device, reps):
    """forward + backward + Adam of the helper model; median seconds per step"""
    import graphcast_ref as R
    p = {k: v.detach().clone().to(device).requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)
    mesh = tuple(t.to(device) for t in R.build_mesh(cfg))
    xd, y = x.to(device), target.to(device)
    net = lambda x_t: R.network(p, x_t, mesh, cfg.get("aggregation", "sum"), R.ACTS[cfg.get("activation_fn", "silu")])      # noqa: E731
    times = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        out = R.ns_forward(p, xd, roll["teacher_forcing_steps"], cfg["context_size"], net)
        torch.nn.functional.mse_loss(out, y).backward()
        opt.step()
        torch.cuda.synchronize()
        if i:                                   # the first step warms allocators and kernel caches
            times.append(time.perf_counter() - t0)
    return statistics.median(times)


def launch_us(fn, warmup=20, reps=5, inner=200):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(out)


def dgrad_mul_against_the_pair(dev, rows, width):
    from dlwp_benchmark_amd import lib as L
    lib, s = L.load(), L.stream()
    g = torch.Generator().manual_seed(width)
    dz, w, mul = (torch.randn(*sh, generator=g).to(dev) for sh in ((rows, width), (width, width), (rows, width)))
    out, dh = torch.empty(rows, width, device=dev), torch.empty(rows, width, device=dev)

    def fused():
        L.check(lib.dlwp_graph_dgrad_mul(L.ptr(dz), L.ptr(w), L.ptr(mul), L.ptr(out), rows, width, width, s))

    def pair():
        L.check(lib.dlwp_conv1x1_dgrad(L.ptr(dz), L.ptr(w), L.ptr(dh), rows, width, width, s))
        torch.mul(dh, mul, out=out)

    def dgrad_alone():
        L.check(lib.dlwp_conv1x1_dgrad(L.ptr(dz), L.ptr(w), L.ptr(dh), rows, width, width, s))

    f, p, d = launch_us(fused), launch_us(pair), launch_us(dgrad_alone)
    return {"rows": rows, "width": width, "graph_dgrad_mul_us": round(f, 2), "conv1x1_dgrad_plus_torch_mul_us": round(p, 2),
            "conv1x1_dgrad_alone_us": round(d, 2), "pair_over_fused": round(p / f, 3)}


def accounting_rows(acc):
    total_ms = sum(r["ms"] for r in acc.rows)
    return total_ms, [
        {"name": r["name"], "calls": r["calls"], "ms": round(r["ms"], 3), "tflops": round(r["flops"] / (r["ms"] * 1e9), 3) if r["ms"] else 0.0,
         "fraction_of_fp32_matrix_roof": round(r["flops"] / (r["ms"] * 1e9) / ROOF_TFLOPS, 4) if r["ms"] else 0.0,
         "fraction_of_8TBs": round(r["bytes"] / (r["ms"] * 1e9) / ROOF_TBS, 4) if r["ms"] else 0.0,
         "share_of_kernel_time": round(r["ms"] / total_ms, 4)} for r in acc.rows]


def main_dlwp(a):
    """the dlwpbench GraphCastNet at its shipped config"""
    import tempfile

    import graphcast_dlwp_ref as R
    from dlwp_benchmark_amd import dlwpbench, gc_mesh, lib as L
    from dlwp_benchmark_amd.train_engine import GraphedTrainStep
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "shipped_graphcast_dlwp_model_config.json")) as f:
        entry = json.load(f)["dlwpbench/graphcast"]
    cfg, frames = dict(entry["kwargs"]), 3
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, f"icospheres_l{entry['icosphere_level']}.json")
        gc_mesh.write_icospheres(path, entry["icosphere_level"])
        torch.manual_seed(0)
        model = dlwpbench.GraphCastNet(device=dev, **dict(cfg, meshgraph_path=path)).train()
        graphs = gc_mesh.build_graphs(*gc_mesh.load_icospheres(path), cfg["input_height"], cfg["input_width"])
    inputs, target = R.make_inputs(cfg, frames, torch.Generator().manual_seed(1))
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    line = {"model": "dlwpbench.GraphCastNet", "config": cfg, "parameters": sum(v.numel() for v in params.values()), "batch": 1,
            "frames": frames, "grid": [model.height, model.width], "precision": "fp32",
            "graphs": {k: {"sources": g.num_src, "destinations": g.num_dst, "edges": g.num_edges} for k, g in model.graphs.items()}}
    ind, yd = {k: v.to(dev) for k, v in inputs.items()}, target.to(dev)
    call = lambda m, kw: m(kw["constants"], kw["prescribed"], kw["prognostic"])      # noqa: E731

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump([line], f, indent=1)

    for _ in range(2):
        model.zero_grad(set_to_none=True)
        with L.kernel_accounting() as acc:
            torch.nn.functional.mse_loss(call(model, ind), yd).backward()
            torch.cuda.synchronize()
    total_ms, line["eager_step_kernels"] = accounting_rows(acc)
    line["eager_step_kernel_ms"] = round(total_ms, 3)
    line["eager_step_launches"] = sum(r["calls"] for r in acc.rows)
    model.zero_grad(set_to_none=True)
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
                 "samples_per_s": round(1 / ms * 1e3, 2), "steps_timed": len(times), "loss": float(step.loss.item())})
    del step
    line["torch_gpu_helper"] = "not reached"
    save()
    try:      # the helper's step: forward + backward + Adam in plain torch on the same card, fp32
        p = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in params.items()}
        opt = torch.optim.Adam(list(p.values()), lr=1e-3)
        net = R.RefGraphCast(graphs, p, cfg)
        htimes = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.mse_loss(net(ind["constants"], ind["prescribed"], ind["prognostic"]), yd).backward()
            opt.step()
            torch.cuda.synchronize()
            if i:
                htimes.append(time.perf_counter() - t0)
        gpu_s = statistics.median(htimes)
        del line["torch_gpu_helper"]
        line.update({"torch_gpu_helper_step_ms": round(gpu_s * 1e3, 2), "torch_gpu_helper_samples_per_s": round(1 / gpu_s, 2),
                     "speedup_over_torch_gpu_helper": round(gpu_s * 1e3 / ms, 2)})
    except Exception as e:      # noqa: BLE001 -- reported, not retried
        line["torch_gpu_helper"] = f"did not run: {type(e).__name__}: {str(e)[:200]}"
    print(json.dumps(line), flush=True)
    save()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("ns", "dlwp"), default="ns")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "graphcast_dlwp_step.json" if a.model == "dlwp" else "graphcast_step.json")
    if a.model == "dlwp":
        return main_dlwp(a)
    import graphcast_ref as R
    from dlwp_benchmark_amd import lib as L, nsbench
    from dlwp_benchmark_amd.train_engine import GraphedTrainStep
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    cfg, shape, roll = workload()
    B = shape[0]
    torch.manual_seed(0)
    x, target = R.make_inputs(cfg, shape, torch.Generator().manual_seed(1))
    model = nsbench.GraphCastNetNS(device=dev, **cfg).train()
    params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    line = {"model": "nsbench.GraphCastNetNS", "config": dict(cfg), "parameters": sum(v.numel() for v in params.values()), "batch": B,
            "frames": shape[1], "grid": [model.height, model.width], "nodes": model.graph.num_nodes, "edges": model.graph.num_edges,
            "rollout": roll, "precision": "fp32"}
    ind, yd = {"x": x.to(dev)}, target.to(dev)
    call = lambda m, kw: m(kw["x"], roll["teacher_forcing_steps"])      # noqa: E731

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump([line], f, indent=1)

    # ---- one eager step under the accounting
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        with L.kernel_accounting() as acc:
            torch.nn.functional.mse_loss(call(model, ind), yd).backward()
            torch.cuda.synchronize()
    total_ms, line["eager_step_kernels"] = accounting_rows(acc)
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
    save()
    # ---- the fused backward launch against the pair it replaces
    line["dgrad_mul_vs_pair"] = [dgrad_mul_against_the_pair(dev, model.graph.num_edges, wd) for wd in (34, 116)]
    save()
    try:
        gpu_s = helper_step_seconds(cfg, roll, params, x, target, dev, 3)
        del line["torch_gpu_helper"]
        line.update({"torch_gpu_helper_step_ms": round(gpu_s * 1e3, 2), "torch_gpu_helper_samples_per_s": round(B / gpu_s, 2),
                     "speedup_over_torch_gpu_helper": round(gpu_s * 1e3 / ms, 2)})
    except Exception as e:      # noqa: BLE001 -- reported, not retried
        line["torch_gpu_helper"] = f"did not run: {type(e).__name__}: {str(e)[:200]}"
    print(json.dumps(line), flush=True)
    save()


if __name__ == "__main__":
    main()
