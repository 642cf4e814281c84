#!/usr/bin/env python3
"""Training-step time of the nsbench U-Net at the published protocol: B 4, 64 x 64, sequence 50, context_size 10, teacher
forcing 10, circular padding, fp32, Adam; widths 8-16-32-64-128, 16-32-64-128-256 and 33-66-132-264-528 of
src/nsbench/scripts/train_commands.txt (lines 8, 10, 12).

Per width one JSON line: the graphed step (train_engine.GraphedTrainStep, 3 warm-up steps, median of >= 10), samples/s, the
per-kernel accounting of ONE eager step (lib.kernel_accounting: name, calls, ms, TFLOP/s, fraction of the 157.3 TFLOP/s fp32
matrix roof and of 8 TB/s), the share of that kernel time spent in the kernels of csrc/unet_ops.hip, the share spent on maps
below 16 x 16 (the accounting has one row per kernel name, not per grid, so every level's modules are replayed forward and
backward on tensors of that level's shapes and accounted on their own), the same step of the plain-torch helper model
(tests/unet_ref.py) on the host CPU with 16 threads, and the helper on the GPU on torch's own convolutions ("what a user gets
without this library"; a failure there is reported in the line, nothing is retried).

    python tools/bench_unet.py [--widths 8-16-32-64-128,...] [--steps 10] [--out profiles/unet_step.json] [--append]

`--mesh healpix` times `dlwpbench.UNetHEALPix` instead: HPX8 (12 faces of 8 x 8), 16 spheres, 4 constant + 1 prescribed + 8
prognostic channels, context_size 1, 5 frames (the protocol of tools/bench_convlstm.py --mesh healpix), the graphed step as
above.  Widths: the first four levels of the three widths above (a fifth level does not exist below 1 x 1 faces) and the
published 92-184-368-736.  Per width the per-kernel accounting of one eager step and the kernel time of one network call per
level (faces of 8, 4, 2, 1 pixels) with its share.

    python tools/bench_unet.py --mesh healpix [--widths ...] --out profiles/unet_hpx_step.json
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
B, H, W, SEQ, TF, CTX = 4, 64, 64, 50, 10, 10
NEW_KERNELS = ("avgpool2x2_fwd", "avgpool2x2_bwd", "conv1x1", "upconv2x2_fwd", "upconv2x2_dgrad", "pixel_wgrad", "pixel_wgrad_fold")


def helper_step_seconds(params, x, y, device, reps):
    """forward + backward + Adam of the helper model; median seconds per step"""
    import unet_ref as R
    p = {k: v.detach().clone().to(device).requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)
    x, y = x.to(device), y.to(device)
    times = []
    for i in range(reps + 1):
        if device.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(R.ns_forward(p, x, TF, CTX, "circular", "relu"), y)
        loss.backward()
        opt.step()
        if device.type == "cuda":
            torch.cuda.synchronize()
        if i:                                   # the first step warms allocators and kernel caches
            times.append(time.perf_counter() - t0)
    return statistics.median(times)


def level_kernel_ms(model, dev):
    """Kernel milliseconds (forward + backward, lib.kernel_accounting) of ONE network call per level, measured by replaying
    each level's own modules on random tensors of that level's shapes: [(grid height, ms)], top level first, and the output
    layer's.  The per-kernel accounting of the whole step has one row per kernel name, not per grid; this splits it."""
    from dlwp_benchmark_amd import lib as L
    from dlwp_benchmark_amd.nsbench.unet import pack_all, run_level
    packs = pack_all(model.encoder, model.decoder)
    hs, n = model.hidden_channels, len(model.hidden_channels)
    r = lambda h, c: torch.randn(B, h, h * W // H, c, device=dev, requires_grad=True)      # noqa: E731

    def timed(fn):
        for _ in range(2):                       # the second run is the one kept (allocator and kernel caches warm)
            with L.kernel_accounting() as acc:
                out = fn()
                out.backward(torch.randn_like(out))
                torch.cuda.synchronize()
        return sum(row["ms"] for row in acc.rows)

    levels = []
    for lvl in range(n):
        h = H >> lvl
        cin = model.in_channels * CTX if lvl == 0 else hs[lvl - 1]
        enc, dec = model.encoder.layers[lvl], model.decoder.layers[n - 1 - lvl]
        ms = timed(lambda: run_level(enc, r(h if lvl == 0 else 2 * h, cin), packs))
        ms += timed(lambda: run_level(dec, r(h, hs[lvl]), packs, skip=r(h, hs[lvl]) if lvl < n - 1 else None))
        levels.append((h, ms))
    return levels, timed(lambda: model.decoder.output_layer.forward_cl(r(H, hs[0])))


HPX_B, HPX_FACE, HPX_SEQ = 16, 8, 5
HPX_CH = dict(constant_channels=4, prescribed_channels=1, prognostic_channels=8, context_size=1)
HPX_WIDTHS = "8-16-32-64,16-32-64-128,33-66-132-264,92-184-368-736"


def hpx_level_kernel_ms(model, dev):
    """as level_kernel_ms for the HEALPix model: [(face size, packed family?, ms)] per level, and the output layer's"""
    from dlwp_benchmark_amd import lib as L
    from dlwp_benchmark_amd.dlwpbench.unet import packs_faces
    from dlwp_benchmark_amd.nsbench.unet import pack_all, run_level
    packs = pack_all(model.encoder, model.decoder)
    hs, n = model.hidden_channels, len(model.hidden_channels)
    r = lambda f, c: torch.randn(HPX_B * 12, f, f, c, device=dev, requires_grad=True)      # noqa: E731

    def timed(fn):
        for _ in range(2):
            with L.kernel_accounting() as acc:
                out = fn()
                out.backward(torch.randn_like(out))
                torch.cuda.synchronize()
        return sum(row["ms"] for row in acc.rows)

    cin0 = HPX_CH["constant_channels"] + (HPX_CH["prescribed_channels"] + HPX_CH["prognostic_channels"]) * HPX_CH["context_size"]
    levels = []
    for lvl in range(n):
        f = HPX_FACE >> lvl
        enc, dec = model.encoder.layers[lvl], model.decoder.layers[n - 1 - lvl]
        ms = timed(lambda: run_level(enc, r(f if lvl == 0 else 2 * f, cin0 if lvl == 0 else hs[lvl - 1]), packs))
        ms += timed(lambda: run_level(dec, r(f, hs[lvl]), packs, skip=r(f, hs[lvl]) if lvl < n - 1 else None))
        levels.append((f, packs_faces(f), ms))
    return levels, timed(lambda: model.decoder.output_layer.forward_cl(r(HPX_FACE, hs[0])))


def hpx_lines(a, dev, lines):
    from dlwp_benchmark_amd import dlwpbench, lib as L
    from dlwp_benchmark_amd.train_engine import GraphedTrainStep
    for spec in (a.widths or HPX_WIDTHS).split(","):
        hidden = [int(v) for v in spec.split("-")]
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(1)
        r = lambda t, c: torch.randn(HPX_B, t, c, 12, HPX_FACE, HPX_FACE, generator=g).to(dev)      # noqa: E731
        kw = {"constants": r(1, HPX_CH["constant_channels"]), "prescribed": r(HPX_SEQ, HPX_CH["prescribed_channels"]),
              "prognostic": r(HPX_SEQ, HPX_CH["prognostic_channels"])}
        yd = r(HPX_SEQ - HPX_CH["context_size"], HPX_CH["prognostic_channels"])
        model = dlwpbench.UNetHEALPix(hidden_channels=hidden, n_convolutions=2, activation="th.nn.ReLU()", device=dev, **HPX_CH).train()
        line = {"model": f"dlwpbench.UNetHEALPix {spec}", "mesh": "healpix", "parameters": sum(p.numel() for p in model.parameters()),
                "batch": HPX_B, "grid": [12, HPX_FACE, HPX_FACE], "sequence": HPX_SEQ, "context_size": HPX_CH["context_size"],
                "precision": "fp32"}
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            with L.kernel_accounting() as acc:
                torch.nn.functional.mse_loss(model(**kw), yd).backward()
                torch.cuda.synchronize()
        total_ms = sum(r_["ms"] for r_ in acc.rows)
        line["eager_step_kernels"] = [
            {"name": r_["name"], "calls": r_["calls"], "ms": round(r_["ms"], 3),
             "tflops": round(r_["flops"] / (r_["ms"] * 1e9), 2) if r_["ms"] else 0.0,
             "fraction_of_8TBs": round(r_["bytes"] / (r_["ms"] * 1e9) / ROOF_TBS, 4) if r_["ms"] else 0.0,
             "share_of_kernel_time": round(r_["ms"] / total_ms, 4)} for r_ in acc.rows]
        line["eager_step_kernel_ms"] = round(total_ms, 3)
        levels, out_ms = hpx_level_kernel_ms(model, dev)
        all_ms = sum(ms for _, _, ms in levels) + out_ms
        line["kernel_ms_per_network_call_by_level"] = [{"face": f, "packed_kernels": pk, "ms": round(ms, 4), "share": round(ms / all_ms, 4)}
                                                       for f, pk, ms in levels]
        model.zero_grad(set_to_none=True)
        step = GraphedTrainStep(model, kw, yd, lr=1e-3)
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
        line.update({"step_ms": round(ms, 3), "step_ms_spread": round((max(times) - min(times)) * 1e3, 3),
                     "samples_per_s": round(HPX_B / ms * 1e3, 2), "steps_timed": len(times), "loss": float(step.loss.item())})
        del step, model
        lines.append(line)
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="ns", choices=["ns", "healpix"], help="ns: the nsbench model (default); healpix: dlwpbench.UNetHEALPix")
    ap.add_argument("--widths", default=None, help="default 8-16-32-64-128,16-32-64-128-256,33-66-132-264-528 (ns) or "
                    "8-16-32-64,16-32-64-128,33-66-132-264,92-184-368-736 (healpix)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--out", default=None, help="default profiles/unet_step.json (ns) or profiles/unet_hpx_step.json (healpix)")
    ap.add_argument("--append", action="store_true", help="keep the lines already in --out (one width per invocation)")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "unet_hpx_step.json" if a.mesh == "healpix" else "unet_step.json")
    from dlwp_benchmark_amd import lib as L, nsbench
    from dlwp_benchmark_amd.train_engine import GraphedTrainStep
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    lines = []
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            lines = json.load(f)
    if a.mesh == "healpix":
        return hpx_lines(a, dev, lines)
    for spec in (a.widths or "8-16-32-64-128,16-32-64-128-256,33-66-132-264-528").split(","):
        hidden = [int(v) for v in spec.split("-")]
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(1)
        u = torch.randn(B, SEQ + 1, 1, H, W, generator=g)
        x, y = u[:, :-1].contiguous(), u[:, 1:].contiguous()
        model = nsbench.UNet(in_channels=1, hidden_channels=hidden, out_channels=1, n_convolutions=2, activation="th.nn.ReLU()",
                             padding_mode="circular", context_size=CTX, device=dev).train()
        params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        line = {"model": f"nsbench.UNet {spec}", "parameters": sum(v.numel() for v in params.values()), "batch": B,
                "grid": [H, W], "sequence": SEQ, "context_size": CTX, "teacher_forcing_steps": TF, "padding_mode": "circular",
                "precision": "fp32"}
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
        line["share_of_kernel_time_in_new_kernels"] = round(sum(r["ms"] for r in acc.rows if r["name"] in NEW_KERNELS) / total_ms, 4)
        levels, out_ms = level_kernel_ms(model, dev)
        line["kernel_ms_per_network_call_by_level"] = [{"grid": [h, h * W // H], "ms": round(ms, 4)} for h, ms in levels]
        line["share_of_kernel_time_below_16x16"] = round(sum(ms for h, ms in levels if h < 16) / (sum(ms for _, ms in levels) + out_ms), 4)
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
        # ---- the helper on the host CPU (16 threads) and on the card on torch's own convolutions
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
            line.update({"torch_gpu_helper_step_ms": round(gpu_s * 1e3, 2), "torch_gpu_helper_samples_per_s": round(B / gpu_s, 2),
                         "speedup_over_torch_gpu_helper": round(gpu_s * 1e3 / ms, 2)})
        except Exception as e:      # noqa: BLE001 -- reported, not retried
            line["torch_gpu_helper"] = f"did not run: {type(e).__name__}: {str(e)[:200]}"
        print(json.dumps(line), flush=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
