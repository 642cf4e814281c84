#!/usr/bin/env python3
"""Golden vectors for the two ConvLSTM baselines, produced by IMPORTING the reference's classes
(src/nsbench/models/convlstm/convlstm.py and src/dlwpbench/models/convlstm/convlstm.py) in this container.

The dlwpbench file does `from utils import CylinderPad, HEALPixLayer`: a stub module `utils` provides the reference's OWN
CylinderPad (src/dlwpbench/utils/utils.py loaded by path) and an empty HEALPixLayer (the healpix branch is not built).

Per case (tests/convlstm_ref.py CASES): inputs, parameters (default initialisation x 3, so that 5 - 8 % of the gate
pre-activations lie beyond |z| = 2), output, mse loss against a stored random target and every parameter gradient, all from the
reference's fp32 run.  The reference is also run in float64; its own fp32 result must sit within 1e-5 (output, loss) / 5e-5
(every gradient tensor) of that, relative to the float64 tensor's max norm -- a case that fails this is too ill-conditioned to
pin anything.  Both gaps are stored (`gap_*`): tests/test_convlstm_ref.py bounds the helper's float64 run by twice them.

    python tests/golden/make_convlstm_golden.py
"""
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from convlstm_ref import CASES, GOLDEN, make_inputs, rel_gap  # noqa: E402

REF = "/root/reference/src"
SCALE = 3.0


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    ns = _load("ref_ns_convlstm", f"{REF}/nsbench/models/convlstm/convlstm.py")
    ref_utils = _load("ref_dlwp_utils", f"{REF}/dlwpbench/utils/utils.py")
    stub = types.ModuleType("utils")
    stub.CylinderPad = ref_utils.CylinderPad
    stub.HEALPixLayer = type("HEALPixLayer", (torch.nn.Module,), {})
    sys.modules["utils"] = stub
    dlwp = _load("ref_dlwp_convlstm", f"{REF}/dlwpbench/models/convlstm/convlstm.py")
    return {"ns": ns.ConvLSTM, "dlwp": dlwp.ConvLSTM}


def run(net, kind, inputs, target, roll, dtype):
    net = copy.deepcopy(net).to(dtype)
    for cell in net.clstm:                       # the states are plain attributes: .to() does not reach them
        cell.h, cell.c = cell.h.to(dtype), cell.c.to(dtype)
    inp = {k: v.to(dtype) for k, v in inputs.items()}
    y = net(inp["x"], **roll) if kind == "ns" else net(constants=inp["constants"], prescribed=inp.get("prescribed"),
                                                       prognostic=inp["prognostic"])
    loss = torch.nn.functional.mse_loss(y, target.to(dtype))
    loss.backward()
    return y.detach(), loss.detach(), {n: p.grad for n, p in net.named_parameters()}


def main():
    classes = load_reference()
    gen = torch.Generator().manual_seed(20260)
    torch.manual_seed(1411)
    out = {"ns": {}, "dlwp": {}}
    for name, (kind, cfg, B, T, roll) in CASES.items():
        net = classes[kind](batch_size=B, device=torch.device("cpu"), **cfg)
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(SCALE)
        inputs, target = make_inputs(kind, cfg, B, T, gen)
        y, loss, grads = run(net, kind, inputs, target, roll, torch.float32)
        y64, loss64, grads64 = run(net, kind, inputs, target, roll, torch.float64)
        o = out[kind]
        gaps = {"y": rel_gap(y, y64), "loss": rel_gap(loss, loss64)}
        gaps.update({"g_" + n: rel_gap(grads[n], grads64[n]) for n in grads})
        assert gaps["y"] <= 1e-5 and gaps["loss"] <= 1e-5, (name, gaps["y"], gaps["loss"])
        worst = max(v for k, v in gaps.items() if k.startswith("g_"))
        assert worst <= 5e-5, (name, worst)
        for k, v in inputs.items():
            o[f"{name}/in_{k}"] = v.numpy()
        o[f"{name}/target"], o[f"{name}/y"], o[f"{name}/loss"] = target.numpy(), y.numpy(), np.float32(loss.item())
        for n, p in net.named_parameters():
            o[f"{name}/p_{n}"], o[f"{name}/g_{n}"] = p.detach().numpy(), grads[n].numpy()
        for k, v in gaps.items():
            o[f"{name}/gap_{k}"] = np.float64(v)
        print(f"{name}: loss {loss.item():.6f}  fp32-vs-fp64 gap: output {gaps['y']:.2e}, loss {gaps['loss']:.2e}, gradients <= {worst:.2e}, "
              f"smallest gradient tensor {min(float(g.abs().max()) for g in grads.values()):.2e}")
    for kind, arrays in out.items():
        path = os.path.join(HERE, GOLDEN[kind])
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size < 1024 * 1024, (path, size)
        print("wrote", path, len(arrays), "arrays", size // 1024, "KiB")


if __name__ == "__main__":
    main()
