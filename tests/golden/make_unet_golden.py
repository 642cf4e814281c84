#!/usr/bin/env python3
"""Golden vectors for the two U-Net baselines, produced by IMPORTING the reference's classes
(src/nsbench/models/unet/unet.py and src/dlwpbench/models/unet/unet.py) in this container.

The dlwpbench file does `from utils import CylinderPad, HEALPixLayer`: a stub module `utils` provides the reference's OWN
CylinderPad (src/dlwpbench/utils/utils.py loaded by path) and an empty HEALPixLayer (the healpix branch is not built).

Per case (tests/unet_ref.py CASES): inputs, parameters (default initialisation x 2: at x 1 one gradient tensor of the deepest
case falls to 1e-10 and pins nothing), output, mse loss against a stored random target and every parameter gradient, all from
the reference's fp32 run.  The reference is also run in float64; its own fp32 result must sit within 1e-5 (output, loss) / 5e-5
(every gradient tensor) of that, relative to the float64 tensor's max norm.  Both gaps are stored (`gap_*`):
tests/test_unet_ref.py bounds the helper's float64 run by twice them.

    python tests/golden/make_unet_golden.py
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_convlstm_golden import REF, _load  # noqa: E402
from unet_ref import CASES, GOLDEN, make_inputs, rel_gap  # noqa: E402

SCALE = 2.0


def load_reference():
    ns = _load("ref_ns_unet", f"{REF}/nsbench/models/unet/unet.py")
    ref_utils = _load("ref_dlwp_utils", f"{REF}/dlwpbench/utils/utils.py")
    stub = types.ModuleType("utils")
    stub.CylinderPad = ref_utils.CylinderPad
    stub.HEALPixLayer = type("HEALPixLayer", (torch.nn.Module,), {})
    sys.modules["utils"] = stub
    dlwp = _load("ref_dlwp_unet", f"{REF}/dlwpbench/models/unet/unet.py")
    return {"ns": ns.UNet, "dlwp": dlwp.UNet}


def run(net, kind, inputs, target, roll, dtype):
    net = copy.deepcopy(net).to(dtype)
    inp = {k: v.to(dtype) for k, v in inputs.items()}
    y = net(inp["x"], **roll) if kind == "ns" else net(constants=inp.get("constants"), prescribed=inp.get("prescribed"),
                                                       prognostic=inp["prognostic"])
    loss = torch.nn.functional.mse_loss(y, target.to(dtype))
    loss.backward()
    return y.detach(), loss.detach(), {n: p.grad for n, p in net.named_parameters()}


def main():
    classes = load_reference()
    out = {"ns": {}, "dlwp": {}}
    for i, (name, (kind, cfg, shape, roll)) in enumerate(CASES.items()):
        gen = torch.Generator().manual_seed(20261 + i)      # per case: adding a case leaves the others' draws alone
        torch.manual_seed(1412 + i)
        net = classes[kind](**cfg)
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(SCALE)
        inputs, target = make_inputs(kind, cfg, shape, gen)
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
