#!/usr/bin/env python3
"""Golden vectors for the U-Net on the HEALPix mesh, produced by IMPORTING the reference's code
(src/dlwpbench/models/unet/unet.py `UNetHPX` and src/dlwpbench/utils/healpix.py) in this container.

The model file does `from utils import CylinderPad, HEALPixLayer`: a stub module `utils` provides the reference's OWN CylinderPad
and its OWN HEALPixLayer (both loaded by path), as in make_hpx_golden.py.

unet_hpx_golden.npz, per case of tests/unet_hpx_ref.py CASES: inputs, parameters (default initialisation x 3), output, mse loss
against a stored random target and every parameter gradient from the reference's fp32 run, and the gaps of that run to the
reference's float64 run, which must be within 1e-5 (output, loss) / 5e-5 (every gradient tensor) relative to the float64
tensor's max norm.  `pad_n1`: HEALPixPadding(1) of tests/hpx_ref.py `pad_input(1)` (one pixel per face, all values distinct).

    python tests/golden/make_unet_hpx_golden.py
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
from make_hpx_golden import REF, SCALE, _load, save  # noqa: E402
from unet_hpx_ref import CASES, GOLDEN, PAD_KEY, make_inputs, pad_input, rel_gap  # noqa: E402


def load_reference():
    healpix = _load("ref_dlwp_healpix", f"{REF}/dlwpbench/utils/healpix.py")
    ref_utils = _load("ref_dlwp_utils", f"{REF}/dlwpbench/utils/utils.py")
    stub = types.ModuleType("utils")
    stub.CylinderPad = ref_utils.CylinderPad
    stub.HEALPixLayer = healpix.HEALPixLayer
    sys.modules["utils"] = stub
    model = _load("ref_dlwp_unet", f"{REF}/dlwpbench/models/unet/unet.py")
    return healpix, model.UNetHPX


def run(net, inputs, target, dtype):
    net = copy.deepcopy(net).to(dtype)
    inp = {k: v.to(dtype) for k, v in inputs.items()}
    y = net(constants=inp.get("constants"), prescribed=inp.get("prescribed"), prognostic=inp["prognostic"])
    loss = torch.nn.functional.mse_loss(y, target.to(dtype))
    loss.backward()
    return y.detach(), loss.detach(), {n: p.grad for n, p in net.named_parameters()}


def main():
    healpix, UNetHPX = load_reference()
    o = {PAD_KEY: healpix.HEALPixPadding(padding=1)(pad_input(1)).numpy()}
    gen = torch.Generator().manual_seed(20262)
    torch.manual_seed(1413)
    for name, (cfg, n, B, T) in CASES.items():
        net = UNetHPX(**cfg)
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(SCALE)
        inputs, target = make_inputs(cfg, n, B, T, gen)
        y, loss, grads = run(net, inputs, target, torch.float32)
        y64, loss64, grads64 = run(net, inputs, target, torch.float64)
        gaps = {"y": rel_gap(y, y64), "loss": rel_gap(loss, loss64)}
        gaps.update({"g_" + k: rel_gap(grads[k], grads64[k]) for k in grads})
        assert gaps["y"] <= 1e-5 and gaps["loss"] <= 1e-5, (name, gaps["y"], gaps["loss"])
        worst = max(v for k, v in gaps.items() if k.startswith("g_"))
        assert worst <= 5e-5, (name, worst)
        for k, v in inputs.items():
            o[f"{name}/in_{k}"] = v.numpy()
        o[f"{name}/target"], o[f"{name}/y"], o[f"{name}/loss"] = target.numpy(), y.numpy(), np.float32(loss.item())
        for k, p in net.named_parameters():
            o[f"{name}/p_{k}"], o[f"{name}/g_{k}"] = p.detach().numpy(), grads[k].numpy()
        for k, v in gaps.items():
            o[f"{name}/gap_{k}"] = np.float64(v)
        print(f"{name}: loss {loss.item():.6f}  fp32-vs-fp64 gap: output {gaps['y']:.2e}, loss {gaps['loss']:.2e}, gradients <= {worst:.2e}, "
              f"smallest gradient tensor {min(float(g.abs().max()) for g in grads.values()):.2e}")
    save(GOLDEN, o)


if __name__ == "__main__":
    main()
