#!/usr/bin/env python3
"""Golden vectors for the HEALPix padding and for ConvLSTMHPX, produced by IMPORTING the reference's code
(src/dlwpbench/utils/healpix.py and src/dlwpbench/models/convlstm/convlstm.py) in this container.

The model file does `from utils import CylinderPad, HEALPixLayer`: a stub module `utils` provides the reference's OWN CylinderPad
and its OWN HEALPixLayer (both loaded by path).

hpx_pad_golden.npz: HEALPixPadding(1) of tests/hpx_ref.py `pad_input(n)` (integer-valued float64, all values distinct: the
0.5 / 0.5 cells are exact) for the face sizes `PAD_SIZES`.

convlstm_hpx_golden.npz, per case of tests/hpx_ref.py CASES: inputs, parameters (default initialisation x 3 as in
make_convlstm_golden.py), output, mse loss against a stored random target and every parameter gradient from the reference's fp32
run, and the gaps of that run to the reference's float64 run, which must be within 1e-5 (output, loss) / 5e-5 (every gradient
tensor) relative to the float64 tensor's max norm.

    python tests/golden/make_hpx_golden.py
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
from hpx_ref import CASES, GOLDEN, PAD_GOLDEN, PAD_SIZES, make_inputs, pad_input, rel_gap  # noqa: E402

REF = "/root/reference/src"
SCALE = 3.0


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    healpix = _load("ref_dlwp_healpix", f"{REF}/dlwpbench/utils/healpix.py")
    ref_utils = _load("ref_dlwp_utils", f"{REF}/dlwpbench/utils/utils.py")
    stub = types.ModuleType("utils")
    stub.CylinderPad = ref_utils.CylinderPad
    stub.HEALPixLayer = healpix.HEALPixLayer
    sys.modules["utils"] = stub
    model = _load("ref_dlwp_convlstm", f"{REF}/dlwpbench/models/convlstm/convlstm.py")
    return healpix, model.ConvLSTMHPX


def run(net, inputs, target, dtype):
    net = copy.deepcopy(net).to(dtype)
    for cell in net.clstm:                       # the states are plain attributes: .to() does not reach them
        cell.h, cell.c = cell.h.to(dtype), cell.c.to(dtype)
    inp = {k: v.to(dtype) for k, v in inputs.items()}
    y = net(constants=inp["constants"], prescribed=inp.get("prescribed"), prognostic=inp["prognostic"])
    loss = torch.nn.functional.mse_loss(y, target.to(dtype))
    loss.backward()
    return y.detach(), loss.detach(), {n: p.grad for n, p in net.named_parameters()}


def save(name, arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 1024 * 1024, (path, size)
    print("wrote", path, len(arrays), "arrays", size // 1024, "KiB")


def main():
    healpix, ConvLSTMHPX = load_reference()
    pad = healpix.HEALPixPadding(padding=1)
    save(PAD_GOLDEN, {f"n{n}": pad(pad_input(n)).numpy() for n in PAD_SIZES})
    gen = torch.Generator().manual_seed(20261)
    torch.manual_seed(1412)
    o = {}
    for name, (cfg, B, T) in CASES.items():
        net = ConvLSTMHPX(batch_size=B * 12, device=torch.device("cpu"), **cfg)
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(SCALE)
        inputs, target = make_inputs(cfg, B, T, gen)
        y, loss, grads = run(net, inputs, target, torch.float32)
        y64, loss64, grads64 = run(net, inputs, target, torch.float64)
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
    save(GOLDEN, o)


if __name__ == "__main__":
    main()
