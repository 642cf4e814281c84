"""`dlwpbench.UNetHEALPix` on the MI355X against the golden vectors of the reference's UNetHPX
(tests/golden/make_unet_hpx_golden.py).

Bars (rel_gap: max |difference| relative to the max norm of the reference array): output 1e-4, loss 1e-4, every gradient tensor
5e-4 -- those of tests/test_gpu_convlstm_hpx.py; by the fixture's own assertion they sit 10 x above what the reference's fp32
arithmetic itself scatters around its float64 result (1e-5 / 5e-5).  Two passes over the same inputs must agree bit for bit (no
atomics anywhere), and the levels with small faces must have run the face-packed kernels.
"""
import os

import numpy as np
import pytest
import torch

from test_gpu_convlstm_hpx import compare
from unet_hpx_ref import CASES, GOLDEN, load_case, rel_gap

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def golden(name):
    return load_case(np.load(os.path.join(HERE, "golden", GOLDEN)), name)


def build(cfg, params, dev):
    from dlwp_benchmark_amd import dlwpbench
    net = dlwpbench.model_class("UNetHPX")(**cfg)
    net.load_state_dict({k: v.float() for k, v in params.items()}, strict=True)
    return net.to(dev)


def train_once(net, inputs, target, dev):
    net.zero_grad(set_to_none=True)
    kw = {k: inputs[k].to(dev) if k in inputs else None for k in ("constants", "prescribed", "prognostic")}
    y = net(**kw)
    loss = torch.nn.functional.mse_loss(y, target.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), loss.item(), {n: p.grad.detach().cpu() for n, p in net.named_parameters()}


@pytest.mark.parametrize("name", list(CASES))
def test_golden_case(cuda, name):
    from dlwp_benchmark_amd import lib as L
    from dlwp_benchmark_amd.dlwpbench.unet import packs_faces
    cfg, n, B, T = CASES[name]
    params, inputs, target, y, loss, grads, _ = golden(name)
    net = build(cfg, params, cuda)                        # load_state_dict(strict=True) of the reference's parameters
    with L.kernel_accounting() as acc:
        first = train_once(net, inputs, target, cuda)
    compare(name, first, (y, loss, grads))
    # ---- a second pass over the same inputs: bit-identical
    again = train_once(net, inputs, target, cuda)
    bits = lambda t: t.contiguous().view(torch.int32)      # noqa: E731
    assert torch.equal(bits(first[0]), bits(again[0])) and first[1] == again[1]
    for k in first[2]:
        assert torch.equal(bits(first[2][k]), bits(again[2][k])), f"{k}: two passes over the same inputs differ"
    # ---- which kernel family ran at which level: 2 convolutions per level and side, 1 + 1 at the bottom; one backward
    # product per forward one, except the input gradient of the first convolution of the first step (its input is data)
    rows = {r["name"]: r["calls"] for r in acc.rows}
    count = lambda *names: sum(rows.get(k, 0) for k in names)      # noqa: E731
    levels, steps = len(cfg["hidden_channels"]), T - cfg["context_size"]
    per_level = [4 if lvl < levels - 1 else 2 for lvl in range(levels)]
    packed = steps * sum(c for lvl, c in enumerate(per_level) if packs_faces(n >> lvl))
    plain = steps * sum(per_level) - packed
    first_packed = packs_faces(n)
    assert packed >= steps * (sum(per_level) - 4) and all(packs_faces(n >> lvl) for lvl in range(1, levels)), "levels with faces <= 4 pack"
    assert count("conv3x3_hpxp_n16", "conv3x3_hpxp_n64") == packed, rows
    assert count("conv3x3_hpx_n16", "conv3x3_hpx_n64") == plain, rows
    assert count("conv3x3_hpxp_wgrad") == packed and count("conv3x3_hpx_wgrad") == plain, rows
    assert count("conv3x3_hpxp_dgrad_n16", "conv3x3_hpxp_dgrad_n64") == count("conv3x3_hpxp_fold") == packed - first_packed, rows
    assert count("conv3x3_hpx_dgrad_n16", "conv3x3_hpx_dgrad_n64") == count("conv3x3_hpx_fold") == plain - (not first_packed), rows
    assert count("conv3x3_n16", "conv3x3_n64", "conv3x3_wgrad") == 0, rows


def test_eval_matches_train_and_spheres_are_independent(cuda):
    name = "unet_f4"
    cfg, n, B, T = CASES[name]
    params, inputs, target, y, _, _, _ = golden(name)
    net = build(cfg, params, cuda).eval()
    with torch.no_grad():
        y_eval = net(prognostic=inputs["prognostic"].to(cuda))
        assert not y_eval.requires_grad
        assert B == 2
        for i in range(B):
            y_one = net(prognostic=inputs["prognostic"][i:i + 1].to(cuda))
            assert rel_gap(y_one.cpu(), y[i:i + 1]) <= 1e-4 and rel_gap(y_one, y_eval[i:i + 1]) <= 1e-4      # the spheres of a batch are independent
    y_train = train_once(net.train(), inputs, target, cuda)[0]
    assert torch.equal(y_train.view(torch.int32), y_eval.cpu().view(torch.int32))
