#!/usr/bin/env python3
"""Golden vectors for the nsbench GraphCast baseline, produced by IMPORTING the reference's class
(src/nsbench/models/graphcast/graph_cast_net_ns.py, GraphCastNetNS) in this container.

The reference needs DGL, which is not installed here: it runs on the stub `dgl` of make_mgn_golden.py (DGL's documented
behaviour RESTATED, see there) with the same synthetic `models.graphcast.*` packages, plus two things this model alone needs:
* `dgl.to_networkx`, written below: a networkx DiGraph with the graph's integer node ids and one edge per directed edge (the
  reference only measures shortest-path lengths on it);
* the reference's OWN utils/activations.py, loaded by path into `models.graphcast.utils.activations`.

Per case (tests/graphcast_ref.py CASES): src, dst and edge_features of the reference's graph, input, target, parameters (default
initialisation, then ALL perturbed: weights x 1.5, every 1-D parameter + 0.2 randn), output, mse loss and every parameter gradient
from the reference's fp32 run.  The reference is also run in float64; its own fp32 result must sit within 1e-5 (output, loss) /
5e-5 (every gradient tensor) of that, relative to the float64 tensor's max norm.  Both gaps are stored (`gap_*`):
tests/test_graphcast_ref.py bounds the helper's float64 run by twice them.  Every gradient tensor must have a max norm of at
least 1e-6.

The width-116 case goes into a file of its own (graphcast_ns_w116_golden.npz): its parameters and gradients alone are 0.75 MiB,
and no committed file may pass 1 MiB.  All cases have B = 1 (the reference never batches its graph: the `cat` in agg_concat_dgl raises for more) and one channel (with
more its residual `x_t[:, -1:]` adds the LAST channel to every output channel).

    python tests/golden/make_graphcast_ns_golden.py
"""
import copy
import os
import sys

import networkx as nx
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_mgn_golden import REF, _load_as, install_dgl, load_app  # noqa: E402
from graphcast_ref import CASES, GOLDEN_OF, make_inputs, rel_gap  # noqa: E402


def to_networkx(g):
    out = nx.DiGraph()
    out.add_nodes_from(range(g.num_nodes()))
    s, d = g.edges()
    out.add_edges_from(zip(s.tolist(), d.tolist()))
    return out


def load_reference():
    install_dgl()
    sys.modules["dgl"].to_networkx = to_networkx
    load_app("nsbench")               # the synthetic packages with the reference's gnn_layers, meta and the stub Module
    base = f"{REF}/nsbench/models/graphcast"
    _load_as("models.graphcast.utils.activations", f"{base}/utils/activations.py")
    return _load_as("ref_nsbench_graphcast", f"{base}/graph_cast_net_ns.py").GraphCastNetNS


def run(net, x, target, roll, dtype):
    net = copy.deepcopy(net).to(dtype)
    net.efeats = net.efeats.to(dtype)          # a plain attribute, not a buffer: .to(dtype) leaves it
    y = net(x.to(dtype), **roll)
    loss = torch.nn.functional.mse_loss(y, target.to(dtype))
    loss.backward()
    return y.detach(), loss.detach(), {n: p.grad for n, p in net.named_parameters()}


def main():
    cls = load_reference()
    files = {f: {} for f in GOLDEN_OF.values()}
    for i, (name, (cfg, shape, roll)) in enumerate(CASES.items()):
        o = files[GOLDEN_OF[name]]
        gen = torch.Generator().manual_seed(41017 + i)      # per case: adding a case leaves the others' draws alone
        torch.manual_seed(1618 + i)
        net = cls(device="cpu", **cfg)
        with torch.no_grad():
            for p in net.parameters():
                if p.dim() == 1:
                    p.add_(0.2 * torch.randn(p.shape, generator=gen))
                else:
                    p.mul_(1.5)
        x, target = make_inputs(cfg, shape, gen)
        y, loss, grads = run(net, x, target, roll, torch.float32)
        y64, loss64, grads64 = run(net, x, target, roll, torch.float64)
        gaps = {"y": rel_gap(y, y64), "loss": rel_gap(loss, loss64)}
        gaps.update({"g_" + n: rel_gap(grads[n], grads64[n]) for n in grads})
        assert gaps["y"] <= 1e-5 and gaps["loss"] <= 1e-5, (name, gaps["y"], gaps["loss"])
        worst = max(v for k, v in gaps.items() if k.startswith("g_"))
        assert worst <= 5e-5, (name, worst)
        smallest = min(float(g.abs().max()) for g in grads.values())
        assert smallest >= 1e-6, (name, {n: float(g.abs().max()) for n, g in grads.items() if float(g.abs().max()) < 1e-6})
        src, dst = net.mesh_graph.edges()
        o[f"{name}/src"], o[f"{name}/dst"] = src.numpy().astype(np.int32), dst.numpy().astype(np.int32)
        o[f"{name}/edge_features"] = net.efeats.numpy()
        o[f"{name}/in_x"], o[f"{name}/target"] = x.numpy(), target.numpy()
        o[f"{name}/y"], o[f"{name}/loss"] = y.numpy(), np.float32(loss.item())
        for n, p in net.named_parameters():
            o[f"{name}/p_{n}"], o[f"{name}/g_{n}"] = p.detach().numpy(), grads[n].numpy()
        for k, v in gaps.items():
            o[f"{name}/gap_{k}"] = np.float64(v)
        print(f"{name}: N {net.mesh_graph.num_nodes()} E {net.mesh_graph.num_edges()} loss {loss.item():.6f}  fp32-vs-fp64 gap: output "
              f"{gaps['y']:.2e}, loss {gaps['loss']:.2e}, gradients <= {worst:.2e}, smallest gradient tensor {smallest:.2e}")
    for fname, o in files.items():
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **o)
        size = os.path.getsize(path)
        assert size < 1024 * 1024, (path, size)
        print("wrote", path, len(o), "arrays", size // 1024, "KiB")


if __name__ == "__main__":
    main()
