#!/usr/bin/env python3
"""Golden vectors for the two MeshGraphNet baselines, produced by IMPORTING the reference's classes
(src/nsbench/models/mgn/meshgraphnet.py and src/dlwpbench/models/mgn/meshgraphnet.py) in this container.

The reference needs DGL, which is not installed here.  DGL is its graph container, not its arithmetic, so this script installs
a stub `dgl` / `dgl.function` written below from DGL's documented behaviour (RESTATED, not executed):
* `from_networkx` relabels the nodes to consecutive integers in sorted label order and gives an undirected edge both directions;
* `to_bidirected` adds the reverse of every edge and drops duplicates;
* `batch` offsets the node ids of graph b by the nodes before it;
* `apply_edges(f)` hands f the edge data and the node data gathered at the sources and destinations;
* `update_all(copy_e, sum | mean)` reduces the edge rows onto their destination nodes (mean: zero for a node without in-edges).
It also builds the synthetic packages `models`, `models.graphcast`, `models.graphcast.gnn_layers` (with an empty CuGraphCSC) and
`models.graphcast.utils` and loads the reference's OWN gnn_layers/{utils,mesh_graph_mlp,mesh_edge_block,mesh_node_block}.py and
utils/meta.py into them by path; `models.graphcast.utils.module.Module` is a stub nn.Module taking `meta=` (the real one imports
fsspec, s3fs and requests, which are absent).

Per case (tests/mgn_ref.py CASES): src, dst and edge_features of the reference's graph, inputs, target, parameters (default
initialisation, then ALL perturbed: weights x 1.5, every 1-D parameter + 0.2 randn, so that LayerNorm's gamma != 1 and beta != 0
are exercised), output, mse loss and every parameter gradient from the reference's fp32 run.  The reference is also run in
float64; its own fp32 result must sit within 1e-5 (output, loss) / 5e-5 (every gradient tensor) of that, relative to the float64
tensor's max norm.  Both gaps are stored (`gap_*`): tests/test_mgn_ref.py bounds the helper's float64 run by twice them.  Every
gradient tensor must have a max norm of at least 1e-6 (a case with an all-zero gradient pins nothing).

nsbench cases have one channel: with more the reference's residual `x_t[:, -1:]` adds the LAST channel to every output channel
and its warm-up frames have the wrong shape.  dlwpbench cases have T = context_size + 1: the reference raises beyond that.

    python tests/golden/make_mgn_golden.py
"""
import contextlib
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_convlstm_golden import REF  # noqa: E402
from mgn_ref import CASES, GOLDEN, make_inputs, rel_gap  # noqa: E402


# ---------------------------------------------------------------- the stub dgl
class StubGraph:
    def __init__(self, src, dst, num_nodes, batch_size=1):
        self._src, self._dst, self._n, self.batch_size = src.long(), dst.long(), int(num_nodes), batch_size
        self.ndata, self.edata = {}, {}

    srcdata = property(lambda self: self.ndata)
    dstdata = property(lambda self: self.ndata)

    def edges(self):
        return self._src, self._dst

    def nodes(self):
        return torch.arange(self._n)

    def num_nodes(self):
        return self._n

    def num_edges(self):
        return len(self._src)

    def to(self, *args, **kwargs):
        return self

    @contextlib.contextmanager
    def local_scope(self):
        nd, ed = dict(self.ndata), dict(self.edata)
        try:
            yield
        finally:
            self.ndata, self.edata = nd, ed

    def apply_edges(self, func):
        edges = types.SimpleNamespace(data=self.edata, src={k: v[self._src] for k, v in self.ndata.items()},
                                      dst={k: v[self._dst] for k, v in self.ndata.items()})
        self.edata.update(func(edges))

    def update_all(self, message, reduce):
        (kind, field, msg), (how, msg2, out) = message, reduce
        assert kind == "copy_e" and msg == msg2 and how in ("sum", "mean")
        e = self.edata[field]
        acc = torch.zeros((self._n,) + tuple(e.shape[1:]), dtype=e.dtype).index_add_(0, self._dst, e)
        if how == "mean":
            deg = torch.zeros(self._n, dtype=e.dtype).index_add_(0, self._dst, torch.ones(len(self._dst), dtype=e.dtype))
            acc = acc / deg.clamp(min=1)[:, None]
        self.ndata[out] = acc


def from_networkx(g):
    label = {u: i for i, u in enumerate(sorted(g.nodes))}
    pairs = set()
    for u, v in g.edges():
        pairs.add((label[u], label[v]))
        pairs.add((label[v], label[u]))
    pairs = sorted(pairs)
    return StubGraph(torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs]), len(label))


def to_bidirected(g):
    s, d = g.edges()
    pairs = sorted(set(zip(s.tolist(), d.tolist())) | set(zip(d.tolist(), s.tolist())))
    return StubGraph(torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs]), g.num_nodes())


def batch(graphs):
    off, src, dst = 0, [], []
    for g in graphs:
        s, d = g.edges()
        src.append(s + off)
        dst.append(d + off)
        off += g.num_nodes()
    return StubGraph(torch.cat(src), torch.cat(dst), off, batch_size=len(graphs))


def install_dgl():
    dgl = types.ModuleType("dgl")
    dgl.DGLGraph = dgl.graph = StubGraph
    dgl.from_networkx, dgl.to_bidirected, dgl.batch = from_networkx, to_bidirected, batch
    fn = types.ModuleType("dgl.function")
    fn.copy_e = lambda field, msg: ("copy_e", field, msg)
    fn.sum = lambda msg, out: ("sum", msg, out)
    fn.mean = lambda msg, out: ("mean", msg, out)
    dgl.function = fn
    sys.modules["dgl"], sys.modules["dgl.function"] = dgl, fn


def _load_as(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_app(app):
    """the reference's MeshGraphNet class of `app` with its own gnn_layers loaded into synthetic packages"""
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[k]
    base = f"{REF}/{app}/models"
    for name in ("models", "models.graphcast", "models.graphcast.gnn_layers", "models.graphcast.utils"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    sys.modules["models.graphcast.gnn_layers"].CuGraphCSC = type("CuGraphCSC", (), {})
    for m in ("utils", "mesh_graph_mlp", "mesh_edge_block", "mesh_node_block"):
        _load_as(f"models.graphcast.gnn_layers.{m}", f"{base}/graphcast/gnn_layers/{m}.py")
    _load_as("models.graphcast.utils.meta", f"{base}/graphcast/utils/meta.py")
    module = types.ModuleType("models.graphcast.utils.module")

    class Module(torch.nn.Module):
        def __init__(self, meta=None):
            super().__init__()
            self.meta = meta

    module.Module = Module
    sys.modules["models.graphcast.utils.module"] = module
    return _load_as(f"ref_{app}_mgn", f"{base}/mgn/meshgraphnet.py").MeshGraphNet


def load_reference():
    install_dgl()
    return {"ns": load_app("nsbench"), "dlwp": load_app("dlwpbench")}


def construct(cls, cfg):
    kw = dict(cfg)
    kw["graph"] = types.SimpleNamespace(**cfg["graph"])
    return cls(device="cpu", **kw)


def run(net, kind, inputs, target, roll, dtype):
    net = copy.deepcopy(net).to(dtype)
    net.edge_features = net.edge_features.to(dtype)          # plain attributes, not buffers: .to(dtype) leaves them
    net.batched_edge_features = net.batched_edge_features.to(dtype)
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
        gen = torch.Generator().manual_seed(30517 + i)      # per case: adding a case leaves the others' draws alone
        torch.manual_seed(2718 + i)
        net = construct(classes[kind], cfg)
        with torch.no_grad():
            for p in net.parameters():
                if p.dim() == 1:
                    p.add_(0.2 * torch.randn(p.shape, generator=gen))
                else:
                    p.mul_(1.5)
        inputs, target = make_inputs(kind, cfg, shape, gen)
        y, loss, grads = run(net, kind, inputs, target, roll, torch.float32)
        y64, loss64, grads64 = run(net, kind, inputs, target, roll, torch.float64)
        o = out[kind]
        gaps = {"y": rel_gap(y, y64), "loss": rel_gap(loss, loss64)}
        gaps.update({"g_" + n: rel_gap(grads[n], grads64[n]) for n in grads})
        assert gaps["y"] <= 1e-5 and gaps["loss"] <= 1e-5, (name, gaps["y"], gaps["loss"])
        worst = max(v for k, v in gaps.items() if k.startswith("g_"))
        assert worst <= 5e-5, (name, worst)
        smallest = min(float(g.abs().max()) for g in grads.values())
        assert smallest >= 1e-6, (name, {n: float(g.abs().max()) for n, g in grads.items() if float(g.abs().max()) < 1e-6})
        src, dst = net.graph.edges()
        o[f"{name}/src"], o[f"{name}/dst"] = src.numpy().astype(np.int32), dst.numpy().astype(np.int32)
        o[f"{name}/edge_features"] = net.edge_features.numpy()
        for k, v in inputs.items():
            o[f"{name}/in_{k}"] = v.numpy()
        o[f"{name}/target"], o[f"{name}/y"], o[f"{name}/loss"] = target.numpy(), y.numpy(), np.float32(loss.item())
        for n, p in net.named_parameters():
            o[f"{name}/p_{n}"], o[f"{name}/g_{n}"] = p.detach().numpy(), grads[n].numpy()
        for k, v in gaps.items():
            o[f"{name}/gap_{k}"] = np.float64(v)
        print(f"{name}: N {net.graph.num_nodes()} E {net.graph.num_edges()} loss {loss.item():.6f}  fp32-vs-fp64 gap: output "
              f"{gaps['y']:.2e}, loss {gaps['loss']:.2e}, gradients <= {worst:.2e}, smallest gradient tensor {smallest:.2e}")
    for kind, arrays in out.items():
        path = os.path.join(HERE, GOLDEN[kind])
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size < 1024 * 1024, (path, size)
        print("wrote", path, len(arrays), "arrays", size // 1024, "KiB")


if __name__ == "__main__":
    main()
