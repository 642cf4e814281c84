#!/usr/bin/env python3
"""Golden vectors for the dlwpbench GraphCastNet, produced by IMPORTING the reference's classes
(src/dlwpbench/models/graphcast/graph_cast_net.py GraphCastNet and utils/graph.py Graph) in this container.

The reference needs DGL, which is not installed here.  DGL is its graph container, not its arithmetic, so this script installs a
stub `dgl` / `dgl.function` written below from DGL's documented behaviour (RESTATED, not executed), the one of make_mgn_golden.py
extended by what this model uses:
* `graph((src, dst))`: a graph on max(id) + 1 nodes; `to_bidirected` adds the reverse of every edge and drops duplicates;
* `heterograph({(srctype, etype, dsttype): ("coo", (src, dst))})`: one edge type between two node types with max(id) + 1 nodes each;
  `srcdata` / `dstdata` are the two node types' feature dicts, `ndata[key]` is a dict by node type;
* `apply_edges(f)` hands f the edge data and the source / destination node data gathered along the edges;
* `update_all(copy_e, sum | mean)` reduces the edge rows onto their DESTINATION nodes (mean: zero for a node without in-edges).
sklearn's NearestNeighbors is the local one.  The icosphere files are written by the project's writer (gc_mesh.write_icospheres):
the reference ships none and its own writer needs pymesh.  `models.graphcast.utils.module.Module` is a stub nn.Module taking
`meta=` (the real one imports fsspec, s3fs and requests, which are absent); everything else is the reference's own file, loaded by
path into synthetic packages.

Stored per case (tests/graphcast_dlwp_ref.py CASES): the three graphs of the reference (src, dst, edge features, the node counts it
assigns positions for, mesh node features), inputs, target, parameters (default initialisation, then ALL perturbed: weights x 3,
every 1-D parameter + 0.2 randn, so that LayerNorm's gamma != 1 and beta != 0 are exercised), output, mse loss and every parameter
gradient from the reference's fp32 run.  The reference is also run in float64; its own fp32 result must sit within 1e-5 (output,
loss) / 5e-5 (every gradient tensor) of that, relative to the float64 tensor's max norm.  The gaps are stored (`gap_*`).  Every
gradient tensor must have a max norm of at least 1e-6.  The stub, like DGL, sizes a node type by the largest id in an edge: the
cases are chosen so that every grid node and every mesh vertex of the last index has an edge (asserted).

    python tests/golden/make_graphcast_dlwp_golden.py
"""
import contextlib
import copy
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from graphcast_dlwp_ref import CASES, GOLDEN, make_inputs, rel_gap  # noqa: E402
from make_convlstm_golden import REF  # noqa: E402
from make_mgn_golden import _load_as  # noqa: E402

from dlwp_benchmark_amd import gc_mesh  # noqa: E402


# ---------------------------------------------------------------- the stub dgl
class _ByType:
    """`ndata` of a graph with two node types: ndata[key] -> {type: tensor}"""

    def __init__(self, g):
        self.g = g

    def __getitem__(self, key):
        return {self.g.srctype: self.g.srcdata[key], self.g.dsttype: self.g.dstdata[key]}


class StubGraph:
    def __init__(self, src, dst, n_src, n_dst, types=None):
        self._src, self._dst, self._ns, self._nd = src.long(), dst.long(), int(n_src), int(n_dst)
        self.edata = {}
        if types is None:
            self.ndata = {}
            self.srcdata = self.dstdata = self.ndata
        else:
            self.srctype, _, self.dsttype = types
            self.srcdata, self.dstdata = {}, {}
            self.ndata = _ByType(self)

    def edges(self):
        return self._src.int(), self._dst.int()

    def num_nodes(self):
        return self._ns

    def num_edges(self):
        return len(self._src)

    def to(self, *args, **kwargs):
        return self

    @contextlib.contextmanager
    def local_scope(self):
        homogeneous = self.srcdata is self.dstdata
        sd, dd, ed = dict(self.srcdata), dict(self.dstdata), dict(self.edata)
        try:
            yield
        finally:
            self.edata = ed
            if homogeneous:
                self.ndata = sd
                self.srcdata = self.dstdata = self.ndata
            else:
                self.srcdata, self.dstdata = sd, dd

    def apply_edges(self, func):
        edges = types.SimpleNamespace(data=self.edata, src={k: v[self._src] for k, v in self.srcdata.items()},
                                      dst={k: v[self._dst] for k, v in self.dstdata.items()})
        self.edata.update(func(edges))

    def update_all(self, message, reduce):
        (kind, field, msg), (how, msg2, out) = message, reduce
        assert kind == "copy_e" and msg == msg2 and how in ("sum", "mean")
        e = self.edata[field]
        acc = torch.zeros((self._nd,) + tuple(e.shape[1:]), dtype=e.dtype).index_add_(0, self._dst, e)
        if how == "mean":
            deg = torch.zeros(self._nd, dtype=e.dtype).index_add_(0, self._dst, torch.ones(len(self._dst), dtype=e.dtype))
            acc = acc / deg.clamp(min=1)[:, None]
        self.dstdata[out] = acc


def _ids(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int64))


def graph(data, idtype=None):
    src, dst = _ids(data[0]), _ids(data[1])
    n = int(max(src.max(), dst.max())) + 1
    return StubGraph(src, dst, n, n)


def heterograph(data, idtype=None):
    (types_, (fmt, (src, dst))), = data.items()
    assert fmt == "coo"
    src, dst = _ids(src), _ids(dst)
    return StubGraph(src, dst, int(src.max()) + 1, int(dst.max()) + 1, types_)


def to_bidirected(g):
    s, d = g.edges()
    pairs = sorted(set(zip(s.tolist(), d.tolist())) | set(zip(d.tolist(), s.tolist())))
    return StubGraph(torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs]), g.num_nodes(), g.num_nodes())


def install_dgl():
    dgl = types.ModuleType("dgl")
    dgl.DGLGraph, dgl.graph, dgl.heterograph, dgl.to_bidirected = StubGraph, graph, heterograph, to_bidirected
    fn = types.ModuleType("dgl.function")
    fn.copy_e = lambda field, msg: ("copy_e", field, msg)
    fn.sum = lambda msg, out: ("sum", msg, out)
    fn.mean = lambda msg, out: ("mean", msg, out)
    dgl.function = fn
    sys.modules["dgl"], sys.modules["dgl.function"] = dgl, fn


def load_reference():
    """(Graph, GraphCastNet) of the reference, its own files loaded into synthetic packages"""
    install_dgl()
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[k]
    base = f"{REF}/dlwpbench/models/graphcast"
    for name in ("models", "models.graphcast", "models.graphcast.gnn_layers", "models.graphcast.utils"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    sys.modules["models.graphcast.gnn_layers"].CuGraphCSC = type("CuGraphCSC", (), {})
    module = types.ModuleType("models.graphcast.utils.module")

    class Module(torch.nn.Module):
        def __init__(self, meta=None):
            super().__init__()
            self.meta = meta

    module.Module = Module
    sys.modules["models.graphcast.utils.module"] = module
    for m in ("meta", "activations", "graph_utils", "graph"):
        _load_as(f"models.graphcast.utils.{m}", f"{base}/utils/{m}.py")
    for m in ("utils", "mesh_graph_mlp", "mesh_edge_block", "mesh_node_block", "embedder", "mesh_graph_encoder", "mesh_graph_decoder"):
        _load_as(f"models.graphcast.gnn_layers.{m}", f"{base}/gnn_layers/{m}.py")
    _load_as("models.graphcast.graph_cast_processor", f"{base}/graph_cast_processor.py")
    net = _load_as("ref_dlwp_graphcast", f"{base}/graph_cast_net.py")
    return sys.modules["models.graphcast.utils.graph"].Graph, net.GraphCastNet


def run(net, inputs, target, dtype):
    net = copy.deepcopy(net).to(dtype)
    inp = {k: v.to(dtype) for k, v in inputs.items()}
    y = net(constants=inp.get("constants"), prescribed=inp.get("prescribed"), prognostic=inp["prognostic"])
    loss = torch.nn.functional.mse_loss(y, target.to(dtype))
    loss.backward()
    return y.detach(), loss.detach(), {n: p.grad for n, p in net.named_parameters()}


def main():
    _, cls = load_reference()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (name, (level, cfg, T)) in enumerate(CASES.items()):
            path = os.path.join(tmp, f"icospheres_l{level}.json")
            gc_mesh.write_icospheres(path, level)
            gen = torch.Generator().manual_seed(41017 + i)
            torch.manual_seed(1618 + i)
            net = cls(meshgraph_path=path, **cfg)
            assert net.graph.max_order == level
            with torch.no_grad():
                for p in net.parameters():
                    if p.dim() == 1:
                        p.add_(0.2 * torch.randn(p.shape, generator=gen))
                    else:
                        p.mul_(3.0)
            inputs, target = make_inputs(cfg, T, gen)
            y, loss, grads = run(net, inputs, target, torch.float32)
            y64, loss64, grads64 = run(net, inputs, target, torch.float64)
            gaps = {"y": rel_gap(y, y64), "loss": rel_gap(loss, loss64)}
            gaps.update({"g_" + n: rel_gap(grads[n], grads64[n]) for n in grads})
            worst = max(v for k, v in gaps.items() if k.startswith("g_"))
            smallest = min(float(g.abs().max()) for g in grads.values())
            print(f"{name}: loss {loss.item():.6f}  fp32-vs-fp64 gap: output {gaps['y']:.2e}, loss {gaps['loss']:.2e}, gradients <= "
                  f"{worst:.2e}, smallest gradient tensor {smallest:.2e}")
            assert gaps["y"] <= 1e-5 and gaps["loss"] <= 1e-5, (name, gaps["y"], gaps["loss"])
            assert worst <= 5e-5, (name, worst)
            assert smallest >= 1e-6, name
            n_grid, n_mesh = cfg["input_height"] * cfg["input_width"], 10 * 4 ** level + 2
            for key, g, ns, nd in (("mesh", net.mesh_graph, n_mesh, n_mesh), ("g2m", net.g2m_graph, n_grid, n_mesh),
                                   ("m2g", net.m2g_graph, n_mesh, n_grid)):
                src, dst = g.edges()
                assert (g._ns, g._nd) == (ns, nd), (name, key, g._ns, g._nd, ns, nd)      # as DGL would size the node types
                out[f"{name}/{key}_src"], out[f"{name}/{key}_dst"] = src.numpy().astype(np.int32), dst.numpy().astype(np.int32)
                out[f"{name}/{key}_edge_features"] = g.edata["x"].numpy()
                out[f"{name}/{key}_num_nodes"] = np.array([len(g.srcdata["pos"]) if "pos" in g.srcdata else len(g.ndata["x"]),
                                                           len(g.dstdata["pos"]) if "pos" in g.dstdata else len(g.ndata["x"])])
            out[f"{name}/mesh_node_features"] = net.mesh_ndata.numpy()
            for k, v in inputs.items():
                out[f"{name}/in_{k}"] = v.numpy()
            out[f"{name}/target"], out[f"{name}/y"], out[f"{name}/loss"] = target.numpy(), y.numpy(), np.float32(loss.item())
            for n, p in net.named_parameters():
                out[f"{name}/p_{n}"], out[f"{name}/g_{n}"] = p.detach().numpy(), grads[n].numpy()
            for k, v in gaps.items():
                out[f"{name}/gap_{k}"] = np.float64(v)
            out[f"{name}/param_order"] = np.array(list(net.state_dict().keys()))
    path = os.path.join(HERE, GOLDEN)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1024 * 1024, (path, size)
    print("wrote", path, len(out), "arrays", size // 1024, "KiB")


if __name__ == "__main__":
    main()
