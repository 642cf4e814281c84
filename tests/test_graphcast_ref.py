"""GraphCastNS on a CPU-only box: the numpy n-hop mesh (mgn_graph.build_nhop_grid) against the reference's graphs, the
plain-torch helper (tests/graphcast_ref.py) against the golden vectors of the reference's own class
(tests/golden/make_graphcast_ns_golden.py), the model class's interface and refusals, and the host-side argument validation of
what the SiLU path adds to the dlwp_graph_* entry points.

Bounds (`rel_gap`: max |difference| relative to the max norm of the reference array), the rule of tests/test_mgn_ref.py:
* helper in float64 vs the golden fp32 arrays: twice the gap the fixture stores for that array (a floor of 1e-12 for an array
  whose stored gap is exactly zero);
* helper in fp32: 1e-5 for output and loss, 5e-5 for every gradient tensor -- what the golden script asserts of the reference.
"""
import ctypes
import json
import os
import time

import numpy as np
import pytest
import torch

from graphcast_ref import CASES, GOLDEN_OF, build_mesh, grid_of, load_case, rel_gap, run_case
from test_mgn_ref import E_INVALID, E_UNSUPPORTED, FAKE, _sorted_rows, err, h, mlp_args  # noqa: F401  (h: the library fixture)

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "shipped_graphcast_model_configs.json")) as f:
    SHIPPED = json.load(f)


def golden(name):
    return np.load(os.path.join(HERE, "golden", GOLDEN_OF[name]))


@pytest.mark.parametrize("name", list(CASES))
def test_nhop_mesh_gives_the_reference_edges_and_features(name):
    """the same edge SET with the same features per (src, dst) pair (compared by their bits); the edge order is ours"""
    from dlwp_benchmark_amd import mgn_graph
    cfg = CASES[name][0]
    rsrc, rdst, rfeat = load_case(golden(name), name)[7]
    H, W = grid_of(cfg)
    m = mgn_graph.build_nhop_grid(H, W, cfg["nhop_neighbors"])
    assert m.src.dtype == m.dst.dtype == np.int32 and m.edge_features.dtype == np.float32
    assert m.num_nodes == H * W and m.edge_features.shape == (len(m.src), 3) and len(m.src) == len(rsrc)
    assert np.array_equal(_sorted_rows(m.src, m.dst, m.edge_features), _sorted_rows(rsrc.numpy(), rdst.numpy(), rfeat.numpy()))
    pairs = set(zip(m.src.tolist(), m.dst.tolist()))
    assert len(pairs) == len(m.src) and all((d, s) in pairs for s, d in pairs)      # both directions, no duplicates
    assert (np.diff(m.dst) >= 0).all()
    mgn_graph.check_csr(m.src, m.dst, m.num_nodes, m.in_ptr, m.in_eid, m.out_ptr, m.out_eid)


@pytest.mark.parametrize("H,W,nhop,N,E", [(4, 4, [2], 16, 72), (6, 6, [2], 36, 180), (8, 8, [2, 4], 64, 336), (64, 64, [2], 4096, 20480)])
def test_nhop_mesh_sizes(H, W, nhop, N, E):
    """the sizes of the reference's graphs (its class on a stub dgl); 64 x 64 is built vectorised, well under a second"""
    from dlwp_benchmark_amd import mgn_graph
    t0 = time.perf_counter()
    m = mgn_graph.build_nhop_grid(H, W, nhop)
    assert time.perf_counter() - t0 < 1.0
    assert (m.num_nodes, len(m.src)) == (N, E)
    assert set(np.unique(m.edge_features[:, :2]).tolist()) <= {-1.0, 0.0, 1.0}
    assert set(np.unique(m.edge_features[:, 2]).tolist()) == {d / max(nhop) for d in [1] + nhop}


def test_nhop_mesh_oddities_and_refusals():
    from dlwp_benchmark_amd import mgn_graph
    # 4 x 4, nhop 2: height - 1 - max(nhop) = 1, so a difference of +1 becomes -1 (first rule) and then +1 again (third rule):
    # every direction component is 0 or +1, never -1
    m = mgn_graph.build_nhop_grid(4, 4, [2])
    assert set(np.unique(m.edge_features[:, :2]).tolist()) == {0.0, 1.0}
    # coordinates are (u // HEIGHT, u % width): on 4 x 8 node 4 = grid point (0, 4) is read as (1, 4), so from node 0 the difference
    # is (1, 4), not (0, 4); >= height - 1 - 2 = 1 turns both into -1, <= -1 both into +1.  dist is on the true grid: 4 steps / 2
    assert mgn_graph.nhop_edge_features([0], [4], 4, 8, [2]).tolist() == [[1.0, 1.0, 2.0]]
    # only listed nodes start shortcuts, and the cutoff shrinks with max(i, j) % nhop: on 8 x 8 with [2, 4] node (2, 2) reaches
    # 2 hops but not 4, node (4, 4) both (4 hops is the antipode: one node per axis)
    m = mgn_graph.build_nhop_grid(8, 8, [2, 4])
    out = lambda i, j: {(int(d) // 8, int(d) % 8) for d in m.dst[m.src == i * 8 + j]}      # noqa: E731
    assert {(2, 6), (6, 2)} & out(2, 2) == set() and {(2, 4), (2, 0), (4, 2), (0, 2)} <= out(2, 2)
    assert {(4, 0), (0, 4), (4, 2), (4, 6), (2, 4), (6, 4)} <= out(4, 4)
    assert out(1, 1) == {(0, 1), (2, 1), (1, 0), (1, 2)}
    assert len(mgn_graph.build_nhop_grid(6, 6, (2, 2)).src) == 180
    with pytest.raises(ValueError, match="3 x 3"):
        mgn_graph.build_nhop_grid(2, 6, [2])
    with pytest.raises(ValueError, match="positive"):
        mgn_graph.build_nhop_grid(6, 6, [0, 2])
    with pytest.raises(ValueError, match="positive"):
        mgn_graph.build_nhop_grid(6, 6, [])


@pytest.mark.parametrize("name", list(CASES))
def test_helper_matches_the_reference(name):
    """the helper on ITS OWN mesh (build_nhop_grid, another edge order than the reference's) against the reference's arrays"""
    cfg, (B, T), roll = CASES[name]
    params, x, target, y, loss, grads, gaps, _ = load_case(golden(name), name)
    assert x.shape[:2] == (B, T) and x.shape[-2:] == grid_of(cfg)
    assert set(grads) == set(params) and len(params) >= 30
    for dtype, bound in ((torch.float64, None), (torch.float32, (1e-5, 5e-5))):
        hy, hloss, hg = run_case(params, x, target, dtype, cfg, roll)
        assert hy.shape == y.shape
        lim = lambda key, i: max(2.0 * gaps[key], 1e-12) if bound is None else bound[i]      # noqa: E731
        g = rel_gap(hy, y)
        print(f"{name} {dtype}: output {g:.2e} (<= {lim('y', 0):.2e})")
        assert g <= lim("y", 0)
        g = rel_gap(hloss, loss)
        assert g <= lim("loss", 0), (g, lim("loss", 0))
        for k in grads:
            g = rel_gap(hg[k], grads[k])
            assert g <= lim("g_" + k, 1), (k, g, lim("g_" + k, 1))


def test_the_relu_case_differs_from_the_silu_case():
    """the two fixtures that differ in activation_fn alone are told apart by the helper: each with the other's activation misses"""
    name = "gc_6x6_hop2_c2_w8_relu"
    cfg, _, roll = CASES[name]
    params, x, target, y, *_ = load_case(golden(name), name)
    wrong = run_case(params, x, target, torch.float64, dict(cfg, activation_fn="silu"), roll)[0]
    assert rel_gap(wrong, y) > 1e-3


def test_registry_exports_graphcast():
    from dlwp_benchmark_amd import nsbench
    assert "GraphCastNetNS" in nsbench.__all__ and nsbench.GraphCastNetNS.__name__ == "GraphCastNetNS"


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_built_model_has_the_golden_keys_and_shapes(name):
    from dlwp_benchmark_amd import nsbench
    cfg = CASES[name][0]
    params = load_case(golden(name), name)[0]
    net = nsbench.GraphCastNetNS(type="GraphCastNetNS", name="gc", partition_size=1, partition_group_name=None, device="cpu", **cfg)
    sd = net.state_dict()
    assert list(sd) == list(params)                      # same keys in the same order: node_encoder, edge_encoder, processor, node_decoder
    assert [k.split(".")[0] for k in sd][0] == "node_encoder" and list(sd)[-1].startswith("node_decoder.")
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in params.items()}
    net.load_state_dict(params, strict=True)
    assert all(torch.equal(net.state_dict()[k], params[k]) for k in params)
    src, dst, feats = build_mesh(cfg)                    # the model's mesh is the helper's
    assert net.graph.num_edges == len(src) and torch.equal(net._edge_features, feats)
    assert (net.height, net.width) == grid_of(cfg)


def test_shipped_config_has_the_reference_keys_and_shapes():
    from dlwp_benchmark_amd import nsbench
    entry = SHIPPED["nsbench/graphcast_ns"]
    kw = dict(entry["kwargs"], input_height=6, input_width=6)         # the parameters do not depend on the grid
    net = getattr(nsbench, kw["type"])(**kw)
    expect = {k: tuple(shape) for k, shape in entry["parameters"]}      # the reference's own class, recorded
    sd = net.state_dict()
    assert list(sd) == list(expect) and len(expect) >= 40
    assert {k: tuple(v.shape) for k, v in sd.items()} == expect
    assert expect["node_encoder.model.0.weight"] == (32, 10) and expect["edge_encoder.model.0.weight"] == (32, 3)
    net.load_state_dict({k: torch.zeros(s) for k, s in expect.items()}, strict=True)


def test_refusals_and_semantics():
    from dlwp_benchmark_amd import lib as L, nsbench
    make = lambda **kw: nsbench.GraphCastNetNS(**dict(dict(input_height=6, input_width=6, downscale_factor=1, processor_layers=1,      # noqa: E731
                                                           hidden_dim_processor=8), **kw))
    assert make().processor.processor_layers[0].edge_mlp.act == "silu"
    assert make(activation_fn="SiLU").node_decoder.act == "silu" and make(activation_fn="ReLU").edge_encoder.act == "relu"
    for name in ("gelu", "tanh", "leaky_relu", "identity", "stan"):
        with pytest.raises(NotImplementedError, match=name):
            make(activation_fn=name)
    with pytest.raises(KeyError, match="swish"):
        make(activation_fn="swish")
    with pytest.raises(NotImplementedError, match="norm_type"):
        make(norm_type="TELayerNorm")
    make(recompute_activation=True)
    make(recompute_activation=False)
    with pytest.raises(NotImplementedError, match="do_concat_trick"):
        make(do_concat_trick=True)
    with pytest.raises(NotImplementedError, match="checkpoint"):
        make(num_processor_checkpoint_segments=1)
    with pytest.raises(NotImplementedError, match="partition_size"):
        make(partition_size=2)
    for k in ("hidden_dim_processor", "hidden_dim_node_encoder", "hidden_dim_edge_encoder", "hidden_dim_node_decoder"):
        with pytest.raises(NotImplementedError, match="128"):
            make(**{k: 129})
        make(**{k: 128})
    for k in ("num_layers_node_processor", "num_layers_edge_processor", "num_layers_node_encoder", "num_layers_edge_encoder",
              "num_layers_node_decoder"):
        with pytest.raises(NotImplementedError, match="hidden layers"):
            make(**{k: 4})
        make(**{k: 3})
    with pytest.raises(NotImplementedError, match="128"):
        make(input_dim_nodes=13, output_dim=13, context_size=10)      # the node encoder's input is 130 wide
    with pytest.raises(ValueError, match="aggregation"):
        make(aggregation="max")
    with pytest.raises(ValueError, match="input_dim_edges"):
        make(input_dim_edges=2)
    with pytest.raises(ValueError, match="output_dim"):
        make(input_dim_nodes=2, output_dim=1)
    # downscale_factor=None is 1; the mesh and the input check use the downscaled grid
    assert (make(downscale_factor=None).height, make(downscale_factor=None).width) == (6, 6)
    net = make(input_height=12, input_width=16, downscale_factor=2, nhop_neighbors=[2, 4])
    assert (net.height, net.width, net.graph.num_nodes) == (6, 8, 48)
    with pytest.raises(ValueError, match="6 x 8"):
        net(torch.zeros(1, 2, 1, 12, 16), teacher_forcing_steps=1)
    with pytest.raises(L.DlwpError):                                    # no CPU path: refused, never computed on by torch
        net(torch.zeros(1, 2, 1, 6, 8), teacher_forcing_steps=1)


def test_operators_take_relu_or_silu_only():
    from dlwp_benchmark_amd import graph_ops
    lin = lambda o, i: [torch.zeros(o, i), torch.zeros(o)]      # noqa: E731
    g = graph_ops.Graph([0, 1], [1, 0], 2)
    assert graph_ops.ACTIVATIONS == ("relu", "silu")
    with pytest.raises(ValueError, match="'relu' or 'silu'"):
        graph_ops.graph_mlp(torch.zeros(5, 3), lin(4, 3) + lin(2, 4), act="tanh")
    with pytest.raises(ValueError, match="'relu' or 'silu'"):
        graph_ops.edge_block(torch.zeros(2, 4), torch.zeros(2, 4), g, lin(4, 12) + lin(4, 4), act="SiLU")
    with pytest.raises(ValueError, match="'relu' or 'silu'"):
        graph_ops.node_block(torch.zeros(2, 4), torch.zeros(2, 4), g, lin(4, 8) + lin(4, 4), act=None)


def test_silu_entry_points_reject_bad_arguments(h):
    from dlwp_benchmark_amd import lib as L
    # the new fields are the LAST of the struct: the earlier layout is a prefix of it
    names = [f[0] for f in L.GraphMlpArgs._fields_]
    assert names[-2:] == ["act", "der"] and names[-3] == "agg"
    fwd = lambda **kw: h.dlwp_graph_mlp_fwd(ctypes.byref(mlp_args(**kw)), None)      # noqa: E731
    assert fwd(act=2) == E_INVALID and "relu (0)" in err(h) and "silu (1)" in err(h)
    assert fwd(act=-1) == E_INVALID and "act" in err(h)
    a = mlp_args(act=0)
    a.der[0] = FAKE
    assert h.dlwp_graph_mlp_fwd(ctypes.byref(a), None) == E_INVALID and "derivative rows 0" in err(h)      # ReLU stores none
    a = mlp_args(act=1)          # two hidden layers
    a.der[2] = FAKE
    assert h.dlwp_graph_mlp_fwd(ctypes.byref(a), None) == E_INVALID and "derivative rows 2" in err(h)
    # dlwp_graph_dgrad_mul: dz, w, mul (nullable), out, rows, in, out_width, stream
    dm = h.dlwp_graph_dgrad_mul
    assert dm(None, FAKE, FAKE, FAKE, 70, 8, 4, None) == E_INVALID and "graph_dgrad_mul" in err(h) and "NULL" in err(h)
    assert dm(FAKE, None, None, FAKE, 70, 8, 4, None) == E_INVALID and dm(FAKE, FAKE, None, None, 70, 8, 4, None) == E_INVALID
    assert dm(FAKE, FAKE, FAKE, FAKE, 0, 8, 4, None) == E_INVALID and "bad shape" in err(h)
    assert dm(FAKE, FAKE, FAKE, FAKE, 1 << 31, 8, 4, None) == E_UNSUPPORTED and "2^31" in err(h)
    assert dm(FAKE, FAKE, FAKE, FAKE, 70, 129, 4, None) == E_UNSUPPORTED and "1..128" in err(h)
    assert dm(FAKE, FAKE, FAKE, FAKE, 70, 8, 0, None) == E_UNSUPPORTED and "1..128" in err(h)
