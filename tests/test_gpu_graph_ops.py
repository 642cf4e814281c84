"""The graph kernels (csrc/graph_ops.hip) through their RAW entry points against float64 torch on the CPU.

Graphs: a hand-made directed graph with N = 37 nodes and E = 101 edges -- node 0 has no in-edge, node 1 no out-edge, (5, 5) is a
self-loop, (2, 3) appears twice, node 7 has in-degree >= 9 -- and the three mesh types of the fixtures.  With B in {1, 3} the row
counts (101, 303, 37, 111, ...) are no multiples of the 64-row tile and cross a tile boundary.

Bars (`rel_gap`: max |difference| relative to the max norm of the float64 array): 1e-5 for outputs, 5e-5 for every gradient --
what the fixture scripts assert of torch's own fp32 run; the MFMA path is exact fp32, so it may differ from torch only by the
order of its sums.  The pure reductions and gathers hold |err| <= deg * 2^-24 * sum |a| per element.  Behind every output and
scratch buffer lie 64 sentinel floats that must come back bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mgn_ref import rel_gap
from test_gpu_conv_ops import Out, bits

pytestmark = pytest.mark.gpu

BAR_OUT, BAR_GRAD = 1e-5, 5e-5
ROWS, EDGE, NODE = 0, 1, 2
MODE_NAME = {ROWS: "rows", EDGE: "edge", NODE: "node"}


def handmade():
    rng = np.random.RandomState(5)
    src = [5, 2, 2] + [10 + i for i in range(9)]          # self-loop, duplicate edge, nine edges into node 7
    dst = [5, 3, 3] + [7] * 9
    while len(src) < 101:
        s, d = int(rng.randint(0, 37)), int(rng.randint(0, 37))
        if s != 1 and d != 0:
            src.append(s)
            dst.append(d)
    src, dst = np.array(src), np.array(dst)
    perm = rng.permutation(101)                           # not sorted by destination: the edge ids matter
    src, dst = src[perm], dst[perm]
    assert 0 not in dst and 1 not in src and (dst == 7).sum() >= 9 and 0 in src and 1 in dst
    return src, dst, 37


@pytest.fixture(scope="module")
def graphs(cuda):
    from dlwp_benchmark_amd import mgn_graph
    from dlwp_benchmark_amd.graph_ops import Graph
    out = {"hand": Graph(*handmade(), device=cuda)}
    for name, args in (("grid", ("grid_2d", 3, 5, True)), ("stencil", ("grid_2d_8stencil", 3, 5, True)), ("delaunay", ("delaunay", 4, 6, True))):
        out[name] = Graph.from_mesh(mgn_graph.build_graph(*args), device=cuda)
    return out


def batched(idx, B, n):
    return (torch.from_numpy(idx.astype(np.int64))[None] + (torch.arange(B) * n)[:, None]).reshape(-1)


def operand64(mode, G, B, x, v, mean):
    """the concatenated operand in float64 (autograd-capable) and the aggregate"""
    src, dst = G._host[0], G._host[1]
    if mode == ROWS:
        return x, None
    srcb, dstb = batched(src, B, G.num_nodes), batched(dst, B, G.num_nodes)
    if mode == EDGE:
        return torch.cat([x, v[srcb], v[dstb]], dim=1), None
    agg = torch.zeros(B * G.num_nodes, x.shape[1], dtype=x.dtype).index_add_(0, dstb, x)
    if mean:
        deg = torch.zeros(B * G.num_nodes, dtype=x.dtype).index_add_(0, dstb, torch.ones(len(dstb), dtype=x.dtype))
        agg = agg / deg.clamp(min=1)[:, None]
    return torch.cat([agg, v], dim=1), agg


def reference(mode, G, B, x, v, params, norm, residual, mean, gy):
    leaf = lambda t: None if t is None else t.double().requires_grad_(True)      # noqa: E731
    x, v, params, norm = leaf(x), leaf(v), [leaf(p) for p in params], ([leaf(t) for t in norm] if norm else None)
    A, agg = operand64(mode, G, B, x, v, mean)
    h, hid = A, []
    nl = len(params) // 2 - 1
    for l in range(nl):
        h = F.relu(F.linear(h, params[2 * l], params[2 * l + 1]))
        hid.append(h)
    z = F.linear(h, params[2 * nl], params[2 * nl + 1])
    y = z
    if norm:
        # LayerNorm from elementary float64 operations, not F.layer_norm: at width 1 the output is beta whatever the input, so every
        # gradient in front of it is exactly zero, and this form gives exactly zero (z - mean is 0, and so is its gradient) where
        # F.layer_norm's backward kernel returns its own rounding noise (~1e-9), against which no relative gap is defined
        c = z - z.mean(dim=1, keepdim=True)
        y = c / torch.sqrt((c * c).mean(dim=1, keepdim=True) + 1e-5) * norm[0] + norm[1]
    if residual:
        y = y + (x if mode == EDGE else v)
    (y * gy.double()).sum().backward()
    g = {"x": x.grad, "v": None if v is None else v.grad}
    g.update({f"p{i}": p.grad for i, p in enumerate(params)})
    if norm:
        g.update(gamma=norm[0].grad, beta=norm[1].grad)
    return y.detach(), [t.detach() for t in hid], (None if agg is None else agg.detach()), g


def raw_run(dev, gen, mode, G, B, x, v, params, norm, residual, mean, gy, twice=False):
    """forward and the whole backward through the raw entry points, every output and scratch buffer in an `Out`;
    returns ({name: cpu tensor}, [Out...])"""
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    s = L.stream()
    N, E = (G.num_nodes, G.num_edges) if mode else (0, 0)
    De, Dv = x.shape[1], (v.shape[1] if v is not None else 0)
    nl = len(params) // 2 - 1
    hidden, out = params[0].shape[0], params[-1].shape[0]
    rows = x.shape[0] if mode != NODE else v.shape[0]
    k0 = params[0].shape[1]
    d = lambda t: None if t is None else t.to(dev).contiguous()      # noqa: E731
    xd, vd, pd, gyd = d(x), d(v), [d(p) for p in params], d(gy)
    nd = [d(t) for t in norm] if norm else None
    outs = {}
    mk = lambda name, shape, zero=False: outs.setdefault(name, Out(shape, dev, gen, zero=zero))      # noqa: E731
    y = mk("y", (rows, out))
    hid = [mk(f"hid{l}", (rows, hidden)) for l in range(nl)]
    a = L.GraphMlpArgs()
    a.mode, a.B, a.N, a.E, a.rows = mode, B, N, E, rows
    a.x, a.v = L.ptr(xd), L.ptr(vd)
    if mode:
        a.src, a.dst, a.in_ptr, a.in_eid = L.ptr(G.src), L.ptr(G.dst), L.ptr(G.in_ptr), L.ptr(G.in_eid)
    a.De, a.Dv, a.hidden, a.out, a.hidden_layers, a.residual, a.mean, a.eps = De, Dv, hidden, out, nl, int(residual), int(mean), 1e-5
    for i in range(nl + 1):
        a.w[i], a.b[i] = L.ptr(pd[2 * i]), L.ptr(pd[2 * i + 1])
    for i, h in enumerate(hid):
        a.hid[i] = L.ptr(h.t)
    a.y = L.ptr(y.t)
    if norm:
        a.gamma, a.beta = L.ptr(nd[0]), L.ptr(nd[1])
        a.xhat, a.rstd = L.ptr(mk("xhat", (rows, out)).t), L.ptr(mk("rstd", (rows,)).t)
    if mode == NODE:
        a.agg = L.ptr(mk("agg", (rows, De)).t)
    L.check(lib.dlwp_graph_mlp_fwd(ctypes.byref(a), s))
    # the same launch without the stores for a backward pass: the output must not depend on them
    y2 = mk("y_nograd", (rows, out))
    a.y, a.xhat, a.rstd, a.agg = L.ptr(y2.t), None, None, None
    for i in range(nl):
        a.hid[i] = None
    L.check(lib.dlwp_graph_mlp_fwd(ctypes.byref(a), s))
    assert torch.equal(bits(y.t), bits(y2.t))

    def ws_of(name, n):
        assert n > 0
        return mk(name, (int(n),))

    pg = [mk(f"g_p{i}", tuple(p.shape), zero=True) for i, p in enumerate(pd)]
    dz = gyd
    if norm:
        gg, gb = mk("g_gamma", (out,), zero=True), mk("g_beta", (out,), zero=True)
        dzo = mk("dz_ln", (rows, out))
        L.check(lib.dlwp_graph_ln_bwd(L.ptr(gyd), L.ptr(outs["xhat"].t), L.ptr(outs["rstd"].t), L.ptr(nd[0]), L.ptr(dzo.t),
                                      L.ptr(ws_of("ws_ln", lib.dlwp_graph_ln_bwd_ws_floats(rows, out)).t), L.ptr(gg.t), L.ptr(gb.t),
                                      rows, out, s))
        dz = dzo.t
    for i in range(nl, 0, -1):                                  # Linears on stored rows: the 1 x 1 convolution's kernels
        cout = out if i == nl else hidden
        ws = torch.empty(lib.dlwp_conv1x1_wgrad_ws_floats(rows, hidden, cout), device=dev)
        L.check(lib.dlwp_conv1x1_wgrad(L.ptr(hid[i - 1].t), L.ptr(dz), L.ptr(ws), L.ptr(pg[2 * i].t), L.ptr(pg[2 * i + 1].t), rows,
                                       hidden, cout, s))
        dh = torch.empty(rows, hidden, device=dev)
        L.check(lib.dlwp_conv1x1_dgrad(L.ptr(dz), L.ptr(pd[2 * i]), L.ptr(dh), rows, hidden, cout, s))
        dz = torch.empty(rows, hidden, device=dev)
        L.check(lib.dlwp_conv3x3_act_bwd(L.ptr(hid[i - 1].t), L.ptr(dh), L.ptr(dz), dh.numel(), 2, s))
    src, dst = (L.ptr(G.src), L.ptr(G.dst)) if mode == EDGE else (None, None)
    x0 = outs["agg"].t if mode == NODE else xd

    def wgrad0():
        L.check(lib.dlwp_graph_wgrad0(mode, L.ptr(x0), L.ptr(vd), src, dst, L.ptr(dz),
                                      L.ptr(ws_of("ws_w0", lib.dlwp_graph_wgrad0_ws_floats(rows, k0, hidden)).t), L.ptr(pg[0].t),
                                      L.ptr(pg[1].t), B, N, E, rows, De, Dv, hidden, s))
    wgrad0()
    res = L.ptr(gyd) if residual else None
    if mode == ROWS:
        L.check(lib.dlwp_graph_dgrad0(mode, L.ptr(dz), L.ptr(pd[0]), None, L.ptr(mk("g_x", (rows, De)).t), None, None, B, N, E, rows,
                                      De, Dv, hidden, s))
    elif mode == EDGE:
        dsrc, ddst = mk("dsrc", (rows, Dv)), mk("ddst", (rows, Dv))
        L.check(lib.dlwp_graph_dgrad0(mode, L.ptr(dz), L.ptr(pd[0]), res, L.ptr(mk("g_x", (rows, De)).t), L.ptr(dsrc.t), L.ptr(ddst.t),
                                      B, N, E, rows, De, Dv, hidden, s))
        L.check(lib.dlwp_graph_gather_sum(L.ptr(dsrc.t), L.ptr(G.out_ptr), L.ptr(G.out_eid), 0, L.ptr(ddst.t), L.ptr(G.in_ptr),
                                          L.ptr(G.in_eid), None, L.ptr(mk("g_v", (B * N, Dv)).t), B, N, E, Dv, s))
    else:
        dagg = mk("dagg", (rows, De))
        L.check(lib.dlwp_graph_dgrad0(mode, L.ptr(dz), L.ptr(pd[0]), res, L.ptr(dagg.t), L.ptr(mk("g_v", (rows, Dv)).t), None, B, N, E,
                                      rows, De, Dv, hidden, s))
        L.check(lib.dlwp_graph_edge_gather(L.ptr(dagg.t), L.ptr(G.dst), L.ptr(G.in_ptr) if mean else None, None,
                                           L.ptr(mk("g_x", (B * E, De)).t), B, N, E, De, s))
    torch.cuda.synchronize()
    got = {k: o.t.detach().cpu().clone() for k, o in outs.items()}
    if twice:           # a second weight-gradient pass into the same slots exactly doubles them
        first = [o.t.clone() for o in pg] + ([gg.t.clone(), gb.t.clone()] if norm else [])
        if norm:
            L.check(lib.dlwp_graph_ln_bwd(L.ptr(gyd), L.ptr(outs["xhat"].t), L.ptr(outs["rstd"].t), L.ptr(nd[0]), L.ptr(outs["dz_ln"].t),
                                          L.ptr(outs["ws_ln"].t), L.ptr(gg.t), L.ptr(gb.t), rows, out, s))
        wgrad0()
        torch.cuda.synchronize()
        assert torch.equal(bits(pg[0].t), bits(2 * first[0])) and torch.equal(bits(pg[1].t), bits(2 * first[1]))
        if norm:
            assert torch.equal(bits(gg.t), bits(2 * first[-2])) and torch.equal(bits(gb.t), bits(2 * first[-1]))
    for k, o in outs.items():
        assert o.sentinels_intact(), f"{k}: the kernel wrote behind its buffer"
    return got


# (in, hidden, out, hidden layers, B, LayerNorm, mean, residual where the mode allows it, graph)
SHAPES = [
    (1, 5, 1, 1, 1, True, False, True, "hand"),
    (2, 7, 6, 2, 3, True, True, False, "hand"),
    (3, 33, 34, 3, 1, True, False, False, "stencil"),
    (34, 34, 34, 2, 3, True, True, True, "hand"),
    (34, 34, 34, 1, 1, True, False, False, "delaunay"),
    (116, 116, 116, 2, 1, True, False, True, "hand"),
    (128, 128, 128, 3, 3, True, True, True, "hand"),
    (6, 4, 1, 1, 3, False, False, False, "grid"),
    (32, 32, 32, 2, 3, True, False, True, "grid"),
    # edge mode: 707 rows = 12 row tiles (the last with 3 rows) for S = 11 splits of the first Linear's weight gradient
    # (K0 = 384: 25 x 2 blocks), so a workgroup walks two tiles and prefetches tile t + S; in every other case S is the tile count
    (128, 128, 128, 1, 7, True, False, True, "hand"),
]


def make_case(mode, G, shape, seed):
    cin, hidden, out, nl, B, use_norm, mean, residual, _ = shape
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    De = Dv = cin
    if mode == ROWS:
        x, v, k0, residual = rnd(B * G.num_edges, cin), None, cin, False
    else:
        x, v = rnd(B * G.num_edges, De), rnd(B * G.num_nodes, Dv)
        k0 = De + 2 * Dv if mode == EDGE else De + Dv
        residual = residual and out == cin
    rows = x.shape[0] if mode != NODE else v.shape[0]
    dims = [k0] + [hidden] * nl + [out]
    params = []
    for i in range(nl + 1):
        params += [1.5 * rnd(dims[i + 1], dims[i]) / dims[i] ** 0.5, 0.3 * rnd(dims[i + 1])]
    norm = [1.0 + 0.3 * rnd(out), 0.3 * rnd(out)] if use_norm else None
    return gen, B, x, v, params, norm, residual, mean and mode == NODE, rnd(rows, out)


@pytest.mark.parametrize("mode", [ROWS, EDGE, NODE], ids=["rows", "edge", "node"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}-{s[1]}-{s[2]}_L{s[3]}_B{s[4]}_{s[8]}" for s in SHAPES])
def test_forward_and_every_gradient(cuda, graphs, mode, shape):
    G = graphs[shape[8]]
    gen, B, x, v, params, norm, residual, mean, gy = make_case(mode, G, shape, seed=100 * mode + sum(shape[:5]))
    y64, hid64, agg64, g64 = reference(mode, G, B, x, v, params, norm, residual, mean, gy)
    got = raw_run(cuda, gen, mode, G, B, x, v, params, norm, residual, mean, gy, twice=True)
    again = raw_run(cuda, gen, mode, G, B, x, v, params, norm, residual, mean, gy)
    for k in got:                                              # every launch repeated on the same operands: bit-identical
        if not k.startswith("ws_"):
            assert torch.equal(bits(got[k]), bits(again[k])), f"{k} differs between two runs"
    gaps = {"y": rel_gap(got["y"], y64)}
    gaps.update({f"hid{l}": rel_gap(got[f"hid{l}"], h) for l, h in enumerate(hid64)})
    if agg64 is not None:
        gaps["agg"] = rel_gap(got["agg"], agg64)
    print(f"{MODE_NAME[mode]} {shape}: outputs " + ", ".join(f"{k} {g:.1e}" for k, g in gaps.items()))
    for k, g in gaps.items():
        assert g <= BAR_OUT, (k, g)
    ggaps = {k: rel_gap(got["g_" + k], ref) for k, ref in g64.items() if ref is not None}
    print("  gradients " + ", ".join(f"{k} {g:.1e}" for k, g in ggaps.items()))
    assert set(ggaps) == {"x"} | ({"v"} if mode else set()) | {f"p{i}" for i in range(len(params))} | ({"gamma", "beta"} if norm else set())
    for k, g in ggaps.items():
        assert g <= BAR_GRAD, (k, g)


@pytest.mark.parametrize("name,B,C", [("hand", 1, 1), ("hand", 3, 34), ("stencil", 3, 128), ("delaunay", 1, 116)])
def test_reductions_and_gathers_alone(cuda, graphs, name, B, C):
    """|err| <= deg * 2^-24 * sum |a| per element (a sum of deg fp32 numbers in any order), and exact for the gather"""
    from dlwp_benchmark_amd import lib as L
    lib, s, G = L.load(), L.stream(), graphs[name]
    N, E = G.num_nodes, G.num_edges
    gen = torch.Generator().manual_seed(B * 1000 + C)
    e1, e2 = torch.randn(B * E, C, generator=gen), torch.randn(B * E, C, generator=gen)
    add = torch.randn(B * N, C, generator=gen)
    src, dst = batched(G._host[0], B, N), batched(G._host[1], B, N)
    deg_in = torch.zeros(B * N, dtype=torch.float64).index_add_(0, dst, torch.ones(B * E, dtype=torch.float64))
    deg_out = torch.zeros(B * N, dtype=torch.float64).index_add_(0, src, torch.ones(B * E, dtype=torch.float64))
    isum = lambda idx, t: torch.zeros(B * N, C, dtype=torch.float64).index_add_(0, idx, t.double())      # noqa: E731
    d = lambda t: t.to(cuda)      # noqa: E731
    e1d, e2d, addd = d(e1), d(e2), d(add)
    # forward aggregation, sum and mean
    for mean in (0, 1):
        o = Out((B * N, C), cuda, gen)
        L.check(lib.dlwp_graph_gather_sum(L.ptr(e1d), L.ptr(G.in_ptr), L.ptr(G.in_eid), mean, None, None, None, None, L.ptr(o.t), B, N, E, C, s))
        ref, mag = isum(dst, e1), isum(dst, e1.abs())
        bound = deg_in[:, None] * 2.0 ** -24 * mag
        if mean:
            ref, bound = ref / deg_in.clamp(min=1)[:, None], bound / deg_in.clamp(min=1)[:, None] + 2.0 ** -24 * ref.abs() / deg_in.clamp(min=1)[:, None]
        err = (o.t.cpu().double() - ref).abs()
        assert bool((err <= bound).all()), float((err - bound).max())
        assert o.sentinels_intact()
        assert bool((o.t.cpu()[deg_in == 0] == 0).all())      # a node without in-edges gets zeros
    # dv of an edge block: out-edges of the first array + in-edges of the second (+ add)
    for with_add in (False, True):
        o = Out((B * N, C), cuda, gen)
        L.check(lib.dlwp_graph_gather_sum(L.ptr(e1d), L.ptr(G.out_ptr), L.ptr(G.out_eid), 0, L.ptr(e2d), L.ptr(G.in_ptr), L.ptr(G.in_eid),
                                          L.ptr(addd) if with_add else None, L.ptr(o.t), B, N, E, C, s))
        ref = isum(src, e1) + isum(dst, e2) + (add.double() if with_add else 0)
        mag = isum(src, e1.abs()) + isum(dst, e2.abs()) + (add.abs().double() if with_add else 0)
        bound = (deg_in + deg_out + 2)[:, None] * 2.0 ** -24 * mag
        err = (o.t.cpu().double() - ref).abs()
        assert bool((err <= bound).all()), float((err - bound).max())
        assert o.sentinels_intact()
        o2 = Out((B * N, C), cuda, gen)
        L.check(lib.dlwp_graph_gather_sum(L.ptr(e1d), L.ptr(G.out_ptr), L.ptr(G.out_eid), 0, L.ptr(e2d), L.ptr(G.in_ptr), L.ptr(G.in_eid),
                                          L.ptr(addd) if with_add else None, L.ptr(o2.t), B, N, E, C, s))
        assert torch.equal(bits(o.t), bits(o2.t))
    # the gather back to the edges: a copy (exact), or one correctly rounded division
    nodes = torch.randn(B * N, C, generator=gen)
    nd_ = d(nodes)
    o = Out((B * E, C), cuda, gen)
    L.check(lib.dlwp_graph_edge_gather(L.ptr(nd_), L.ptr(G.dst), None, None, L.ptr(o.t), B, N, E, C, s))
    assert torch.equal(bits(o.t.cpu()), bits(nodes[dst])) and o.sentinels_intact()
    o = Out((B * E, C), cuda, gen)
    edge_add = torch.randn(B * E, C, generator=gen)
    L.check(lib.dlwp_graph_edge_gather(L.ptr(nd_), L.ptr(G.dst), L.ptr(G.in_ptr), L.ptr(d(edge_add)), L.ptr(o.t), B, N, E, C, s))
    ref = edge_add + nodes[dst] / deg_in[dst].float()[:, None]
    assert torch.equal(bits(o.t.cpu()), bits(ref)) and o.sentinels_intact()


def test_kernel_names(cuda, graphs):
    from dlwp_benchmark_amd import graph_ops, lib as L
    G = graphs["hand"]
    gen = torch.Generator().manual_seed(3)
    lin = lambda o, i: [torch.nn.Parameter(torch.randn(o, i, generator=gen).to(cuda) / i ** 0.5), torch.nn.Parameter(torch.zeros(o, device=cuda))]      # noqa: E731
    norm = [torch.nn.Parameter(torch.ones(8, device=cuda)), torch.nn.Parameter(torch.zeros(8, device=cuda))]
    e = torch.randn(2 * G.num_edges, 8, generator=gen).to(cuda).requires_grad_(True)
    v = torch.randn(2 * G.num_nodes, 8, generator=gen).to(cuda).requires_grad_(True)
    with L.kernel_accounting() as acc:
        x = graph_ops.graph_mlp(v, lin(8, 8) + lin(8, 8), norm)
        e2 = graph_ops.edge_block(e, x, G, lin(8, 24) + lin(8, 8), norm)
        v2 = graph_ops.node_block(e2, x, G, lin(8, 16) + lin(8, 8), norm, "mean")
        (v2.sum() + e2.sum()).backward()
        graph_ops.aggregate(e, G)
    names = {r["name"] for r in acc.rows}
    print(sorted(names))
    assert {n for n in names if n.startswith("graph_")} == {
        "graph_mlp_rows", "graph_mlp_edge", "graph_mlp_node", "graph_ln_bwd", "graph_ln_bwd_fold", "graph_wgrad0_rows",
        "graph_wgrad0_edge", "graph_wgrad0_node", "graph_wgrad0_fold", "graph_dgrad0_rows", "graph_dgrad0_edge", "graph_dgrad0_node",
        "graph_gather_sum", "graph_edge_gather"}
    assert {"conv1x1", "pixel_wgrad", "pixel_wgrad_fold"} <= names      # the Linears on stored rows
    calls = {r["name"]: r["calls"] for r in acc.rows}
    assert calls["graph_mlp_rows"] == calls["graph_mlp_edge"] == calls["graph_mlp_node"] == 1      # one launch per MLP


def test_operators_same_sample_three_times_and_no_grad(cuda, graphs):
    """B = 3 with the same sample three times: the three output blocks are bit-identical; under no_grad the operators give the
    same bits and keep nothing"""
    from dlwp_benchmark_amd import graph_ops
    G = graphs["hand"]
    gen = torch.Generator().manual_seed(11)
    lin = lambda o, i: [(torch.randn(o, i, generator=gen) / i ** 0.5).to(cuda).requires_grad_(True), torch.randn(o, generator=gen).to(cuda).requires_grad_(True)]      # noqa: E731
    norm = [torch.randn(34, generator=gen).to(cuda).requires_grad_(True), torch.randn(34, generator=gen).to(cuda).requires_grad_(True)]
    e1, v1 = torch.randn(G.num_edges, 34, generator=gen).to(cuda), torch.randn(G.num_nodes, 34, generator=gen).to(cuda)
    e, v = e1.repeat(3, 1), v1.repeat(3, 1)
    pe, pn = lin(34, 102) + lin(34, 34) + lin(34, 34), lin(34, 68) + lin(34, 34)
    e2 = graph_ops.edge_block(e, v, G, pe, norm)
    v2 = graph_ops.node_block(e2, v, G, pn, norm, "mean")
    assert e2.requires_grad and v2.requires_grad
    for t in (e2, v2):
        blocks = t.detach().view(3, -1, 34)
        assert torch.equal(bits(blocks[0]), bits(blocks[1])) and torch.equal(bits(blocks[0]), bits(blocks[2]))
    with torch.no_grad():
        e3 = graph_ops.edge_block(e, v, G, pe, norm)
        v3 = graph_ops.node_block(e3, v, G, pn, norm, "mean")
    assert not e3.requires_grad and e3.grad_fn is None
    assert torch.equal(bits(e2), bits(e3)) and torch.equal(bits(v2), bits(v3))
    # one sample alone gives the first block
    with torch.no_grad():
        e4 = graph_ops.edge_block(e1, v1, G, pe, norm)
    assert torch.equal(bits(e4), bits(e3[:G.num_edges]))


def test_no_grad_stores_nothing_for_a_backward_pass(cuda, graphs):
    """Under torch.no_grad() the launch gets no buffer for hidden rows, normalised rows, 1/sigma or agg, although the parameters
    still report needs_input_grad: the bytes the accounting derives from the launch's own arguments drop by exactly the stored
    rows ((L * hidden + out) floats per row), and the call leaves nothing allocated but its output."""
    from dlwp_benchmark_amd import graph_ops, lib as L
    G = graphs["hand"]
    gen = torch.Generator().manual_seed(17)
    lin = lambda o, i: [torch.nn.Parameter((torch.randn(o, i, generator=gen) / i ** 0.5).to(cuda)), torch.nn.Parameter(torch.zeros(o, device=cuda))]      # noqa: E731
    norm = [torch.nn.Parameter(torch.ones(34, device=cuda)), torch.nn.Parameter(torch.zeros(34, device=cuda))]
    e, v = torch.randn(2 * G.num_edges, 34, generator=gen).to(cuda), torch.randn(2 * G.num_nodes, 34, generator=gen).to(cuda)
    pr, pe, pn = lin(20, 34) + lin(20, 20) + lin(34, 20), lin(34, 102) + lin(34, 34), lin(34, 68) + lin(34, 34) + lin(34, 34) + lin(34, 34)
    # name -> (call, rows, floats per row stored for a backward pass and counted by the accounting: L * hidden + out)
    calls = {"graph_mlp_rows": (lambda: graph_ops.graph_mlp(v, pr, norm), 2 * G.num_nodes, 2 * 20 + 34),
             "graph_mlp_edge": (lambda: graph_ops.edge_block(e, v, G, pe, norm), 2 * G.num_edges, 34 + 34),
             "graph_mlp_node": (lambda: graph_ops.node_block(e, v, G, pn, norm, "mean"), 2 * G.num_nodes, 3 * 34 + 34)}
    for name, (fn, rows, stored) in calls.items():
        nbytes, held = {}, {}
        for mode in ("grad", "no_grad"):
            with (torch.no_grad() if mode == "no_grad" else torch.enable_grad()):
                with L.kernel_accounting() as acc:
                    y = fn()
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated()
                y2 = fn()
                torch.cuda.synchronize()
                held[mode] = torch.cuda.memory_allocated() - before
            assert y.requires_grad == (mode == "grad") and torch.equal(bits(y), bits(y2))
            nbytes[mode] = {r["name"]: r["bytes"] for r in acc.rows}[name]
            del y, y2
        print(name, nbytes, held)
        assert nbytes["grad"] - nbytes["no_grad"] == 4.0 * rows * stored, (name, nbytes)
        # the allocator rounds every block up to 512 bytes: the output alone under no_grad, the stored rows on top in grad mode
        assert 4 * rows * 34 <= held["no_grad"] < 4 * rows * 34 + 512, (name, held)
        assert held["grad"] >= held["no_grad"] + 4 * rows * stored, (name, held)
