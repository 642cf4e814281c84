"""The backward entry points of the two graph families (csrc/graph_bwd.hip: dlwp_graph_* at widths 1..128, dlwp_graph_wide_* at
1..512) launch ONE kernel set, so on the same operands they must give the same BITS: every comparison here is `torch.equal`.  The
families differ in what must not show: the fused family's input gradient runs on 64-column blocks and the wide one's on 128, a
fused-family graph is the wide family's with Ns == Nd, and the two-list node sum is two one-list launches, the second adding onto
the first.

Inputs: a hand-written graph of 8 nodes and 18 edges in no order (node 0 has no in-edge, node 7 no out-edge; a self-loop, a duplicate
edge), B = 2 (36 edge rows, 16 node rows), wrapped as `Graph` and as `BipartiteGraph` with Ns == Nd; the rows mode on 130 rows (three
64-row tiles with a tail of 2).  Widths (De, Dv, hidden) = (5, 3, 8) and (40, 20, 24): the second gives the edge mode K0 = 80 (past
one 64-column block, 16-chunk tails) and the node mode K0 = 60.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, EDGE, NODE = 0, 1, 2
N_NODES, B, ROWS_R = 8, 2, 130
SRC = np.array([3, 0, 5, 1, 2, 0, 6, 4, 1, 3, 2, 5, 0, 4, 6, 2, 3, 1])
DST = np.array([3, 2, 7, 4, 5, 1, 1, 7, 2, 6, 3, 6, 3, 5, 7, 7, 4, 2])
WIDTHS = [(5, 3, 8), (40, 20, 24)]


@pytest.fixture(scope="module")
def graphs(cuda):
    from dlwp_benchmark_amd.graph_ops import BipartiteGraph, Graph
    assert len(SRC) <= 20 and 0 not in DST and 7 not in SRC
    return Graph(SRC, DST, N_NODES, device=cuda), BipartiteGraph(SRC, DST, N_NODES, N_NODES, device=cuda)


def rand(cuda, seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(cuda)


def shape_of(mode, De, Dv):
    """(rows, K0, the widths of the three parts of the input gradient)"""
    E = len(SRC)
    if mode == ROWS:
        return ROWS_R, De, (De,)
    if mode == EDGE:
        return B * E, De + 2 * Dv, (De, Dv, Dv)
    return B * N_NODES, De + Dv, (De, Dv)


def wide_op(mode, Gw, rows, x, v):
    from dlwp_benchmark_amd import graph_ops as go
    return go._operand(mode, Gw, 1 if mode == ROWS else B, rows, x, v, v)


def fused_shape(mode):
    """(B, N, E) as the fused family's entry points take them"""
    return (1, 0, 0) if mode == ROWS else (B, N_NODES, len(SRC))


@pytest.mark.parametrize("De,Dv,hidden", WIDTHS)
@pytest.mark.parametrize("mode", [ROWS, EDGE, NODE])
def test_wgrad0(cuda, graphs, mode, De, Dv, hidden):
    from dlwp_benchmark_amd import lib as L
    lib, s = L.load(), L.stream()
    G, Gw = graphs
    rows, k0, _ = shape_of(mode, De, Dv)
    x = rand(cuda, 1, rows, De)
    v = None if mode == ROWS else rand(cuda, 2, B * N_NODES, Dv)
    dz = rand(cuda, 3, rows, hidden)
    op = wide_op(mode, Gw, rows, x, v)
    n_ws = lib.dlwp_graph_wgrad0_ws_floats(rows, k0, hidden)
    assert n_ws > 0 and n_ws == lib.dlwp_graph_wide_wgrad0_ws_floats(ctypes.byref(op), hidden)
    got = []
    for wide in (False, True):
        ws = torch.full((n_ws,), float("nan"), device=cuda)
        gw, gb = torch.zeros(hidden, k0, device=cuda), torch.zeros(hidden, device=cuda)
        if wide:
            L.check(lib.dlwp_graph_wide_wgrad0(ctypes.byref(op), L.ptr(dz), L.ptr(ws), L.ptr(gw), L.ptr(gb), hidden, s))
        else:
            src, dst = (L.ptr(G.src), L.ptr(G.dst)) if mode == EDGE else (None, None)
            Bf, N, E = fused_shape(mode)
            L.check(lib.dlwp_graph_wgrad0(mode, L.ptr(x), L.ptr(v), src, dst, L.ptr(dz), L.ptr(ws), L.ptr(gw), L.ptr(gb), Bf, N, E, rows,
                                          De, Dv, hidden, s))
        got.append((gw, gb))
    assert torch.isfinite(got[0][0]).all() and got[0][0].abs().max() > 0
    assert torch.equal(got[0][0], got[1][0]), "gw"
    assert torch.equal(got[0][1], got[1][1]), "gb"


# (mode, index of the output left NULL or None): the rows mode has one output, which the wide entry point requires
DGRAD_CASES = [(ROWS, None), (EDGE, None), (EDGE, 0), (EDGE, 1), (EDGE, 2), (NODE, None), (NODE, 0), (NODE, 1)]


@pytest.mark.parametrize("De,Dv,hidden", WIDTHS)
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("mode,drop", DGRAD_CASES)
def test_dgrad0(cuda, graphs, mode, drop, residual, De, Dv, hidden):
    """dlwp_graph_dgrad0 (64-column blocks) against dlwp_graph_wide_dgrad (128).  On plain rows the fused entry point has no
    residual -- it ignores `res` --, so there it is compared with the wide launch WITHOUT one"""
    from dlwp_benchmark_amd import lib as L
    lib, s = L.load(), L.stream()
    _, Gw = graphs
    rows, k0, parts = shape_of(mode, De, Dv)
    dz, w = rand(cuda, 4, rows, hidden), rand(cuda, 5, hidden, k0)
    res = rand(cuda, 6, rows, parts[{ROWS: 0, EDGE: 0, NODE: 1}[mode]]) if residual else None
    op = wide_op(mode, Gw, rows, torch.empty(rows, De, device=cuda), None if mode == ROWS else torch.empty(B * N_NODES, Dv, device=cuda))
    got = []
    for wide in (False, True):
        outs = [None if i == drop else torch.full((rows, d), float("nan"), device=cuda) for i, d in enumerate(parts)] + [None, None]
        o = [L.ptr(t) for t in outs[:3]]
        if wide:
            L.check(lib.dlwp_graph_wide_dgrad(ctypes.byref(op), L.ptr(dz), L.ptr(w), None if mode == ROWS else L.ptr(res), None, 0,
                                              o[0], o[1], o[2], hidden, s))
        else:
            Bf, N, E = fused_shape(mode)
            L.check(lib.dlwp_graph_dgrad0(mode, L.ptr(dz), L.ptr(w), L.ptr(res), o[0], o[1], o[2], Bf, N, E, rows, De, Dv, hidden, s))
        got.append(outs[:len(parts)])
    for i, (a, b) in enumerate(zip(*got)):
        assert (a is None) == (i == drop)
        if a is not None:
            assert torch.isfinite(a).all(), f"part {i} was not written everywhere"
            assert torch.equal(a, b), f"part {i}"


@pytest.mark.parametrize("De,Dv,hidden", WIDTHS)
def test_dgrad_mul(cuda, De, Dv, hidden):
    """dlwp_graph_dgrad_mul against the wide rows-mode launch with the multiplier taken as it is (mask = 0); the input width is the
    edge mode's K0 (8 and 80 columns: within one block, and past the fused family's 64-column block)"""
    from dlwp_benchmark_amd import graph_ops as go
    from dlwp_benchmark_amd import lib as L
    lib, s = L.load(), L.stream()
    rows, k = ROWS_R, De + 2 * Dv
    dz, w, mul = rand(cuda, 7, rows, hidden), rand(cuda, 8, hidden, k), rand(cuda, 9, rows, k)
    a, b = (torch.full((rows, k), float("nan"), device=cuda) for _ in range(2))
    L.check(lib.dlwp_graph_dgrad_mul(L.ptr(dz), L.ptr(w), L.ptr(mul), L.ptr(a), rows, k, hidden, s))
    op = go._rows_operand(torch.empty(rows, k, device=cuda))
    L.check(lib.dlwp_graph_wide_dgrad(ctypes.byref(op), L.ptr(dz), L.ptr(w), None, L.ptr(mul), 0, L.ptr(b), None, None, hidden, s))
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


@pytest.mark.parametrize("C", [3, 20])
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("mean", [0, 1])
def test_gather_sum_one_list(cuda, graphs, mean, with_add, C):
    from dlwp_benchmark_amd import lib as L
    lib, s = L.load(), L.stream()
    G, Gw = graphs
    E = len(SRC)
    e = rand(cuda, 10, B * E, C)
    add = rand(cuda, 11, B * N_NODES, C) if with_add else None
    a, b = (torch.full((B * N_NODES, C), float("nan"), device=cuda) for _ in range(2))
    L.check(lib.dlwp_graph_gather_sum(L.ptr(e), L.ptr(G.in_ptr), L.ptr(G.in_eid), mean, None, None, None, L.ptr(add), L.ptr(a), B, N_NODES,
                                      E, C, s))
    L.check(lib.dlwp_graph_wide_gather_sum(L.ptr(e), L.ptr(Gw.in_ptr), L.ptr(Gw.in_eid), mean, L.ptr(add), L.ptr(b), B, N_NODES, E, C, s))
    assert torch.isfinite(a).all()
    if not with_add:
        assert not a.view(B, N_NODES, C)[:, 0].any(), "node 0 has no in-edge"
    assert torch.equal(a, b)


@pytest.mark.parametrize("C", [3, 20])
def test_gather_sum_two_lists(cuda, graphs, C):
    """out-edges of d_src + in-edges of d_dst in one launch against the wide family's two, the second adding onto the first"""
    from dlwp_benchmark_amd import lib as L
    lib, s = L.load(), L.stream()
    G, Gw = graphs
    E = len(SRC)
    dsrc, ddst = rand(cuda, 12, B * E, C), rand(cuda, 13, B * E, C)
    a, t, b = (torch.full((B * N_NODES, C), float("nan"), device=cuda) for _ in range(3))
    L.check(lib.dlwp_graph_gather_sum(L.ptr(dsrc), L.ptr(G.out_ptr), L.ptr(G.out_eid), 0, L.ptr(ddst), L.ptr(G.in_ptr), L.ptr(G.in_eid),
                                      None, L.ptr(a), B, N_NODES, E, C, s))
    L.check(lib.dlwp_graph_wide_gather_sum(L.ptr(dsrc), L.ptr(Gw.out_ptr), L.ptr(Gw.out_eid), 0, None, L.ptr(t), B, N_NODES, E, C, s))
    L.check(lib.dlwp_graph_wide_gather_sum(L.ptr(ddst), L.ptr(Gw.in_ptr), L.ptr(Gw.in_eid), 0, L.ptr(t), L.ptr(b), B, N_NODES, E, C, s))
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


@pytest.mark.parametrize("C", [5, 40])
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("mean", [False, True])
def test_edge_gather(cuda, graphs, mean, with_add, C):
    from dlwp_benchmark_amd import lib as L
    lib, s = L.load(), L.stream()
    G, Gw = graphs
    E = len(SRC)
    dagg = rand(cuda, 14, B * N_NODES, C)
    add = rand(cuda, 15, B * E, C) if with_add else None
    a, b = (torch.full((B * E, C), float("nan"), device=cuda) for _ in range(2))
    L.check(lib.dlwp_graph_edge_gather(L.ptr(dagg), L.ptr(G.dst), L.ptr(G.in_ptr) if mean else None, L.ptr(add), L.ptr(a), B, N_NODES, E,
                                       C, s))
    L.check(lib.dlwp_graph_wide_edge_gather(L.ptr(dagg), L.ptr(Gw.dst), L.ptr(Gw.in_ptr) if mean else None, L.ptr(add), L.ptr(b), B,
                                            N_NODES, E, C, s))
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
