"""Row MLPs on graphs over libdlwpmi (csrc/graph_ops.hip forward, csrc/graph_bwd.hip backward; include/dlwpmi.h dlwp_graph_*): the
three blocks the reference's MeshGraphNet (and GraphCast) are built from -- MeshGraphMLP, MeshEdgeBlock, MeshNodeBlock of
models/graphcast/gnn_layers/.

Activations are fp32 row-major `[rows, width]`: node features `[B * N, D]`, edge features `[B * E, D]`, sample after sample.  A
`Graph` holds the int32 index arrays of ONE sample's graph on the device; the kernels form row `b * N + i` / `b * E + k`
themselves, so the arrays do not grow with the batch and never change under graph capture.  `cat(e, v[src], v[dst])` and
`cat(agg, v)` are never written, forward or backward.  Parameters are `nn.Linear` / `nn.LayerNorm`'s own tensors
(`params = [w0, b0, w1, b1, ..., wL, bL]`, `norm = (gamma, beta)` or None); their gradients are accumulated into the preallocated
gradient buffers where those exist.  Under `torch.no_grad()` nothing is stored for a backward pass.  fp32 only; there is no CPU
or torch fallback.

The hidden layers' activation is ReLU (MeshGraphNet) or SiLU (GraphCast).  ReLU's backward takes its mask from the stored
post-ReLU rows.  SiLU is not monotone, so its derivative cannot be read off `z sigmoid(z)`: the forward launch also stores the
derivative rows, and the backward of a later Linear is ONE launch, `dz_{l-1} = (dz_l . W_l) * d_{l-1}` (dlwp_graph_dgrad_mul).

Every width above is 1..128.  The second half of the module is the wide, bipartite family of the dlwpbench GraphCastNet
(csrc/graph_wide.hip forward, the same csrc/graph_bwd.hip backward; dlwp_graph_wide_*): `BipartiteGraph`, `wide_graph_mlp`,
`wide_edge_block`, `wide_node_block` at widths 1..512.
"""
import ctypes as C

import numpy as np
import torch

from . import lib as L
from . import mgn_graph
from .conv_ops import ACT
from .token_ops import _grad_buffer, _grad_slot

ROWS, EDGE, NODE = L.GRAPH_ROWS, L.GRAPH_EDGE, L.GRAPH_NODE
AGGREGATIONS = ("sum", "mean")
ACTIVATIONS = tuple(L.GRAPH_ACT)      # "relu", "silu"
EPS = 1e-5      # nn.LayerNorm's default, which the reference's MeshGraphMLP uses


class _IndexArrays:
    """The six int32 index arrays of one sample's graph -- src, dst, in_ptr, in_eid, out_ptr, out_eid -- kept on the host and moved to
    a device on demand.  The subclasses check them at construction."""

    def _store(self, src, dst, csr, device):
        self._host = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (src, dst) + tuple(csr))
        self.device = None
        if device is not None:
            self.to(device)

    def to(self, device):
        device = torch.device(device)
        if device != self.device:
            (self.src, self.dst, self.in_ptr, self.in_eid, self.out_ptr, self.out_eid) = (torch.from_numpy(a).to(device)
                                                                                          for a in self._host)
            self.device = device
        return self


class Graph(_IndexArrays):
    """Device index arrays of one sample's directed graph: src, dst [E]; in_ptr [N + 1] / in_eid [E]: the edge ids grouped by
    destination; out_ptr / out_eid: grouped by source (all int32).  The CSR forms are built here when absent.  Everything is
    checked on the CPU at construction (indices in range, CSR consistent with src / dst): the kernels trust it."""

    def __init__(self, src, dst, num_nodes, in_ptr=None, in_eid=None, out_ptr=None, out_eid=None, device=None):
        src, dst = np.asarray(src), np.asarray(dst)
        if src.ndim != 1 or src.shape != dst.shape or len(src) == 0 or int(num_nodes) < 1:
            raise ValueError("src and dst must be two non-empty 1-D arrays of the same length, over at least one node")
        if not (np.issubdtype(src.dtype, np.integer) and np.issubdtype(dst.dtype, np.integer)):
            raise ValueError("src and dst must be integer arrays")
        csr = (in_ptr, in_eid, out_ptr, out_eid)
        if any(c is None for c in csr):
            if not all(c is None for c in csr):
                raise ValueError("give all four CSR arrays or none")
            mgn_graph.check_range(src, dst, num_nodes)
            csr = mgn_graph.build_csr(src, dst, num_nodes)
        mgn_graph.check_csr(src, dst, num_nodes, *csr)
        self.num_nodes, self.num_edges = int(num_nodes), len(src)
        self._store(src, dst, csr, device)

    @classmethod
    def from_mesh(cls, mesh, device=None):
        """from a mgn_graph.Graph"""
        return cls(mesh.src, mesh.dst, mesh.num_nodes, mesh.in_ptr, mesh.in_eid, mesh.out_ptr, mesh.out_eid, device=device)


def _rows(t, what):
    if t.dtype != torch.float32:
        raise L.DlwpError(f"{what}: fp32 needed, not {t.dtype}")
    if t.dim() != 2:
        raise L.DlwpError(f"{what}: a [rows, width] tensor is needed, not {tuple(t.shape)}")
    return t.contiguous()


def _check_params(what, params, norm, k0, max_width, check_k0):
    """(hidden layers, hidden width, output width) of [w0, b0, ..., wL, bL] on an operand of width k0; every width (k0 too where
    check_k0) is 1..max_width"""
    if len(params) < 4 or len(params) % 2:
        raise L.DlwpError(f"{what}: params is [w0, b0, ..., wL, bL] with at least one hidden layer, not {len(params)} tensors")
    nl = len(params) // 2 - 1
    if nl > L.GRAPH_MAX_HIDDEN_LAYERS:
        takes = "the kernel takes" if max_width == L.GRAPH_MAX_WIDTH else "the kernels take"
        raise L.DlwpError(f"{what}: {nl} hidden layers, {takes} 1..{L.GRAPH_MAX_HIDDEN_LAYERS}")
    ws = params[0::2]
    hidden, out = ws[0].shape[0], ws[-1].shape[0]
    fan_in = k0
    for i, (w, b) in enumerate(zip(ws, params[1::2])):
        want = (out if i == nl else hidden, fan_in)
        if w.dim() != 2 or tuple(w.shape) != want or b is None or tuple(b.shape) != (want[0],):
            raise L.DlwpError(f"{what}: Linear {i} has weight {tuple(w.shape)}, {want} is needed (all hidden layers share one width)")
        fan_in = hidden
    for d in ((k0,) if check_k0 else ()) + (hidden, out):
        if not 1 <= d <= max_width:
            raise L.DlwpError(f"{what}: width {d} outside 1..{max_width}")
    if norm is not None and (len(norm) != 2 or any(tuple(t.shape) != (out,) for t in norm)):
        raise L.DlwpError(f"{what}: norm is (gamma, beta) of shape ({out},)")
    return nl, hidden, out


class _GraphMlpFn(torch.autograd.Function):
    """One fused launch forward (all three modes, csrc/graph_ops.hip); backward as described in csrc/graph_bwd.hip."""

    @staticmethod
    def forward(ctx, mode, graph, mean, residual, grad, act, x, v, gamma, beta, *params):
        lib = L.load()
        what = ("graph_mlp", "edge_block", "node_block")[mode]
        x = _rows(x, what)
        v = _rows(v, what) if v is not None else None
        dev = x.device
        De, Dv = x.shape[1], (v.shape[1] if v is not None else 0)
        B = 1
        if mode == ROWS:
            rows, k0 = x.shape[0], De
            N = E = 0
        else:
            graph.to(dev)
            N, E = graph.num_nodes, graph.num_edges
            if x.shape[0] % E or v.shape[0] % N or x.shape[0] // E != v.shape[0] // N or x.shape[0] == 0:
                raise L.DlwpError(f"{what}: {x.shape[0]} edge rows and {v.shape[0]} node rows do not make whole samples of a graph "
                                  f"with {E} edges and {N} nodes")
            B = x.shape[0] // E
            rows, k0 = (B * E, De + 2 * Dv) if mode == EDGE else (B * N, De + Dv)
        norm = (gamma, beta) if gamma is not None else None
        nl, hidden, out = _check_params(what, params, norm, k0, L.GRAPH_MAX_WIDTH, mode == ROWS)
        if rows == 0:
            raise L.DlwpError(f"{what}: no rows")
        ws = [p.detach().contiguous() for p in params]
        # grad = torch.is_grad_enabled() as the wrapper saw it: under no_grad a Parameter argument still reports needs_input_grad,
        # and inside forward grad mode is always off
        keep = grad and any(ctx.needs_input_grad)
        y = torch.empty(rows, out, device=dev)
        hid = [torch.empty(rows, hidden, device=dev) for _ in range(nl)] if keep else []
        der = [torch.empty(rows, hidden, device=dev) for _ in range(nl)] if keep and act == L.GRAPH_ACT["silu"] else []
        xhat = torch.empty(rows, out, device=dev) if keep and norm is not None else None
        rstd = torch.empty(rows, device=dev) if keep and norm is not None else None
        agg = torch.empty(rows, De, device=dev) if keep and mode == NODE else None
        a = L.GraphMlpArgs()
        a.mode, a.B, a.N, a.E, a.rows = mode, B, N, E, rows
        a.x, a.v = L.ptr(x), L.ptr(v)
        if mode == EDGE:
            a.src, a.dst = L.ptr(graph.src), L.ptr(graph.dst)
        elif mode == NODE:
            a.in_ptr, a.in_eid = L.ptr(graph.in_ptr), L.ptr(graph.in_eid)
        a.De, a.Dv, a.hidden, a.out, a.hidden_layers = De, Dv, hidden, out, nl
        a.residual, a.mean, a.eps = int(residual), int(mean), EPS
        for i in range(nl + 1):
            a.w[i], a.b[i] = L.ptr(ws[2 * i]), L.ptr(ws[2 * i + 1])
        for i, h in enumerate(hid):
            a.hid[i] = L.ptr(h)
        a.act = act
        for i, d in enumerate(der):
            a.der[i] = L.ptr(d)
        if norm is not None:
            a.gamma, a.beta = L.ptr(gamma.detach().contiguous()), L.ptr(beta.detach().contiguous())
        a.y, a.xhat, a.rstd, a.agg = L.ptr(y), L.ptr(xhat), L.ptr(rstd), L.ptr(agg)
        L.check(lib.dlwp_graph_mlp_fwd(C.byref(a), L.stream()))
        if keep:
            ctx.save_for_backward(x, v, gamma, xhat, rstd, agg, *hid, *ws[0::2], *der)
            ctx.cfg = (mode, graph, mean, residual, B, N, E, rows, De, Dv, hidden, out, nl, act)
            ctx.slots = [_grad_slot(p) for p in params]
            ctx.norm_slots = (_grad_slot(gamma), _grad_slot(beta)) if norm is not None else (None, None)
            ctx.shapes = [p.shape for p in params]
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = L.load()
        mode, graph, mean, residual, B, N, E, rows, De, Dv, hidden, out, nl, act = ctx.cfg
        saved = ctx.saved_tensors
        x, v, gamma, xhat, rstd, agg = saved[:6]
        hid, ws, der = saved[6:6 + nl], saved[6 + nl:7 + 2 * nl], saved[7 + 2 * nl:]
        what = ("graph_mlp", "edge_block", "node_block")[mode]
        gy = _rows(gy, what + " backward")
        dev, s = gy.device, L.stream()
        need = ctx.needs_input_grad            # mode, graph, mean, residual, grad, act, x, v, gamma, beta, *params
        k0 = ws[0].shape[1]

        # LayerNorm (buffers and returned gradients of gamma, beta)
        gnorm, gnorm_out = (None, None), (None, None)
        dz = gy
        if gamma is not None:
            gnorm, gnorm_out = zip(*(_grad_buffer(sl, (out,), dev, n) for sl, n in zip(ctx.norm_slots, need[8:10])))
            scratch = L.workspace(lib.dlwp_graph_ln_bwd_ws_floats, rows, out, device=dev)
            dz = torch.empty(rows, out, device=dev)
            L.check(lib.dlwp_graph_ln_bwd(L.ptr(gy), L.ptr(xhat), L.ptr(rstd), L.ptr(gamma.detach().contiguous()), L.ptr(dz),
                                          L.ptr(scratch), L.ptr(gnorm[0]), L.ptr(gnorm[1]), rows, out, s))
        # the Linears on stored rows, last to second: the 1 x 1 convolution's kernels (a Linear IS one on [rows] pixels)
        pgrads, pgrads_out = zip(*(_grad_buffer(sl, sh, dev, n) for sl, sh, n in zip(ctx.slots, ctx.shapes, need[10:])))
        for i in range(nl, 0, -1):
            cout = out if i == nl else hidden
            scratch = L.workspace(lib.dlwp_conv1x1_wgrad_ws_floats, rows, hidden, cout, device=dev)
            L.check(lib.dlwp_conv1x1_wgrad(L.ptr(hid[i - 1]), L.ptr(dz), L.ptr(scratch), L.ptr(pgrads[2 * i]), L.ptr(pgrads[2 * i + 1]),
                                           rows, hidden, cout, s))
            if der:            # SiLU: the input gradient times the stored derivative, one launch
                dzp = torch.empty(rows, hidden, device=dev)
                L.check(lib.dlwp_graph_dgrad_mul(L.ptr(dz), L.ptr(ws[i]), L.ptr(der[i - 1]), L.ptr(dzp), rows, hidden, cout, s))
                dz = dzp
                continue
            dh = torch.empty(rows, hidden, device=dev)
            L.check(lib.dlwp_conv1x1_dgrad(L.ptr(dz), L.ptr(ws[i]), L.ptr(dh), rows, hidden, cout, s))
            dz = torch.empty(rows, hidden, device=dev)
            L.check(lib.dlwp_conv3x3_act_bwd(L.ptr(hid[i - 1]), L.ptr(dh), L.ptr(dz), dh.numel(), ACT["relu"], s))
        # the first Linear: its operand is gathered again, its input gradient leaves in parts
        src = L.ptr(graph.src) if mode == EDGE else None
        dst = L.ptr(graph.dst) if mode == EDGE else None
        scratch = L.workspace(lib.dlwp_graph_wgrad0_ws_floats, rows, k0, hidden, device=dev)
        L.check(lib.dlwp_graph_wgrad0(mode, L.ptr(agg if mode == NODE else x), L.ptr(v), src, dst, L.ptr(dz), L.ptr(scratch),
                                      L.ptr(pgrads[0]), L.ptr(pgrads[1]), B, N, E, rows, De, Dv, hidden, s))
        gx = gv = None
        res = L.ptr(gy) if residual else None
        if mode == ROWS:
            if need[6]:
                gx = torch.empty_like(x)
                L.check(lib.dlwp_graph_dgrad0(mode, L.ptr(dz), L.ptr(ws[0]), None, L.ptr(gx), None, None, B, N, E, rows, De, Dv, hidden, s))
        elif mode == EDGE:
            gx = torch.empty_like(x) if need[6] else None
            dsrc = torch.empty(rows, Dv, device=dev) if need[7] else None
            ddst = torch.empty(rows, Dv, device=dev) if need[7] else None
            if need[6] or need[7]:
                L.check(lib.dlwp_graph_dgrad0(mode, L.ptr(dz), L.ptr(ws[0]), res, L.ptr(gx), L.ptr(dsrc), L.ptr(ddst), B, N, E, rows,
                                              De, Dv, hidden, s))
            if need[7]:
                gv = torch.empty_like(v)
                L.check(lib.dlwp_graph_gather_sum(L.ptr(dsrc), L.ptr(graph.out_ptr), L.ptr(graph.out_eid), 0, L.ptr(ddst),
                                                  L.ptr(graph.in_ptr), L.ptr(graph.in_eid), None, L.ptr(gv), B, N, E, Dv, s))
        else:
            dagg = torch.empty(rows, De, device=dev) if need[6] else None
            gv = torch.empty_like(v) if need[7] else None
            if need[6] or need[7]:
                L.check(lib.dlwp_graph_dgrad0(mode, L.ptr(dz), L.ptr(ws[0]), res, L.ptr(dagg), L.ptr(gv), None, B, N, E, rows, De, Dv,
                                              hidden, s))
            if need[6]:
                gx = torch.empty_like(x)
                L.check(lib.dlwp_graph_edge_gather(L.ptr(dagg), L.ptr(graph.dst), L.ptr(graph.in_ptr) if mean else None, None,
                                                   L.ptr(gx), B, N, E, De, s))
        return (None, None, None, None, None, None, gx, gv) + tuple(gnorm_out) + tuple(pgrads_out)


def _norm_pair(norm):
    return (None, None) if norm is None else tuple(norm)


def _act_code(act):
    if act not in L.GRAPH_ACT:
        raise ValueError(f"act must be 'relu' or 'silu', not {act!r}")
    return L.GRAPH_ACT[act]


def graph_mlp(x, params, norm=None, act="relu"):
    """`LayerNorm(Linear(act(... act(Linear(x)))))` on rows `x [rows, in]`: params = [w0, b0, ..., wL, bL] (1 to 3 hidden
    layers of one width, every width 1..128), norm = (gamma, beta) or None, act "relu" or "silu".  One launch."""
    return _GraphMlpFn.apply(ROWS, None, False, False, torch.is_grad_enabled(), _act_code(act), x, None, *_norm_pair(norm), *params)


def edge_block(e, v, graph, params, norm=None, residual=True, act="relu"):
    """`e + MLP(cat(e, v[src], v[dst]))` on edge rows `e [B * E, De]` and node rows `v [B * N, Dv]` (MeshEdgeBlock)."""
    if not isinstance(graph, Graph):
        raise TypeError("edge_block: graph must be a graph_ops.Graph")
    return _GraphMlpFn.apply(EDGE, graph, False, bool(residual), torch.is_grad_enabled(), _act_code(act), e, v, *_norm_pair(norm),
                             *params)


def node_block(e, v, graph, params, norm=None, aggregation="sum", residual=True, act="relu"):
    """`v + MLP(cat(agg, v))`, agg[i] = sum or mean of the rows of `e` over the in-edges of node i, zeros where there is none
    (MeshNodeBlock).  Returns the new node rows."""
    if not isinstance(graph, Graph):
        raise TypeError("node_block: graph must be a graph_ops.Graph")
    if aggregation not in AGGREGATIONS:
        raise ValueError(f"aggregation must be 'sum' or 'mean', not {aggregation!r}")
    return _GraphMlpFn.apply(NODE, graph, aggregation == "mean", bool(residual), torch.is_grad_enabled(), _act_code(act), e, v,
                             *_norm_pair(norm), *params)


def aggregate(e, graph, aggregation="sum"):
    """The aggregation on its own (no gradient): `[B * N, D]` sums or means of the rows of `e [B * E, D]` over every node's in-edges."""
    if aggregation not in AGGREGATIONS:
        raise ValueError(f"aggregation must be 'sum' or 'mean', not {aggregation!r}")
    if not isinstance(graph, Graph):
        raise TypeError("aggregate: graph must be a graph_ops.Graph")
    e = _rows(e.detach(), "aggregate")
    if e.shape[0] == 0 or e.shape[0] % graph.num_edges:
        raise L.DlwpError(f"aggregate: {e.shape[0]} edge rows do not make whole samples of a graph with {graph.num_edges} edges")
    graph.to(e.device)
    B = e.shape[0] // graph.num_edges
    out = torch.empty(B * graph.num_nodes, e.shape[1], device=e.device)
    L.check(L.load().dlwp_graph_gather_sum(L.ptr(e), L.ptr(graph.in_ptr), L.ptr(graph.in_eid), int(aggregation == "mean"), None, None,
                                           None, None, L.ptr(out), B, graph.num_nodes, graph.num_edges, e.shape[1], L.stream()))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# The wide, bipartite family (csrc/graph_wide.hip, csrc/graph_bwd.hip; include/dlwpmi.h dlwp_graph_wide_*): widths 1..512, source
# and destination nodes as two sets.  One Linear per launch on a (row tile x column block) grid; LayerNorm and the in-edge
# aggregation are launches of their own.  The forward above keeps its fused 1..128 kernel; the backward kernels are the same ones.


def _check_side(name, ptr, eid, key, n, E):
    ptr, eid = np.asarray(ptr, np.int64), np.asarray(eid, np.int64)
    if len(ptr) != n + 1 or len(eid) != E or ptr[0] != 0 or ptr[-1] != E or (np.diff(ptr) < 0).any():
        raise ValueError(f"{name}_ptr must rise from 0 to {E} over {n + 1} entries and {name}_eid hold {E} edge ids")
    if eid.min() < 0 or eid.max() >= E or len(np.unique(eid)) != E:
        raise ValueError(f"{name}_eid must be a permutation of the {E} edge ids")
    if not np.array_equal(key[eid], np.repeat(np.arange(n), np.diff(ptr))):
        raise ValueError(f"{name}_ptr / {name}_eid do not group the edges by their {'destination' if name == 'in' else 'source'}")


class BipartiteGraph(_IndexArrays):
    """Device index arrays of one sample's directed graph from `num_src` source nodes to `num_dst` destination nodes: src, dst [E];
    in_ptr [num_dst + 1] / in_eid [E]: the edge ids grouped by destination; out_ptr [num_src + 1] / out_eid [E]: grouped by source
    (all int32).  A graph on one node set is the case num_src == num_dst with the same node rows on both sides.  The CSR forms are
    built here when absent; everything is checked on the CPU at construction: the kernels trust it."""

    def __init__(self, src, dst, num_src, num_dst, in_ptr=None, in_eid=None, out_ptr=None, out_eid=None, device=None):
        src, dst = np.asarray(src), np.asarray(dst)
        num_src, num_dst = int(num_src), int(num_dst)
        if src.ndim != 1 or src.shape != dst.shape or len(src) == 0 or num_src < 1 or num_dst < 1:
            raise ValueError("src and dst must be two non-empty 1-D arrays of the same length, over at least one node on each side")
        if not (np.issubdtype(src.dtype, np.integer) and np.issubdtype(dst.dtype, np.integer)):
            raise ValueError("src and dst must be integer arrays")
        src64, dst64 = src.astype(np.int64), dst.astype(np.int64)
        E = len(src)
        if src64.min() < 0 or dst64.min() < 0 or src64.max() >= num_src or dst64.max() >= num_dst:
            raise ValueError(f"edge endpoints must be {E} pairs (source in [0, {num_src}), destination in [0, {num_dst}))")
        csr = (in_ptr, in_eid, out_ptr, out_eid)
        if any(c is None for c in csr):
            if not all(c is None for c in csr):
                raise ValueError("give all four CSR arrays or none")
            csr = ()
            for key, n in ((dst64, num_dst), (src64, num_src)):
                ptr = np.zeros(n + 1, np.int64)
                np.cumsum(np.bincount(key, minlength=n), out=ptr[1:])
                csr += (ptr, np.argsort(key, kind="stable"))
        _check_side("in", csr[0], csr[1], dst64, num_dst, E)
        _check_side("out", csr[2], csr[3], src64, num_src, E)
        self.num_src, self.num_dst, self.num_edges = num_src, num_dst, E
        self._store(src, dst, csr, device)


def _wide_rows(t, what):
    if not t.is_cuda:
        raise L.DlwpError(f"{what}: a tensor on the CPU; the graph kernels run on the GPU and there is no CPU path")
    return _rows(t, what)


def _operand(mode, graph, B, rows, x, vs, vd):
    """dlwp_graph_wide_operand of a first Linear (x: rows, edge rows or the aggregate)"""
    op = L.GraphWideOperand()
    op.mode, op.B, op.rows = mode, B, rows
    op.x, op.D0 = L.ptr(x), x.shape[1]
    if mode == EDGE:
        op.Ns, op.Nd, op.E = graph.num_src, graph.num_dst, graph.num_edges
        op.vs, op.vd, op.D1, op.D2 = L.ptr(vs), L.ptr(vd), vs.shape[1], vd.shape[1]
        op.src, op.dst = L.ptr(graph.src), L.ptr(graph.dst)
    elif mode == NODE:
        op.Nd, op.E = graph.num_dst, graph.num_edges
        op.vs, op.D1 = L.ptr(vs), vs.shape[1]
    return op


def _rows_operand(x):
    return _operand(ROWS, None, 1, x.shape[0], x, None, None)


WIDE_NAMES = ("wide_graph_mlp", "wide_edge_block", "wide_node_block")


def wide_forward(mode, graph, mean, residual, act, x, vs, vd, norm, params, keep):
    """The launches of one MLP: [aggregation,] L x (Linear + bias + activation), Linear + bias [+ residual] [, LayerNorm + residual].
    Returns (y, stored): `stored` holds what a backward pass reads -- x, vs, vd, agg, hid (post-activation rows), der (SiLU's
    derivative rows), xhat, rstd -- and is EMPTY when keep is false: nothing is stored then (the hidden rows are temporaries)."""
    lib = L.load()
    what = WIDE_NAMES[mode]
    x = _wide_rows(x, what)
    vs = _wide_rows(vs, what) if vs is not None else None
    vd = _wide_rows(vd, what) if vd is not None else None
    dev = x.device
    B = 1
    if mode == ROWS:
        rows, k0 = x.shape[0], x.shape[1]
    else:
        graph.to(dev)
        E, Ns, Nd = graph.num_edges, graph.num_src, graph.num_dst
        B = x.shape[0] // E
        ok = x.shape[0] > 0 and x.shape[0] == B * E and vd.shape[0] == B * Nd and (mode == NODE or vs.shape[0] == B * Ns)
        if not ok:
            raise L.DlwpError(f"{what}: {x.shape[0]} edge rows, {None if vs is None else vs.shape[0]} source and {vd.shape[0]} destination "
                              f"node rows do not make whole samples of a graph with {E} edges, {Ns} source and {Nd} destination nodes")
        rows, k0 = (B * E, x.shape[1] + vs.shape[1] + vd.shape[1]) if mode == EDGE else (B * Nd, x.shape[1] + vd.shape[1])
    for t in (x, vs, vd):
        if t is not None and not 1 <= t.shape[1] <= L.GRAPH_WIDE_MAX_WIDTH:
            raise L.DlwpError(f"{what}: width {t.shape[1]} outside 1..{L.GRAPH_WIDE_MAX_WIDTH}")
    nl, hidden, out = _check_params(what, params, norm, k0, L.GRAPH_WIDE_MAX_WIDTH, False)
    if rows == 0:
        raise L.DlwpError(f"{what}: no rows")
    res = None
    if residual:
        res = (x, x, vd)[mode]
        if res.shape[1] != out:
            raise L.DlwpError(f"{what}: the residual has width {res.shape[1]}, the output {out}")
    ws = [p.detach().contiguous() for p in params]
    silu, s = act == L.GRAPH_ACT["silu"], L.stream()
    agg = None
    if mode == NODE:
        agg = torch.empty(rows, x.shape[1], device=dev)
        L.check(lib.dlwp_graph_wide_gather_sum(L.ptr(x), L.ptr(graph.in_ptr), L.ptr(graph.in_eid), int(mean), None, L.ptr(agg), B,
                                               graph.num_dst, graph.num_edges, x.shape[1], s))
        op = _operand(NODE, graph, B, rows, agg, vd, None)
    else:
        op = _operand(mode, graph, B, rows, x, vs, vd)
    hid, der = [], []
    for i in range(nl):
        h = torch.empty(rows, hidden, device=dev)
        d = torch.empty(rows, hidden, device=dev) if keep and silu else None
        L.check(lib.dlwp_graph_wide_linear_fwd(C.byref(op), L.ptr(ws[2 * i]), L.ptr(ws[2 * i + 1]), None, L.ptr(h), L.ptr(d), hidden,
                                               act, s))
        hid.append(h)
        if d is not None:
            der.append(d)
        op = _rows_operand(h)
    y = torch.empty(rows, out, device=dev)
    xhat = rstd = None
    if norm is None:
        L.check(lib.dlwp_graph_wide_linear_fwd(C.byref(op), L.ptr(ws[2 * nl]), L.ptr(ws[2 * nl + 1]), L.ptr(res), L.ptr(y), None, out,
                                               L.GRAPH_WIDE_ACT_NONE, s))
    else:
        z = torch.empty(rows, out, device=dev)
        L.check(lib.dlwp_graph_wide_linear_fwd(C.byref(op), L.ptr(ws[2 * nl]), L.ptr(ws[2 * nl + 1]), None, L.ptr(z), None, out,
                                               L.GRAPH_WIDE_ACT_NONE, s))
        if keep:
            xhat, rstd = torch.empty(rows, out, device=dev), torch.empty(rows, device=dev)
        L.check(lib.dlwp_graph_wide_ln_fwd(L.ptr(z), L.ptr(norm[0].detach().contiguous()), L.ptr(norm[1].detach().contiguous()),
                                           L.ptr(res), L.ptr(y), L.ptr(xhat), L.ptr(rstd), rows, out, EPS, s))
    stored = dict(x=x, vs=vs, vd=vd, agg=agg, hid=hid, der=der, xhat=xhat, rstd=rstd, ws=ws, B=B, rows=rows) if keep else {}
    return y, stored


class _WideMlpFn(torch.autograd.Function):
    """wide_forward, and the backward described in csrc/graph_bwd.hip."""

    @staticmethod
    def forward(ctx, mode, graph, mean, residual, grad, act, x, vs, vd, gamma, beta, *params):
        norm = (gamma, beta) if gamma is not None else None
        keep = grad and any(ctx.needs_input_grad)      # as _GraphMlpFn: grad is the wrapper's torch.is_grad_enabled()
        y, st = wide_forward(mode, graph, mean, residual, act, x, vs, vd, norm, params, keep)
        if keep:
            nl = len(st["hid"])
            same = mode == EDGE and vs is vd
            ctx.save_for_backward(st["x"], st["vs"], st["vd"], gamma, st["xhat"], st["rstd"], st["agg"], *st["hid"], *st["ws"][0::2],
                                  *st["der"])
            ctx.cfg = (mode, graph, mean, residual, st["B"], st["rows"], nl, act, same)
            ctx.slots = [_grad_slot(p) for p in params]
            ctx.norm_slots = (_grad_slot(gamma), _grad_slot(beta)) if norm is not None else (None, None)
            ctx.shapes = [p.shape for p in params]
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = L.load()
        mode, graph, mean, residual, B, rows, nl, act, same = ctx.cfg
        saved = ctx.saved_tensors
        x, vs, vd, gamma, xhat, rstd, agg = saved[:7]
        hid, ws, der = saved[7:7 + nl], saved[7 + nl:8 + 2 * nl], saved[8 + 2 * nl:]
        what = WIDE_NAMES[mode]
        gy = _rows(gy, what + " backward")
        dev, s = gy.device, L.stream()
        need = ctx.needs_input_grad            # mode, graph, mean, residual, grad, act, x, vs, vd, gamma, beta, *params
        hidden, out = ws[0].shape[0], ws[-1].shape[0]

        gnorm_out = (None, None)
        dz = gy
        if gamma is not None:
            gnorm, gnorm_out = zip(*(_grad_buffer(sl, (out,), dev, n) for sl, n in zip(ctx.norm_slots, need[9:11])))
            scratch = L.workspace(lib.dlwp_graph_wide_ln_bwd_ws_floats, rows, out, device=dev)
            dz = torch.empty(rows, out, device=dev)
            L.check(lib.dlwp_graph_wide_ln_bwd(L.ptr(gy), L.ptr(xhat), L.ptr(rstd), L.ptr(gamma.detach().contiguous()), L.ptr(dz),
                                               L.ptr(scratch), L.ptr(gnorm[0]), L.ptr(gnorm[1]), rows, out, s))
        pgrads, pgrads_out = zip(*(_grad_buffer(sl, sh, dev, n) for sl, sh, n in zip(ctx.slots, ctx.shapes, need[11:])))
        # the Linears on stored rows, last to second: dz_{l-1} = (dz_l . W_l) * d_{l-1}, one launch (SiLU: the stored derivative
        # rows; ReLU: the mask of the stored post-activation rows)
        for i in range(nl, 0, -1):
            cout = out if i == nl else hidden
            scratch = L.workspace(lib.dlwp_conv1x1_wgrad_ws_floats, rows, hidden, cout, device=dev)
            L.check(lib.dlwp_conv1x1_wgrad(L.ptr(hid[i - 1]), L.ptr(dz), L.ptr(scratch), L.ptr(pgrads[2 * i]), L.ptr(pgrads[2 * i + 1]),
                                           rows, hidden, cout, s))
            dzp = torch.empty(rows, hidden, device=dev)
            mul = der[i - 1] if der else hid[i - 1]
            L.check(lib.dlwp_graph_wide_dgrad(C.byref(_rows_operand(hid[i - 1])), L.ptr(dz), L.ptr(ws[i]), None, L.ptr(mul),
                                              0 if der else 1, L.ptr(dzp), None, None, cout, s))
            dz = dzp
        # the first Linear: its operand is gathered again, its input gradient leaves in parts
        op = _operand(mode, graph, B, rows, agg if mode == NODE else x, vd if mode == NODE else vs, vd)
        scratch = L.workspace(lib.dlwp_graph_wide_wgrad0_ws_floats, C.byref(op), hidden, device=dev)
        L.check(lib.dlwp_graph_wide_wgrad0(C.byref(op), L.ptr(dz), L.ptr(scratch), L.ptr(pgrads[0]), L.ptr(pgrads[1]), hidden, s))
        gx = gvs = gvd = None
        res = L.ptr(gy) if residual else None
        if mode == ROWS:
            if need[6]:
                gx = torch.empty_like(x)
                L.check(lib.dlwp_graph_wide_dgrad(C.byref(op), L.ptr(dz), L.ptr(ws[0]), res, None, 0, L.ptr(gx), None, None, hidden, s))
        elif mode == EDGE:
            want_v = need[7] or need[8]
            gx = torch.empty_like(x) if need[6] else None
            dsrc = torch.empty(rows, vs.shape[1], device=dev) if want_v else None
            ddst = torch.empty(rows, vd.shape[1], device=dev) if want_v else None
            if need[6] or want_v:
                L.check(lib.dlwp_graph_wide_dgrad(C.byref(op), L.ptr(dz), L.ptr(ws[0]), res, None, 0, L.ptr(gx), L.ptr(dsrc), L.ptr(ddst),
                                                  hidden, s))
            if want_v:      # out-edges onto the sources, in-edges onto the destinations (one node set: the second sum on top)
                gvs = torch.empty_like(vs)
                L.check(lib.dlwp_graph_wide_gather_sum(L.ptr(dsrc), L.ptr(graph.out_ptr), L.ptr(graph.out_eid), 0, None, L.ptr(gvs), B,
                                                       graph.num_src, graph.num_edges, vs.shape[1], s))
                gvd = gvs if same else torch.empty_like(vd)
                L.check(lib.dlwp_graph_wide_gather_sum(L.ptr(ddst), L.ptr(graph.in_ptr), L.ptr(graph.in_eid), 0,
                                                       L.ptr(gvs) if same else None, L.ptr(gvd), B, graph.num_dst, graph.num_edges,
                                                       vd.shape[1], s))
                if same:      # autograd adds what the two arguments return: the sum goes back once
                    gvd = None
        else:
            dagg = torch.empty(rows, x.shape[1], device=dev) if need[6] else None
            gvd = torch.empty_like(vd) if need[8] else None
            if need[6] or need[8]:
                L.check(lib.dlwp_graph_wide_dgrad(C.byref(op), L.ptr(dz), L.ptr(ws[0]), res, None, 0, L.ptr(dagg), L.ptr(gvd), None,
                                                  hidden, s))
            if need[6]:
                gx = torch.empty_like(x)
                L.check(lib.dlwp_graph_wide_edge_gather(L.ptr(dagg), L.ptr(graph.dst), L.ptr(graph.in_ptr) if mean else None, None,
                                                        L.ptr(gx), B, graph.num_dst, graph.num_edges, x.shape[1], s))
        return (None, None, None, None, None, None, gx, gvs, gvd) + tuple(gnorm_out) + tuple(pgrads_out)


def _bipartite(what, graph):
    if not isinstance(graph, BipartiteGraph):
        raise TypeError(f"{what}: graph must be a graph_ops.BipartiteGraph")


def wide_graph_mlp(x, params, norm=None, act="silu", residual=False):
    """`[x +] LayerNorm(Linear(act(... act(Linear(x)))))` on rows `x [rows, in]`: params = [w0, b0, ..., wL, bL] (1 to 3 hidden
    layers of one width, every width 1..512), norm = (gamma, beta) or None, act "silu" or "relu"."""
    return _WideMlpFn.apply(ROWS, None, False, bool(residual), torch.is_grad_enabled(), _act_code(act), x, None, None,
                            *_norm_pair(norm), *params)


def wide_edge_block(e, v_src, v_dst, graph, params, norm=None, residual=True, act="silu"):
    """`[e +] MLP(cat(e, v_src[src], v_dst[dst]))` on edge rows `e [B * E, De]`, source node rows `v_src [B * Ns, Ds]` and
    destination node rows `v_dst [B * Nd, Dd]` (MeshGraphEdgeMLPConcat; with the residual, MeshEdgeBlock).  On a graph over one
    node set pass the same tensor twice."""
    _bipartite("wide_edge_block", graph)
    return _WideMlpFn.apply(EDGE, graph, False, bool(residual), torch.is_grad_enabled(), _act_code(act), e, v_src, v_dst,
                            *_norm_pair(norm), *params)


def wide_node_block(e, v_dst, graph, params, norm=None, aggregation="sum", residual=True, act="silu"):
    """`[v_dst +] MLP(cat(agg, v_dst))`, agg[i] = sum or mean of the rows of `e` over the in-edges of destination node i, zeros
    where there is none (aggregate_and_concat + MeshGraphMLP).  Returns the new destination node rows."""
    _bipartite("wide_node_block", graph)
    if aggregation not in AGGREGATIONS:
        raise ValueError(f"aggregation must be 'sum' or 'mean', not {aggregation!r}")
    return _WideMlpFn.apply(NODE, graph, aggregation == "mean", bool(residual), torch.is_grad_enabled(), _act_code(act), e, None,
                            v_dst, *_norm_pair(norm), *params)
