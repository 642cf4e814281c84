"""Row MLPs on graphs over libdlwpmi (csrc/graph_ops.hip; include/dlwpmi.h dlwp_graph_*): the three blocks the reference's
MeshGraphNet (and GraphCast) are built from -- MeshGraphMLP, MeshEdgeBlock, MeshNodeBlock of models/graphcast/gnn_layers/.

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


class Graph:
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
        self._host = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (src, dst) + tuple(csr))
        self.device = None
        if device is not None:
            self.to(device)

    @classmethod
    def from_mesh(cls, mesh, device=None):
        """from a mgn_graph.Graph"""
        return cls(mesh.src, mesh.dst, mesh.num_nodes, mesh.in_ptr, mesh.in_eid, mesh.out_ptr, mesh.out_eid, device=device)

    def to(self, device):
        device = torch.device(device)
        if device != self.device:
            (self.src, self.dst, self.in_ptr, self.in_eid, self.out_ptr, self.out_eid) = (torch.from_numpy(a).to(device)
                                                                                          for a in self._host)
            self.device = device
        return self


def _rows(t, what):
    if t.dtype != torch.float32:
        raise L.DlwpError(f"{what}: fp32 needed, not {t.dtype}")
    if t.dim() != 2:
        raise L.DlwpError(f"{what}: a [rows, width] tensor is needed, not {tuple(t.shape)}")
    return t.contiguous()


def _check_params(what, params, norm, k0):
    """(hidden layers, hidden width, output width) of [w0, b0, ..., wL, bL] on an operand of width k0"""
    if len(params) < 4 or len(params) % 2:
        raise L.DlwpError(f"{what}: params is [w0, b0, ..., wL, bL] with at least one hidden layer, not {len(params)} tensors")
    nl = len(params) // 2 - 1
    if nl > L.GRAPH_MAX_HIDDEN_LAYERS:
        raise L.DlwpError(f"{what}: {nl} hidden layers, the kernel takes 1..{L.GRAPH_MAX_HIDDEN_LAYERS}")
    ws = params[0::2]
    hidden, out = ws[0].shape[0], ws[-1].shape[0]
    fan_in = k0
    for i, (w, b) in enumerate(zip(ws, params[1::2])):
        want = (out if i == nl else hidden, fan_in)
        if w.dim() != 2 or tuple(w.shape) != want or b is None or tuple(b.shape) != (want[0],):
            raise L.DlwpError(f"{what}: Linear {i} has weight {tuple(w.shape)}, {want} is needed (all hidden layers share one width)")
        fan_in = hidden
    for d in (k0 if what == "graph_mlp" else 1, hidden, out):
        if not 1 <= d <= L.GRAPH_MAX_WIDTH:
            raise L.DlwpError(f"{what}: width {d} outside 1..{L.GRAPH_MAX_WIDTH}")
    if norm is not None and (len(norm) != 2 or any(tuple(t.shape) != (out,) for t in norm)):
        raise L.DlwpError(f"{what}: norm is (gamma, beta) of shape ({out},)")
    return nl, hidden, out


class _GraphMlpFn(torch.autograd.Function):
    """One fused launch forward (all three modes); backward as described in csrc/graph_ops.hip."""

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
        nl, hidden, out = _check_params(what, params, norm, k0)
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
