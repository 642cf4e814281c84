"""float64 torch restatement of ONE row MLP of the wide, bipartite graph kernels (csrc/graph_wide.hip), from elementary operations
on the CPU: the operand assembled by index, L x (Linear + SiLU | ReLU), Linear, LayerNorm (biased variance, eps 1e-5), residual, and
everything a backward pass stores.  Used by tests/test_gpu_graph_wide.py; tests/graphcast_dlwp_ref.py builds the model from it."""
import numpy as np
import torch
import torch.nn.functional as F

ROWS, EDGE, NODE = 0, 1, 2
EPS = 1e-5


def bipartite_handmade():
    """(src, dst, Ns, Nd): 23 sources, 17 destinations, 65 edges in no order.  Destination 0 has no in-edge and source 1 no
    out-edge; sources 19..22 and destinations 15, 16 do not occur at all; a duplicate edge; nine edges into destination 7."""
    rng = np.random.RandomState(11)
    src = [2, 2] + [3 + i for i in range(9)]
    dst = [3, 3] + [7] * 9
    while len(src) < 65:
        s, d = int(rng.randint(0, 19)), int(rng.randint(0, 15))
        if s != 1 and d != 0:
            src.append(s)
            dst.append(d)
    perm = rng.permutation(65)
    src, dst = np.array(src)[perm], np.array(dst)[perm]
    assert 0 not in dst and 1 not in src and 0 in src and 1 in dst and src.max() < 19 and dst.max() < 15
    return src, dst, 23, 17


def aggregate64(e, dst, Nd, B, mean):
    """[B * Nd, D] sums (means) of the edge rows over every destination's in-edges; zeros where there is none"""
    E = len(dst)
    idx = torch.as_tensor(np.concatenate([np.asarray(dst, np.int64) + b * Nd for b in range(B)]))
    agg = torch.zeros(B * Nd, e.shape[1], dtype=e.dtype).index_add(0, idx, e)
    if mean:
        deg = torch.bincount(idx, minlength=B * Nd).clamp(min=1).to(e.dtype)
        agg = agg / deg[:, None]
    assert e.shape[0] == B * E
    return agg


def operand64(mode, graph, B, x, vs, vd, mean):
    """(A, agg): the operand rows of the first Linear.  graph = (src, dst, Ns, Nd) numpy"""
    if mode == ROWS:
        return x, None
    src, dst, Ns, Nd = graph
    if mode == EDGE:
        si = torch.as_tensor(np.concatenate([np.asarray(src, np.int64) + b * Ns for b in range(B)]))
        di = torch.as_tensor(np.concatenate([np.asarray(dst, np.int64) + b * Nd for b in range(B)]))
        return torch.cat([x, vs[si], vd[di]], dim=1), None
    agg = aggregate64(x, dst, Nd, B, mean)
    return torch.cat([agg, vd], dim=1), agg


def mlp64(mode, graph, B, x, vs, vd, params, norm, residual, mean, act, gy=None, same=False):
    """-> (y, stored, grads) in float64.  stored: hid, der (SiLU), xhat, rstd, agg; grads (when gy is given): x, vs, vd, p0.., gamma,
    beta.  same: vs and vd are ONE tensor (a graph on one node set): its gradient is returned as grads["vs"]."""
    leaf = lambda t: None if t is None else t.detach().double().cpu().requires_grad_(True)      # noqa: E731
    x, vs, params = leaf(x), leaf(vs), [leaf(p) for p in params]
    vd = vs if same else leaf(vd)
    norm = [leaf(t) for t in norm] if norm is not None else None
    A, agg = operand64(mode, graph, B, x, vs, vd, mean)
    h, hid, der = A, [], []
    nl = len(params) // 2 - 1
    for l in range(nl):
        z = F.linear(h, params[2 * l], params[2 * l + 1])
        if act == "silu":
            s = torch.sigmoid(z)
            h = z * s
            der.append((s * (1 + z * (1 - s))).detach())
        else:
            h = torch.clamp(z, min=0)
        hid.append(h.detach())
    y = F.linear(h, params[2 * nl], params[2 * nl + 1])
    xhat = rstd = None
    if norm is not None:
        c = y - y.mean(dim=1, keepdim=True)
        r = 1 / torch.sqrt((c * c).mean(dim=1, keepdim=True) + EPS)
        xhat, rstd = (c * r).detach(), r[:, 0].detach()
        y = c * r * norm[0] + norm[1]
    if residual:
        y = y + (x, x, vd)[mode]
    stored = dict(hid=hid, der=der, xhat=xhat, rstd=rstd, agg=None if agg is None else agg.detach())
    grads = None
    if gy is not None:
        (y * gy.detach().double().cpu()).sum().backward()
        grads = {"x": x.grad, "vs": None if vs is None else vs.grad, "vd": None if (vd is None or same) else vd.grad}
        grads.update({f"p{i}": p.grad for i, p in enumerate(params)})
        if norm is not None:
            grads.update(gamma=norm[0].grad, beta=norm[1].grad)
    return y.detach(), stored, grads
