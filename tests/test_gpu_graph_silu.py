"""The SiLU path of the graph kernels (csrc/graph_ops.hip: graph_mlp_kernel<.., SILU>, dlwp_graph_dgrad_mul) through the RAW entry
points against float64 torch on the CPU, in the style of tests/test_gpu_graph_ops.py and on its hand-made graph (N = 37 nodes,
E = 101 edges: a node without in-edges, one without out-edges, a self-loop, a duplicate edge, in-degree >= 9).  With B in {1, 3}
the row counts (101, 303, 37, 111) are no multiples of the 64-row tile and cross a tile boundary.

Bars (`rel_gap`: max |difference| relative to the max norm of the float64 array), that file's: 1e-5 for y, the stored
post-activation rows and the stored derivative rows, 5e-5 for every gradient.  The MFMA path is exact fp32; SiLU adds one
hardware exp (1 ulp on an argument rounded once: relative error of exp(-v) about (1 + |v|) 2^-23, i.e. <= 2e-6 up to |v| = 16,
beyond which exp(-v) no longer shows in 1 + exp(-v) or the result is below 2e-6 of the row's norm) and one division.  Behind every
output and scratch buffer lie 64 sentinel floats that must come back bit for bit.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from mgn_ref import rel_gap
from test_gpu_graph_ops import EDGE, MODE_NAME, NODE, ROWS, Out, bits, handmade, operand64

pytestmark = pytest.mark.gpu

BAR_OUT, BAR_GRAD = 1e-5, 5e-5
SILU = 1


@pytest.fixture(scope="module")
def G(cuda):
    from dlwp_benchmark_amd.graph_ops import Graph
    return Graph(*handmade(), device=cuda)


def reference(mode, G, B, x, v, params, norm, residual, mean, gy):
    leaf = lambda t: None if t is None else t.double().requires_grad_(True)      # noqa: E731
    x, v, params, norm = leaf(x), leaf(v), [leaf(p) for p in params], ([leaf(t) for t in norm] if norm else None)
    A, agg = operand64(mode, G, B, x, v, mean)
    h, hid, der = A, [], []
    nl = len(params) // 2 - 1
    for l in range(nl):
        z = F.linear(h, params[2 * l], params[2 * l + 1])
        s = torch.sigmoid(z)
        h = z * s
        hid.append(h)
        der.append((s * (1 + z * (1 - s))).detach())
    z = F.linear(h, params[2 * nl], params[2 * nl + 1])
    y = z
    if norm:      # from elementary operations, as in test_gpu_graph_ops.reference (exact zeros at width 1)
        c = z - z.mean(dim=1, keepdim=True)
        y = c / torch.sqrt((c * c).mean(dim=1, keepdim=True) + 1e-5) * norm[0] + norm[1]
    if residual:
        y = y + (x if mode == EDGE else v)
    (y * gy.double()).sum().backward()
    g = {"x": x.grad, "v": None if v is None else v.grad}
    g.update({f"p{i}": p.grad for i, p in enumerate(params)})
    if norm:
        g.update(gamma=norm[0].grad, beta=norm[1].grad)
    return y.detach(), [t.detach() for t in hid], der, (None if agg is None else agg.detach()), g


def raw_run(dev, gen, mode, G, B, x, v, params, norm, residual, mean, gy):
    """SiLU forward and the whole backward through the raw entry points, every output and scratch buffer in an `Out`"""
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
    der = [mk(f"der{l}", (rows, hidden)) for l in range(nl)]
    a = L.GraphMlpArgs()
    a.mode, a.B, a.N, a.E, a.rows, a.act = mode, B, N, E, rows, SILU
    a.x, a.v = L.ptr(xd), L.ptr(vd)
    if mode:
        a.src, a.dst, a.in_ptr, a.in_eid = L.ptr(G.src), L.ptr(G.dst), L.ptr(G.in_ptr), L.ptr(G.in_eid)
    a.De, a.Dv, a.hidden, a.out, a.hidden_layers, a.residual, a.mean, a.eps = De, Dv, hidden, out, nl, int(residual), int(mean), 1e-5
    for i in range(nl + 1):
        a.w[i], a.b[i] = L.ptr(pd[2 * i]), L.ptr(pd[2 * i + 1])
    for i in range(nl):
        a.hid[i], a.der[i] = L.ptr(hid[i].t), L.ptr(der[i].t)
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
        a.hid[i], a.der[i] = None, None
    L.check(lib.dlwp_graph_mlp_fwd(ctypes.byref(a), s))
    assert torch.equal(bits(y.t), bits(y2.t))

    ws_of = lambda name, n: mk(name, (int(n),))      # noqa: E731
    pg = [mk(f"g_p{i}", tuple(p.shape), zero=True) for i, p in enumerate(pd)]
    dz = gyd
    if norm:
        dzo = mk("dz_ln", (rows, out))
        L.check(lib.dlwp_graph_ln_bwd(L.ptr(gyd), L.ptr(outs["xhat"].t), L.ptr(outs["rstd"].t), L.ptr(nd[0]), L.ptr(dzo.t),
                                      L.ptr(ws_of("ws_ln", lib.dlwp_graph_ln_bwd_ws_floats(rows, out)).t),
                                      L.ptr(mk("g_gamma", (out,), zero=True).t), L.ptr(mk("g_beta", (out,), zero=True).t), rows, out, s))
        dz = dzo.t
    for i in range(nl, 0, -1):        # later Linears: weight gradient on the stored rows, then (dz . W) * d in ONE launch
        cout = out if i == nl else hidden
        ws = ws_of(f"ws_w{i}", lib.dlwp_conv1x1_wgrad_ws_floats(rows, hidden, cout))
        L.check(lib.dlwp_conv1x1_wgrad(L.ptr(hid[i - 1].t), L.ptr(dz), L.ptr(ws.t), L.ptr(pg[2 * i].t), L.ptr(pg[2 * i + 1].t), rows,
                                       hidden, cout, s))
        dzp = mk(f"dz{i - 1}", (rows, hidden))
        L.check(lib.dlwp_graph_dgrad_mul(L.ptr(dz), L.ptr(pd[2 * i]), L.ptr(der[i - 1].t), L.ptr(dzp.t), rows, hidden, cout, s))
        dz = dzp.t
    src, dst = (L.ptr(G.src), L.ptr(G.dst)) if mode == EDGE else (None, None)
    x0 = outs["agg"].t if mode == NODE else xd
    L.check(lib.dlwp_graph_wgrad0(mode, L.ptr(x0), L.ptr(vd), src, dst, L.ptr(dz),
                                  L.ptr(ws_of("ws_w0", lib.dlwp_graph_wgrad0_ws_floats(rows, k0, hidden)).t), L.ptr(pg[0].t),
                                  L.ptr(pg[1].t), B, N, E, rows, De, Dv, hidden, s))
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
    for k, o in outs.items():
        assert o.sentinels_intact(), f"{k}: the kernel wrote behind its buffer"
    return got


# (in, hidden, out, hidden layers, B, LayerNorm, mean, residual where the mode allows it): widths 5 / 34 / 116 take the NS 2 / 4 / 8
# instantiations with K and N tails (no multiple of 16); every depth, both batch sizes, with and without LayerNorm and residual,
# sum and mean
SHAPES = [
    (5, 5, 5, 1, 1, True, False, True),
    (5, 5, 5, 3, 3, False, True, False),
    (3, 5, 4, 2, 1, True, True, False),
    (34, 34, 34, 2, 3, True, False, True),
    (34, 34, 34, 3, 1, False, True, True),
    (34, 20, 34, 1, 3, True, True, False),
    (116, 116, 116, 2, 1, True, False, True),
    (116, 116, 116, 3, 3, True, True, False),
    (116, 116, 116, 1, 1, False, False, True),
]


def make_case(mode, G, shape, seed, big_bias=False):
    cin, hidden, out, nl, B, use_norm, mean, residual = shape
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
    if big_bias:      # hidden units 0, 3, 6, ... of the first layer far out on either side
        params[1][0::6] += 150.0
        params[1][3::6] -= 150.0
    norm = [1.0 + 0.3 * rnd(out), 0.3 * rnd(out)] if use_norm else None
    return gen, B, x, v, params, norm, residual, mean and mode == NODE, rnd(rows, out)


def compare(tag, got, ref, nparams, mode, norm):
    y64, hid64, der64, agg64, g64 = ref
    gaps = {"y": rel_gap(got["y"], y64)}
    gaps.update({f"hid{l}": rel_gap(got[f"hid{l}"], h) for l, h in enumerate(hid64)})
    gaps.update({f"der{l}": rel_gap(got[f"der{l}"], h) for l, h in enumerate(der64)})
    if agg64 is not None:
        gaps["agg"] = rel_gap(got["agg"], agg64)
    print(f"{tag}: outputs " + ", ".join(f"{k} {g:.1e}" for k, g in gaps.items()))
    ggaps = {k: rel_gap(got["g_" + k], r) for k, r in g64.items() if r is not None}
    print("  gradients " + ", ".join(f"{k} {g:.1e}" for k, g in ggaps.items()))
    for k, t in got.items():
        if not k.startswith("ws_"):
            assert torch.isfinite(t).all(), k
    for k, g in gaps.items():
        assert g <= BAR_OUT, (k, g)
    assert set(ggaps) == {"x"} | ({"v"} if mode else set()) | {f"p{i}" for i in range(nparams)} | ({"gamma", "beta"} if norm else set())
    for k, g in ggaps.items():
        assert g <= BAR_GRAD, (k, g)


@pytest.mark.parametrize("mode", [ROWS, EDGE, NODE], ids=["rows", "edge", "node"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}-{s[1]}-{s[2]}_L{s[3]}_B{s[4]}" for s in SHAPES])
def test_silu_forward_and_every_gradient(cuda, G, mode, shape):
    gen, B, x, v, params, norm, residual, mean, gy = make_case(mode, G, shape, seed=1000 + 100 * mode + sum(shape[:5]))
    ref = reference(mode, G, B, x, v, params, norm, residual, mean, gy)
    got = raw_run(cuda, gen, mode, G, B, x, v, params, norm, residual, mean, gy)
    again = raw_run(cuda, gen, mode, G, B, x, v, params, norm, residual, mean, gy)
    for k in got:                                              # every launch repeated on the same operands: bit-identical
        if not k.startswith("ws_"):
            assert torch.equal(bits(got[k]), bits(again[k])), f"{k} differs between two runs"
    compare(f"{MODE_NAME[mode]} {shape}", got, ref, len(params), mode, norm)


@pytest.mark.parametrize("mode", [ROWS, EDGE, NODE], ids=["rows", "edge", "node"])
def test_silu_far_out_stays_finite_and_right(cuda, G, mode):
    """a first-layer bias of +-150 on every third hidden unit: exp(-v) overflows to inf on one side and underflows to 0 on the
    other; value and derivative must be (-0 | 0, -0 | 0) and (v, 1) there -- finite, and float64's to fp32 rounding -- and the
    whole backward still within the bars.  The second layer sums products of magnitude ~40 (rows of value ~150) that cancel to
    pre-activations of order 1, so its derivative rows carry the fp32 rounding of those sums (a few ulp(40) = 4e-6 each): measured
    9.3e-6 (rows), 4.8e-6 (edge), 4.5e-6 (node) against the 1e-5 bar, the closest any figure of this file comes to its bar"""
    shape = (34, 34, 34, 2, 3, True, True, True)
    gen, B, x, v, params, norm, residual, mean, gy = make_case(mode, G, shape, seed=77 + mode, big_bias=True)
    ref = reference(mode, G, B, x, v, params, norm, residual, mean, gy)
    got = raw_run(cuda, gen, mode, G, B, x, v, params, norm, residual, mean, gy)
    h64, d64 = ref[1][0], ref[2][0]
    hi, lo = h64 > 100, (h64.abs() < 1e-30) & (d64.abs() < 1e-30)      # far out: silu(v) = v above, ~ -v exp(v) below
    assert int(hi.sum()) >= h64.shape[0] * 5 and int(lo.sum()) >= h64.shape[0] * 5
    h, dd = got["hid0"].double(), got["der0"].double()
    assert bool((h[lo] == 0).all()) and bool((dd[lo] == 0).all())
    assert bool(((h[hi] - h64[hi]).abs() <= 1e-5 * h64[hi]).all()) and bool((dd[hi] == 1).all())
    rest = ~(hi | lo)
    assert float((h[rest] - h64[rest]).abs().max()) <= 1e-5 * float(h64[rest].abs().max())
    assert float((dd[rest] - d64[rest]).abs().max()) <= 1e-5 * float(d64[rest].abs().max())
    compare(f"{MODE_NAME[mode]} far out", got, ref, len(params), mode, norm)


@pytest.mark.parametrize("rows,cin,cout", [(101, 5, 4), (303, 34, 34), (111, 116, 116), (303, 116, 34), (130, 128, 128)])
def test_dgrad_mul(cuda, rows, cin, cout):
    """out = (dz . W) * mul against float64; with a null multiplier dz . W itself, bit for bit what dlwp_graph_dgrad0 gives in
    rows mode (the same loop) and within the bar of dlwp_conv1x1_dgrad; two launches are bit-identical"""
    from dlwp_benchmark_amd import lib as L
    lib, s = L.load(), L.stream()
    gen = torch.Generator().manual_seed(rows + cin)
    dz, w, mul = torch.randn(rows, cout, generator=gen), torch.randn(cout, cin, generator=gen) / cout ** 0.5, torch.randn(rows, cin, generator=gen)
    dzd, wd, muld = dz.to(cuda), w.to(cuda), mul.to(cuda)
    o = {k: Out((rows, cin), cuda, gen) for k in ("mul", "mul2", "plain", "dgrad0", "conv1x1")}
    L.check(lib.dlwp_graph_dgrad_mul(L.ptr(dzd), L.ptr(wd), L.ptr(muld), L.ptr(o["mul"].t), rows, cin, cout, s))
    L.check(lib.dlwp_graph_dgrad_mul(L.ptr(dzd), L.ptr(wd), L.ptr(muld), L.ptr(o["mul2"].t), rows, cin, cout, s))
    L.check(lib.dlwp_graph_dgrad_mul(L.ptr(dzd), L.ptr(wd), None, L.ptr(o["plain"].t), rows, cin, cout, s))
    L.check(lib.dlwp_graph_dgrad0(ROWS, L.ptr(dzd), L.ptr(wd), None, L.ptr(o["dgrad0"].t), None, None, 1, 0, 0, rows, cin, 0, cout, s))
    L.check(lib.dlwp_conv1x1_dgrad(L.ptr(dzd), L.ptr(wd), L.ptr(o["conv1x1"].t), rows, cin, cout, s))
    torch.cuda.synchronize()
    assert all(b.sentinels_intact() for b in o.values())
    ref = dz.double() @ w.double()
    assert torch.equal(bits(o["mul"].t), bits(o["mul2"].t))
    assert torch.equal(bits(o["plain"].t), bits(o["dgrad0"].t))
    assert torch.equal(bits(o["mul"].t), bits(o["plain"].t * muld))      # one fp32 product on the same sum
    gaps = (rel_gap(o["plain"].t.cpu(), ref), rel_gap(o["mul"].t.cpu(), ref * mul.double()), rel_gap(o["conv1x1"].t.cpu(), ref))
    print(f"dgrad_mul {rows} x {cin} <- {cout}: plain {gaps[0]:.1e}, times mul {gaps[1]:.1e}, conv1x1_dgrad {gaps[2]:.1e}")
    assert max(gaps) <= BAR_OUT


def test_operators_silu_kernel_names_and_no_grad(cuda, G):
    """graph_ops with act="silu": the backward of the later Linears is graph_dgrad_mul (no conv1x1 dgrad, no activation pass),
    ReLU's stays on conv1x1 + act_bwd; under no_grad the launch stores nothing -- the bytes the accounting derives from the
    launch's own arguments drop by exactly the stored rows (2 L hidden + out floats per row: post-activation, derivative,
    normalised) and the call leaves nothing allocated but its output -- and gives the same bits"""
    from dlwp_benchmark_amd import graph_ops, lib as L
    gen = torch.Generator().manual_seed(23)
    lin = lambda o, i: [torch.nn.Parameter((torch.randn(o, i, generator=gen) / i ** 0.5).to(cuda)), torch.nn.Parameter(torch.zeros(o, device=cuda))]      # noqa: E731
    norm = [torch.nn.Parameter(torch.ones(34, device=cuda)), torch.nn.Parameter(torch.zeros(34, device=cuda))]
    e = torch.randn(2 * G.num_edges, 34, generator=gen).to(cuda).requires_grad_(True)
    v = torch.randn(2 * G.num_nodes, 34, generator=gen).to(cuda).requires_grad_(True)
    pr, pe, pn = lin(20, 34) + lin(20, 20) + lin(34, 20), lin(34, 102) + lin(34, 34), lin(34, 68) + lin(34, 34) + lin(34, 34) + lin(34, 34)
    names = {}
    for act in ("silu", "relu"):
        with L.kernel_accounting() as acc:
            x = graph_ops.graph_mlp(v, pr, norm, act=act)
            e2 = graph_ops.edge_block(e, x, G, pe, norm, act=act)
            v2 = graph_ops.node_block(e2, x, G, pn, norm, "mean", act=act)
            (v2.sum() + e2.sum()).backward()
        names[act] = {r["name"]: r["calls"] for r in acc.rows}
    print(names)
    assert names["silu"]["graph_dgrad_mul"] == 2 + 1 + 3 and "conv1x1" not in names["silu"] and "graph_dgrad_mul" not in names["relu"]
    assert names["relu"]["conv1x1"] == 6 and names["silu"]["pixel_wgrad"] == names["relu"]["pixel_wgrad"] == 6
    assert names["silu"]["graph_mlp_rows"] == names["silu"]["graph_mlp_edge"] == names["silu"]["graph_mlp_node"] == 1
    ed, vd = e.detach(), v.detach()
    calls = {"graph_mlp_rows": (lambda: graph_ops.graph_mlp(vd, pr, norm, act="silu"), 2 * G.num_nodes, 2 * 2 * 20 + 34),
             "graph_mlp_edge": (lambda: graph_ops.edge_block(ed, vd, G, pe, norm, act="silu"), 2 * G.num_edges, 2 * 34 + 34),
             "graph_mlp_node": (lambda: graph_ops.node_block(ed, vd, G, pn, norm, "mean", act="silu"), 2 * G.num_nodes, 2 * 3 * 34 + 34)}
    for name, (fn, rows, stored) in calls.items():
        nbytes, held, ys = {}, {}, {}
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
            ys[mode] = y.detach().clone()
            del y, y2
        print(name, nbytes, held)
        assert torch.equal(bits(ys["grad"]), bits(ys["no_grad"]))
        assert nbytes["grad"] - nbytes["no_grad"] == 4.0 * rows * stored, (name, nbytes)
        assert 4 * rows * 34 <= held["no_grad"] < 4 * rows * 34 + 512, (name, held)
        assert held["grad"] >= held["no_grad"] + 4 * rows * stored, (name, held)


def test_silu_argument_errors_are_named(cuda):
    from dlwp_benchmark_amd import graph_ops, lib as L
    lib = L.load()
    t = torch.zeros(70, 8, device=cuda)
    with pytest.raises(L.DlwpError, match="graph_dgrad_mul: NULL"):
        L.check(lib.dlwp_graph_dgrad_mul(None, L.ptr(t), None, L.ptr(t), 70, 8, 8, L.stream()))
    with pytest.raises(L.DlwpError, match=r"graph_dgrad_mul: width \(input 129, output 8\) outside 1\.\.128"):
        L.check(lib.dlwp_graph_dgrad_mul(L.ptr(t), L.ptr(t), None, L.ptr(t), 70, 129, 8, L.stream()))
    with pytest.raises(L.DlwpError, match="graph_dgrad_mul: bad shape"):
        L.check(lib.dlwp_graph_dgrad_mul(L.ptr(t), L.ptr(t), None, L.ptr(t), 0, 8, 8, L.stream()))
    a = L.GraphMlpArgs()
    a.mode, a.rows, a.De, a.hidden, a.out, a.hidden_layers, a.act = 0, 70, 8, 8, 8, 1, 2
    a.x = a.y = a.w[0] = a.w[1] = L.ptr(t)
    with pytest.raises(L.DlwpError, match=r"graph_mlp_fwd: act 2 is neither relu \(0\) nor silu \(1\)"):
        L.check(lib.dlwp_graph_mlp_fwd(ctypes.byref(a), L.stream()))
    a.act = 0
    a.der[0] = L.ptr(t)
    with pytest.raises(L.DlwpError, match="derivative rows 0"):
        L.check(lib.dlwp_graph_mlp_fwd(ctypes.byref(a), L.stream()))
    lin = lambda o, i: [torch.zeros(o, i, device=cuda), torch.zeros(o, device=cuda)]      # noqa: E731
    with pytest.raises(ValueError, match="'relu' or 'silu'"):
        graph_ops.graph_mlp(t, lin(8, 8) + lin(8, 8), act="tanh")
