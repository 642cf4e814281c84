"""The wide, bipartite graph kernels (csrc/graph_wide.hip, graph_ops.wide_*) against the float64 torch restatement on the CPU
(tests/graph_wide_ref.py), on a hand-made bipartite graph: 23 sources, 17 destinations, 65 edges in no order, a destination without
in-edges, a source without out-edges, nodes that occur in no edge, a duplicate edge, in-degree >= 9.  With B in {1, 2} the edge rows
(65, 130) and node rows (17, 34) are no multiples of the 64-row tile; the rows mode runs 1, 63, 64, 65, 130 and 1030 rows (1030:
more rows than the LayerNorm backward's 256 workgroups x 4 waves take in one pass, and a weight gradient split over 17 row tiles).

Bars (`rel_gap`: max |difference| relative to the max norm of the float64 array), those of tests/test_gpu_graph_ops.py: 1e-5 for
the output and every stored row, 5e-5 for every gradient.  The MFMA path is exact fp32 (an fma chain: about 1e-7 sum |a b| up to
K = 1536); SiLU adds one hardware exp and one division.
"""
import ctypes

import pytest
import torch

from graph_wide_ref import EDGE, NODE, ROWS, bipartite_handmade, mlp64
from mgn_ref import rel_gap

pytestmark = pytest.mark.gpu

BAR_OUT, BAR_GRAD = 1e-5, 5e-5


@pytest.fixture(scope="module")
def G(cuda):
    from dlwp_benchmark_amd.graph_ops import BipartiteGraph
    src, dst, ns, nd = bipartite_handmade()
    return BipartiteGraph(src, dst, ns, nd, device=cuda)


def make(seed, mode, B, widths, hidden, out, nl, norm, dev, rows=None):
    """seeded operands and nn.Linear-scaled parameters; widths = (D0, D1, D2)"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    _, _, ns, nd = bipartite_handmade()
    D0, D1, D2 = widths
    if mode == ROWS:
        x, vs, vd, k0, R = rn(rows, D0), None, None, D0, rows
    elif mode == EDGE:
        x, vs, vd, k0, R = rn(B * 65, D0), rn(B * ns, D1), rn(B * nd, D2), D0 + D1 + D2, B * 65
    else:
        x, vs, vd, k0, R = rn(B * 65, D0), None, rn(B * nd, D1), D0 + D1, B * nd
    params, fan = [], k0
    for i in range(nl + 1):
        n = out if i == nl else hidden
        params += [(torch.rand(n, fan, generator=gen) * 2 - 1) / fan ** 0.5, (torch.rand(n, generator=gen) * 2 - 1) / fan ** 0.5]
        fan = hidden
    nrm = [1 + 0.5 * rn(out), 0.5 * rn(out)] if norm else None
    gy = rn(R, out)
    cu = lambda t: None if t is None else t.to(dev)      # noqa: E731
    return dict(x=cu(x), vs=cu(vs), vd=cu(vd), params=[cu(p) for p in params], norm=None if nrm is None else [cu(t) for t in nrm],
                gy=cu(gy))


def run_public(mode, G, d, residual, mean, act, same=False):
    """the public functions with autograd -> (y, grads)"""
    from dlwp_benchmark_amd import graph_ops as go
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)      # noqa: E731
    x, vs, params = leaf(d["x"]), leaf(d["vs"]), [leaf(p) for p in d["params"]]
    vd = vs if same else leaf(d["vd"])
    norm = [leaf(t) for t in d["norm"]] if d["norm"] is not None else None
    if mode == ROWS:
        y = go.wide_graph_mlp(x, params, norm, act=act, residual=residual)
    elif mode == EDGE:
        y = go.wide_edge_block(x, vs, vd, G, params, norm, residual=residual, act=act)
    else:
        y = go.wide_node_block(x, vd, G, params, norm, aggregation="mean" if mean else "sum", residual=residual, act=act)
    y.backward(d["gy"])
    g = {"x": x.grad, "vs": None if vs is None else vs.grad, "vd": None if (vd is None or same) else vd.grad}
    g.update({f"p{i}": p.grad for i, p in enumerate(params)})
    if norm is not None:
        g.update(gamma=norm[0].grad, beta=norm[1].grad)
    return y.detach(), g


def check(mode, G, d, B, residual, mean, act, what):
    """output, every stored row and every gradient against float64; two identical launches bit-equal; nothing stored under no_grad"""
    from dlwp_benchmark_amd import graph_ops as go
    graph = bipartite_handmade()
    y64, st64, g64 = mlp64(mode, graph, B, d["x"], d["vs"], d["vd"], d["params"], d["norm"], residual, mean, act, d["gy"])
    code = go._act_code(act)
    with torch.no_grad():
        y, st = go.wide_forward(mode, G, mean, residual, code, d["x"], d["vs"], d["vd"], d["norm"], d["params"], True)
        y2, st2 = go.wide_forward(mode, G, mean, residual, code, d["x"], d["vs"], d["vd"], d["norm"], d["params"], False)
    assert st2 == {}, "under no_grad nothing is stored"
    assert torch.equal(y, y2)
    worst = {"y": rel_gap(y.cpu(), y64)}
    for l, h in enumerate(st64["hid"]):
        worst[f"hid{l}"] = rel_gap(st["hid"][l].cpu(), h)
    assert len(st["der"]) == len(st64["der"])
    for l, h in enumerate(st64["der"]):
        worst[f"der{l}"] = rel_gap(st["der"][l].cpu(), h)
    for k in ("xhat", "rstd", "agg"):
        assert (st[k] is None) == (st64[k] is None), k
        if st64[k] is not None:
            worst[k] = rel_gap(st[k].cpu(), st64[k])
    yp, g = run_public(mode, G, d, residual, mean, act)
    assert torch.equal(yp, y), "the autograd path runs the same launches"
    yp2, g2 = run_public(mode, G, d, residual, mean, act)
    gworst = {}
    for k, ref in g64.items():
        assert (g[k] is None) == (ref is None), k
        if ref is None:
            continue
        assert torch.equal(g[k], g2[k]), f"{k}: two identical launches differ"
        gworst[k] = rel_gap(g[k].cpu(), ref)
    print(f"{what}: out/stored {max(worst.values()):.2e} ({max(worst, key=worst.get)}), grads {max(gworst.values()):.2e} "
          f"({max(gworst, key=gworst.get)})")
    assert max(worst.values()) <= BAR_OUT, worst
    assert max(gworst.values()) <= BAR_GRAD, gworst


@pytest.mark.parametrize("norm,residual", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("nl", [1, 3])
@pytest.mark.parametrize("act", ["silu", "relu"])
@pytest.mark.parametrize("mode", [ROWS, EDGE, NODE])
def test_modes_activations_depths(cuda, G, mode, act, nl, norm, residual):
    """every mode x activation x depth x (norm, residual) at width 16, B = 2 (130 edge rows, 34 node rows; 65 rows)"""
    widths = {ROWS: (16, 0, 0), EDGE: (16, 5, 7), NODE: (9, 16, 0)}[mode]
    d = make(100 + 7 * mode + nl, mode, 2, widths, 16, 16, nl, norm, cuda, rows=65)
    check(mode, G, d, 2, residual, mode == NODE and nl == 3, act, f"mode {mode} {act} L{nl} norm {norm} res {residual}")


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130, 1030])
def test_row_counts(cuda, G, rows):
    d = make(rows, ROWS, 1, (4, 0, 0), 16, 16, 2, True, cuda, rows=rows)
    check(ROWS, G, d, 1, False, False, "silu", f"{rows} rows")


# (mode, B, (D0, D1, D2), hidden, out, layers, norm, residual, mean, act): column-block edges and tails (129, 257, 512), fan-in 3, 4,
# 130 and 1536, part widths that differ
WIDE_CASES = [
    (ROWS, 1, (3, 0, 0), 129, 257, 1, False, False, False, "silu"),
    (ROWS, 1, (4, 0, 0), 257, 129, 2, True, False, False, "relu"),
    (ROWS, 1, (130, 0, 0), 512, 130, 1, True, True, False, "silu"),
    (EDGE, 2, (512, 512, 512), 512, 512, 1, True, True, False, "silu"),
    (EDGE, 1, (5, 129, 16), 129, 5, 3, True, True, False, "relu"),
    (NODE, 2, (512, 512, 0), 257, 512, 1, True, True, True, "silu"),
    (NODE, 1, (130, 64, 0), 64, 64, 2, False, True, False, "silu"),
]


@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: f"m{c[0]}-B{c[1]}-{'x'.join(map(str, c[2]))}-h{c[3]}-o{c[4]}-L{c[5]}")
def test_widths_and_fan_in(cuda, G, case):
    mode, B, widths, hidden, out, nl, norm, residual, mean, act = case
    d = make(hidden + out, mode, B, widths, hidden, out, nl, norm, cuda, rows=65)
    check(mode, G, d, B, residual, mean, act, str(case))


def test_one_node_set(cuda):
    """a graph over ONE node set (the multimesh): the same tensor on both sides, its gradient the sum of both gathers"""
    from dlwp_benchmark_amd.graph_ops import BipartiteGraph
    from test_gpu_graph_ops import handmade
    src, dst, n = handmade()
    g = BipartiteGraph(src, dst, n, n, device=cuda)
    gen = torch.Generator().manual_seed(3)
    D = 129
    d = dict(x=torch.randn(2 * 101, D, generator=gen).to(cuda), vs=torch.randn(2 * n, D, generator=gen).to(cuda), vd=None, norm=None,
             gy=torch.randn(2 * 101, D, generator=gen).to(cuda),
             params=[((torch.rand(s, generator=gen) * 2 - 1) / (3 * D) ** 0.5).to(cuda) for s in ((D, 3 * D), (D,), (D, D), (D,))])
    y64, _, g64 = mlp64(EDGE, (src, dst, n, n), 2, d["x"], d["vs"], None, d["params"], None, True, False, "silu", d["gy"], same=True)
    y, gr = run_public(EDGE, g, d, True, False, "silu", same=True)
    gaps = {k: rel_gap(gr[k].cpu(), v) for k, v in g64.items() if v is not None}
    print(f"one node set: y {rel_gap(y.cpu(), y64):.2e}, grads {max(gaps.values()):.2e}")
    assert rel_gap(y.cpu(), y64) <= BAR_OUT
    assert max(gaps.values()) <= BAR_GRAD, gaps


@pytest.mark.parametrize("mode", [EDGE, NODE])
def test_batch_of_two_is_two_singles(cuda, G, mode):
    """B = 2 is two independent samples on the same graph: outputs and input gradients bit for bit those of two B = 1 runs; the
    parameter gradients are the two runs' sums (another order of the same fp32 sums: the gradient bar against their float64 sum)"""
    widths = {EDGE: (129, 16, 33), NODE: (33, 129, 0)}[mode]
    d = make(5, mode, 2, widths, 129, 129, 2, True, cuda)
    y, g = run_public(mode, G, d, True, mode == NODE, "silu")
    _, _, ns, nd = bipartite_handmade()
    per = {"x": 65, "vs": ns, "vd": nd, "gy": 65 if mode == EDGE else nd}
    halves = []
    for b in range(2):
        h = dict(d)
        for k, n in per.items():
            h[k] = None if d[k] is None else d[k][b * n:(b + 1) * n].contiguous()
        halves.append(run_public(mode, G, h, True, mode == NODE, "silu"))
    assert torch.equal(y, torch.cat([halves[0][0], halves[1][0]]))
    for k in ("x", "vs", "vd"):
        if g[k] is not None:
            assert torch.equal(g[k], torch.cat([halves[0][1][k], halves[1][1][k]])), k
    for k in g:
        if k.startswith("p") or k in ("gamma", "beta"):
            assert rel_gap(g[k].cpu(), halves[0][1][k].double().cpu() + halves[1][1][k].double().cpu()) <= BAR_GRAD, k


def test_no_grad_allocates_the_output_only(cuda, G):
    """under no_grad the public call leaves nothing behind but its output (no hidden, derivative or normalised rows)"""
    from dlwp_benchmark_amd import graph_ops as go
    d = make(9, EDGE, 2, (64, 64, 64), 512, 64, 3, True, cuda)
    params = [p.clone().requires_grad_(True) for p in d["params"]]
    norm = [t.clone().requires_grad_(True) for t in d["norm"]]
    run = lambda: go.wide_edge_block(d["x"], d["vs"], d["vd"], G, params, norm, residual=True, act="silu")      # noqa: E731
    y_train = run()
    assert y_train.grad_fn is not None
    del y_train
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        y = run()
    torch.cuda.synchronize()
    assert y.grad_fn is None
    extra = torch.cuda.memory_allocated() - before
    assert extra <= y.numel() * 4 + 1024, f"{extra} bytes kept for an output of {y.numel() * 4}"      # one hidden row block is 266240
    assert torch.equal(y, run().detach())


def test_cpu_tensors_are_refused():
    from dlwp_benchmark_amd import graph_ops as go
    from dlwp_benchmark_amd.lib import DlwpError
    w = [torch.zeros(8, 4), torch.zeros(8), torch.zeros(4, 8), torch.zeros(4)]
    with pytest.raises(DlwpError, match="no CPU path"):
        go.wide_graph_mlp(torch.zeros(5, 4), w)


def test_abi_errors_name_the_argument(cuda):
    """host-side refusals of the raw entry points: a NULL pointer, width 513, a bad shape -- before anything is launched (every
    pointer handed over is a real device buffer larger than any shape named here)"""
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    err = lambda: lib.dlwp_last_error().decode()      # noqa: E731
    buf = torch.zeros(8192, device=cuda)
    idx = torch.zeros(64, dtype=torch.int32, device=cuda)
    p, q = buf.data_ptr(), idx.data_ptr()
    op = L.GraphWideOperand()
    op.mode, op.rows, op.D0, op.x = ROWS, 5, 4, p
    assert lib.dlwp_graph_wide_linear_fwd(ctypes.byref(op), None, None, None, p, None, 8, 0, None) != 0
    assert "NULL argument (w or y)" in err()
    assert lib.dlwp_graph_wide_linear_fwd(ctypes.byref(op), p, None, None, p, None, 513, 0, None) != 0
    assert "513" in err() and "1..512" in err()
    op.D0 = 513
    assert lib.dlwp_graph_wide_wgrad0_ws_floats(ctypes.byref(op), 8) < 0
    assert "width 513" in err()
    op.D0, op.rows = 4, 0
    assert lib.dlwp_graph_wide_dgrad(ctypes.byref(op), p, p, None, None, 0, p, None, None, 8, None) != 0
    assert "bad shape (0 rows)" in err()
    op.mode, op.B, op.Ns, op.Nd, op.E, op.D1, op.D2 = EDGE, 1, 3, 0, 4, 4, 4
    assert lib.dlwp_graph_wide_linear_fwd(ctypes.byref(op), p, None, None, p, None, 8, 0, None) != 0
    assert "bad shape" in err() and "0 destination nodes" in err()
    assert lib.dlwp_graph_wide_ln_fwd(None, p, p, None, p, None, None, 4, 8, 1e-5, None) != 0 and "NULL" in err()
    assert lib.dlwp_graph_wide_ln_bwd_ws_floats(4, 513) < 0 and "513" in err()
    assert lib.dlwp_graph_wide_gather_sum(p, q, q, 0, None, p, 1, 3, 4, 513, None) != 0 and "width 513" in err()
    assert lib.dlwp_graph_wide_edge_gather(p, None, None, None, p, 1, 3, 4, 8, None) != 0 and "NULL" in err()
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0, "a refused call wrote nothing"
