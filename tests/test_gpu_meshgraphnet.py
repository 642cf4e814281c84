"""The two MeshGraphNet models on the MI355X against the reference's golden vectors (tests/golden/make_mgn_golden.py) and against
the plain-torch helper (tests/mgn_ref.py) in float64.

Bars (rel_gap: max |difference| relative to the max norm of the reference array): output 1e-4, loss 1e-4, every gradient tensor
5e-4 -- the project's fp32 bars (tests/test_gpu_unet.py, DESIGN.md "Tolerances"); by the fixture's own assertion they sit 10 x
above what the reference's fp32 arithmetic itself scatters around its float64 result (1e-5 / 5e-5).
"""
import json
import os

import numpy as np
import pytest
import torch

from mgn_ref import CASES, GOLDEN, _dlwp, _ns, _widths, load_case, make_inputs, rel_gap, run_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BAR_OUT, BAR_LOSS, BAR_GRAD = 1e-4, 1e-4, 5e-4

# fresh cases beyond the fixtures: a multi-lead-time dlwpbench rollout (the reference itself raises there), dlwpbench's published
# width 116 with processor_size 4, and the reference's default width 128
FRESH = {
    "dlwp_grid_4x8_c2_T5": ("dlwp", _dlwp("grid_2d", 4, 8, (False, True), 2, 1, 3, 2, 2, _widths(12)), (2, 5, 4, 8), {}),
    "dlwp_delaunay_6x8_d116": ("dlwp", _dlwp("delaunay", 6, 8, True, 4, 1, 8, 1, 4, _widths(116)), (1, 3, 6, 8), {}),
    "ns_8stencil_5x6_d128": ("ns", _ns("grid_2d_8stencil", 5, 6, True, 2, 1, _widths(128), num_layers_edge_processor=3),
                             (2, 4, 5, 6), dict(teacher_forcing_steps=2)),
}


def build(kind, cfg, params, dev):
    from dlwp_benchmark_amd import dlwpbench, nsbench
    net = (nsbench if kind == "ns" else dlwpbench).MeshGraphNet(**cfg)
    net.load_state_dict({k: v.float() for k, v in params.items()}, strict=True)
    return net.to(dev)


def forward(net, kind, inputs, roll, dev):
    if kind == "ns":
        return net(inputs["x"].to(dev), **roll)
    opt = lambda k: inputs[k].to(dev) if k in inputs else None      # noqa: E731
    return net(constants=opt("constants"), prescribed=opt("prescribed"), prognostic=inputs["prognostic"].to(dev))


def train_once(net, kind, inputs, target, roll, dev):
    net.zero_grad(set_to_none=True)
    y = forward(net, kind, inputs, roll, dev)
    loss = torch.nn.functional.mse_loss(y, target.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), loss.item(), {n: p.grad.detach().cpu() for n, p in net.named_parameters()}


def compare(tag, got, ref):
    y, loss, grads = got
    ry, rloss, rgrads = ref
    assert y.shape == ry.shape
    g = rel_gap(y, ry)
    gl = abs(loss - float(rloss)) / abs(float(rloss))
    gg = {k: rel_gap(grads[k], rgrads[k]) for k in rgrads}
    worst = max(gg, key=gg.get)
    print(f"{tag}: output {g:.2e}, loss {gl:.2e}, worst gradient {gg[worst]:.2e} ({worst})")
    assert set(grads) == set(rgrads)
    assert g <= BAR_OUT, (tag, g)
    assert gl <= BAR_LOSS, (tag, gl)
    assert gg[worst] <= BAR_GRAD, (tag, worst, gg[worst])


@pytest.mark.parametrize("name", list(CASES))
def test_golden_case(cuda, name):
    kind, cfg, shape, roll = CASES[name]
    params, inputs, target, y, loss, grads, _, _ = load_case(np.load(os.path.join(HERE, "golden", GOLDEN[kind])), name)
    net = build(kind, cfg, params, cuda)
    compare(name, train_once(net, kind, inputs, target, roll, cuda), (y, loss, grads))


def helper_reference(kind, params, inputs, target, cfg, roll):
    """the helper in float64, after asserting that its own fp32 run is within 1e-5 / 5e-5 of it (a property of the model at
    this size and parameter scale, not of the kernels: a case that misses it cannot pin anything)"""
    y64, l64, g64 = run_case(kind, params, inputs, target, torch.float64, cfg, roll)
    y32, l32, g32 = run_case(kind, params, inputs, target, torch.float32, cfg, roll)
    gap_y, gap_l = rel_gap(y32, y64), rel_gap(l32, l64)
    gap_g = max(rel_gap(g32[k], g64[k]) for k in g64)
    print(f"helper fp32 vs float64: output {gap_y:.2e}, loss {gap_l:.2e}, gradients {gap_g:.2e}")
    assert gap_y <= 1e-5 and gap_l <= 1e-5 and gap_g <= 5e-5, (gap_y, gap_l, gap_g)
    return y64, float(l64), g64


def fresh_params(kind, cfg, seed):
    """default initialisation with ALL parameters perturbed, as the golden script does"""
    from dlwp_benchmark_amd import dlwpbench, nsbench
    torch.manual_seed(seed)
    net = (nsbench if kind == "ns" else dlwpbench).MeshGraphNet(**cfg)
    gen = torch.Generator().manual_seed(seed + 1)
    return {k: (v.detach() + 0.2 * torch.randn(v.shape, generator=gen) if v.dim() == 1 else v.detach() * 1.5)
            for k, v in net.state_dict().items()}


@pytest.mark.parametrize("name", list(CASES) + list(FRESH))
def test_fresh_inputs_against_the_helper(cuda, name):
    kind, cfg, shape, roll = (CASES.get(name) or FRESH[name])
    params = fresh_params(kind, cfg, seed=sum(map(ord, name)))
    inputs, target = make_inputs(kind, cfg, shape, torch.Generator().manual_seed(len(name) + 99))
    ref = helper_reference(kind, params, inputs, target, cfg, roll)
    net = build(kind, cfg, params, cuda)
    compare(name, train_once(net, kind, inputs, target, roll, cuda), ref)


@pytest.mark.parametrize("name", ["ns_grid_3x5_c2", "dlwp_delaunay_4x8_c2"])
def test_state_dict_eval_and_other_batch_size(cuda, name):
    kind, cfg, (B, T, H, W), roll = CASES[name]
    params, inputs, target, y, loss, grads, _, _ = load_case(np.load(os.path.join(HERE, "golden", GOLDEN[kind])), name)
    net = build(kind, cfg, params, cuda)                                   # load_state_dict(strict=True) inside
    sd = net.state_dict()
    assert list(sd) == list(params) and all(torch.equal(sd[k].cpu(), params[k]) for k in params)
    net2 = build(kind, cfg, {k: v.cpu() for k, v in sd.items()}, cuda)      # round trip
    net.train()
    y_train = forward(net, kind, inputs, roll, cuda).detach()
    net2.eval()
    with torch.no_grad():
        y_eval = forward(net2, kind, inputs, roll, cuda)
    assert not y_eval.requires_grad
    assert torch.equal(y_train.view(torch.int32), y_eval.view(torch.int32))      # bit for bit
    # the samples are independent: the doubled batch reproduces the original one in both halves (a batch size that changes
    # between two calls of the same model)
    big = {k: torch.cat([v, v], 0) for k, v in inputs.items()}
    with torch.no_grad():
        y_big = forward(net2, kind, big, roll, cuda)
    assert y_big.shape[0] == 2 * y_eval.shape[0]
    assert torch.equal(y_big[:B].view(torch.int32), y_eval.view(torch.int32)) and torch.equal(y_big[B:].view(torch.int32), y_eval.view(torch.int32))
    assert rel_gap(y_big[:B].cpu(), y) <= BAR_OUT
    one = {k: v[:1] for k, v in inputs.items()}
    with torch.no_grad():
        y_one = forward(net2, kind, one, roll, cuda)
    assert rel_gap(y_one.cpu(), y[:1]) <= BAR_OUT
    with torch.no_grad():                                                     # and back to the first batch size
        assert torch.equal(forward(net2, kind, inputs, roll, cuda).view(torch.int32), y_eval.view(torch.int32))


def test_graphed_train_step_matches_eager(cuda):
    """GraphedTrainStep (flat parameters, gradients accumulated in place by the kernels, hipGraph replay) of the nsbench model
    over three steps on changing batches against the eager sequence of the same steps (autograd accumulation + torch Adam):
    losses within 2e-4 relative, parameters within 2e-4 -- the bars of tests/test_gpu_train_engine.py for this comparison."""
    from dlwp_benchmark_amd import nsbench
    from dlwp_benchmark_amd.train_engine import GraphedTrainStep, mse_loss
    cfg = _ns("grid_2d", 6, 10, True, 2, 2, _widths(13, 9, 7, 11), message_passing_steps=2)
    g = torch.Generator().manual_seed(21)
    batches = [torch.randn(2, 7, 1, 6, 10, generator=g).to(cuda) for _ in range(3)]
    call = lambda m, kw: m(kw["x"], 3)      # noqa: E731

    def make():
        torch.manual_seed(8)
        return nsbench.MeshGraphNet(**cfg).to(cuda).train()

    ref = make()
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    ref_losses = []
    for u in batches:
        opt.zero_grad(set_to_none=True)
        loss = mse_loss(ref(u[:, :-1].contiguous(), 3), u[:, 1:].contiguous())
        loss.backward()
        opt.step()
        ref_losses.append(loss.item())
    for use_graph in (False, True):
        model = make()
        u0 = batches[0]
        step = GraphedTrainStep(model, {"x": u0[:, :-1].contiguous()}, u0[:, 1:].contiguous(), lr=1e-3, use_graph=use_graph, call=call)
        losses = [step({"x": u[:, :-1].contiguous()}, u[:, 1:].contiguous()).item() for u in batches]
        print("graph" if use_graph else "eager-flat", losses, ref_losses)
        for a, b in zip(losses, ref_losses):
            assert abs(a - b) <= 2e-4 * abs(b), (use_graph, losses, ref_losses)
        for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
            assert (p - q).abs().max().item() <= 2e-4, (use_graph, n)


with open(os.path.join(HERE, "golden", "shipped_mgn_model_configs.json")) as f:
    SHIPPED = json.load(f)


@pytest.mark.parametrize("key", sorted(SHIPPED))
def test_shipped_config_constructs_and_trains_one_step(cuda, key):
    """nsbench at 64 x 64, B = 1, T = 12 (context 10); dlwpbench at its delaunay 32 x 64, T = 2 (context 1)"""
    from dlwp_benchmark_amd import dlwpbench, nsbench
    app, _ = key.split("/")
    kw = dict(SHIPPED[key]["kwargs"])
    H, W = SHIPPED[key]["grid"]
    model = getattr(nsbench if app == "nsbench" else dlwpbench, kw["type"])(device=cuda, **kw).train()
    assert next(model.parameters()).device.type == "cuda"
    g = torch.Generator().manual_seed(6)
    ctx = int(kw["context_size"])
    if app == "nsbench":
        x = torch.randn(1, ctx + 2, kw["input_dim_nodes"], H, W, generator=g).to(cuda)
        y = torch.randn(1, ctx + 2, kw["output_dim"], H, W, generator=g).to(cuda)
        out = model(x, teacher_forcing_steps=ctx + 1)
    else:
        T = ctx + 1
        c = torch.randn(1, 1, kw["constant_channels"], H, W, generator=g).to(cuda)
        p = torch.randn(1, T, kw["prescribed_channels"], H, W, generator=g).to(cuda)
        x = torch.randn(1, T, kw["prognostic_channels"], H, W, generator=g).to(cuda)
        y = torch.randn(1, T - ctx, kw["prognostic_channels"], H, W, generator=g).to(cuda)
        out = model(constants=c, prescribed=p, prognostic=x)
    assert out.shape == y.shape and torch.isfinite(out).all()
    torch.nn.functional.mse_loss(out, y).backward()
    for n, p_ in model.named_parameters():
        assert p_.grad is not None and torch.isfinite(p_.grad).all() and p_.grad.abs().max().item() > 0, n
