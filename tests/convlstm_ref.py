"""Plain-torch restatement of the two ConvLSTM baselines (helper module for the tests, not a conftest): CPU ops only,
dtype-generic (the arithmetic runs in the dtype of the parameters), written from the models' description:

* a 3 x 3 convolution pads by one pixel per side, per axis either circularly or with zeros;
* encoder: three convolutions in -> h -> h -> h, tanh after the first two; decoder: one convolution h -> out;
* a cell: ONE convolution over cat(x, h_prev) to 4 h channels, split into (input, i, f, o) blocks of h;
  c = sigmoid(f) c_prev + sigmoid(i) tanh(input), h = sigmoid(o) tanh(c); states start at zero;
* nsbench: circular on both axes, input x[:, t] while t < teacher_forcing_steps, else the previous output; all T outputs;
* dlwpbench: zeros in latitude (H), circular in longitude (W); input cat(constants, prescribed_t, prognostic_t), the output is
  a residual to prognostic_t; teacher forcing while t < context_size; the frames from context_size on.

`params` is a state_dict-like mapping with the reference's keys.
"""
import torch
import torch.nn.functional as F

NS_PAD = ("circular", "circular")
DLWP_PAD = ("zeros", "circular")


def pad1(x, modes):
    """x [B, C, H, W] padded by one pixel per side; modes = (height, width)"""
    if modes[1] == "circular":
        x = torch.cat([x[..., -1:], x, x[..., :1]], dim=-1)
    else:
        x = F.pad(x, (1, 1, 0, 0))
    if modes[0] == "circular":
        x = torch.cat([x[..., -1:, :], x, x[..., :1, :]], dim=-2)
    else:
        x = F.pad(x, (0, 0, 1, 1))
    return x


def conv3x3(x, w, b, modes, act=None):
    y = F.conv2d(pad1(x, modes), w, b)
    if act == "tanh":
        y = torch.tanh(y)
    elif act == "relu":
        y = torch.relu(y)
    return y


def cell(x, h_prev, c_prev, w, b, modes):
    hid = w.shape[0] // 4
    z = conv3x3(torch.cat([x, h_prev], dim=1), w, b, modes)
    zi, ii, ff, oo = torch.split(z, hid, dim=1)
    c = torch.sigmoid(ff) * c_prev + torch.sigmoid(ii) * torch.tanh(zi)
    return torch.sigmoid(oo) * torch.tanh(c), c


def _net(params, x, states, keys, modes):
    enc, cells, dec = keys
    for i, k in enumerate(enc):
        x = conv3x3(x, params[k + ".weight"], params.get(k + ".bias"), modes, "tanh" if i < 2 else None)
    for i, k in enumerate(cells):
        w = params[k + ".weight"]
        if states[i] is None:
            z = x.new_zeros(x.shape[0], w.shape[0] // 4, x.shape[2], x.shape[3])
            states[i] = (z, z)
        states[i] = cell(x, states[i][0], states[i][1], w, params.get(k + ".bias"), modes)
        x = states[i][0]
    return conv3x3(x, params[dec + ".weight"], params.get(dec + ".bias"), modes)


def _count_cells(params, fmt):
    n = 0
    while fmt.format(n) + ".weight" in params:
        n += 1
    return n


def ns_forward(params, x, teacher_forcing_steps):
    """x [B, T, 1, H, W] -> [B, T, D, H, W]"""
    n = _count_cells(params, "clstm.{}.conv")
    keys = (["encoder.0", "encoder.2", "encoder.4"], [f"clstm.{i}.conv" for i in range(n)], "decoder.0")
    states, outs, out = [None] * n, [], None
    for t in range(x.shape[1]):
        out = _net(params, x[:, t] if t < teacher_forcing_steps else out, states, keys, NS_PAD)
        outs.append(out)
    return torch.stack(outs, dim=1)


def dlwp_forward(params, constants, prescribed, prognostic, context_size):
    """constants [B, 1, C, H, W] | None, prescribed [B, T, C, H, W] | None, prognostic [B, T, C, H, W] -> [B, T - ctx, C, H, W]"""
    n = _count_cells(params, "clstm.{}.conv.1")
    keys = (["encoder.1", "encoder.4", "encoder.7"], [f"clstm.{i}.conv.1" for i in range(n)], "decoder.1")
    states, outs, frame = [None] * n, [], None
    for t in range(prognostic.shape[1]):
        prog_t = prognostic[:, t] if t < context_size else frame
        parts = ([constants[:, 0]] if constants is not None else []) + ([prescribed[:, t]] if prescribed is not None else [])
        frame = prog_t + _net(params, torch.cat(parts + [prog_t], dim=1), states, keys, DLWP_PAD)
        outs.append(frame)
    return torch.stack(outs[context_size:], dim=1)


def rel_gap(a, ref):
    """max |a - ref| relative to the max norm of ref (the measure of every bound of the ConvLSTM tests)"""
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def run_case(kind, params, inputs, target, dtype, **cfg):
    """forward + mse loss + backward in `dtype`; returns (output, loss, {name: gradient}) as tensors of that dtype"""
    p = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}
    cast = lambda v: None if v is None else torch.as_tensor(v).to(dtype)      # noqa: E731
    if kind == "ns":
        y = ns_forward(p, cast(inputs["x"]), cfg["teacher_forcing_steps"])
    else:
        y = dlwp_forward(p, cast(inputs.get("constants")), cast(inputs.get("prescribed")), cast(inputs["prognostic"]),
                         cfg["context_size"])
    loss = F.mse_loss(y, cast(target))
    loss.backward()
    return y.detach(), loss.detach(), {k: v.grad for k, v in p.items()}


# the golden cases: name -> (kind, constructor keywords, B, T, rollout keyword)
CASES = {
    "ns_13x4": ("ns", dict(input_size=1, hidden_sizes=[13, 13, 13, 13], height=16, width=16), 2, 12, dict(teacher_forcing_steps=6)),
    "ns_16x2": ("ns", dict(input_size=1, hidden_sizes=[16, 16], height=16, width=24), 3, 10, dict(teacher_forcing_steps=4)),
    "ns_5_tf4": ("ns", dict(input_size=1, hidden_sizes=[5], height=8, width=8), 1, 4, dict(teacher_forcing_steps=4)),
    "ns_5_tf1": ("ns", dict(input_size=1, hidden_sizes=[5], height=8, width=8), 1, 4, dict(teacher_forcing_steps=1)),
    "dlwp_16x2": ("dlwp", dict(constant_channels=4, prescribed_channels=1, prognostic_channels=8, hidden_sizes=[16, 16], height=16,
                               width=32, context_size=1), 1, 5, dict(context_size=1)),
    "dlwp_8x3": ("dlwp", dict(constant_channels=4, prescribed_channels=0, prognostic_channels=8, hidden_sizes=[8, 8, 8], height=8,
                              width=16, context_size=2), 2, 6, dict(context_size=2)),
}
GOLDEN = {"ns": "convlstm_ns_golden.npz", "dlwp": "convlstm_dlwp_golden.npz"}


def make_inputs(kind, cfg, B, T, gen):
    """fresh random inputs and target of a case (the fixtures store their own)"""
    H, W = cfg["height"], cfg["width"]
    if kind == "ns":
        return {"x": torch.randn(B, T, 1, H, W, generator=gen)}, torch.randn(B, T, cfg["input_size"], H, W, generator=gen)
    inp = {"constants": torch.randn(B, 1, cfg["constant_channels"], H, W, generator=gen),
           "prognostic": torch.randn(B, T, cfg["prognostic_channels"], H, W, generator=gen)}
    if cfg["prescribed_channels"]:
        inp["prescribed"] = torch.randn(B, T, cfg["prescribed_channels"], H, W, generator=gen)
    return inp, torch.randn(B, T - cfg["context_size"], cfg["prognostic_channels"], H, W, generator=gen)


def load_case(npz, name):
    """(params, inputs, target, y, loss, grads, gaps) of a golden case, as torch tensors"""
    pre = name + "/"
    params = {k[len(pre) + 2:]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(pre + "p_")}
    grads = {k[len(pre) + 2:]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(pre + "g_")}
    inputs = {k[len(pre) + 3:]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(pre + "in_")}
    gaps = {k[len(pre) + 4:]: float(npz[k]) for k in npz.files if k.startswith(pre + "gap_")}
    return (params, inputs, torch.from_numpy(npz[pre + "target"]), torch.from_numpy(npz[pre + "y"]), float(npz[pre + "loss"]), grads,
            gaps)
