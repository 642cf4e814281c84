"""Plain-torch restatement of the two U-Net baselines (helper module for the tests, not a conftest): CPU ops only, dtype-generic
(the arithmetic runs in the dtype of the parameters), written from the models' description:

* a level is a run of 3 x 3 convolutions (one pixel of padding per side, per axis circular or zeros), each followed by the
  activation (relu or tanh).  Every level runs `n_convolutions` of them except the bottom one, which runs `n_convolutions // 2`
  in the encoder and as many in the decoder;
* encoder: below the top level a 2 x 2 average pool (stride 2) comes first; the output of every level is kept;
* decoder, bottom to top: above the bottom the input of a level is cat(encoder output of that level, upsampled); below the top
  a level ends in a 2 x 2 stride-2 transposed convolution to the width of the level above; a 1 x 1 convolution maps the top
  level to the output channels;
* nsbench: padding as configured on both axes.  At step t the window is x[:, max(0, t - ctx + 1) : t + 1] while
  t < teacher_forcing_steps; afterwards, with ts = max(0, teacher_forcing_steps - t - 1 + ctx), the last ts observed frames
  before teacher_forcing_steps followed by the last ctx - ts outputs.  While t < ctx - 1 the output is the newest frame of the
  window; otherwise newest frame + network(window flattened over (time, channel)).  All T outputs;
* dlwpbench: zeros in latitude (H), circular in longitude (W).  For t in [ctx, T): prognostic window = prognostic[:, 0:ctx] at
  t = ctx, afterwards cat(prognostic[:, t - ctx : ctx], the last ctx outputs); input = cat(constants[:, 0],
  prescribed[:, t - ctx : t] flattened, window flattened); output = newest window frame + network(input).

`params` is a state_dict-like mapping with the reference's keys; the layer structure is read from the keys.
"""
import torch
import torch.nn.functional as F

from convlstm_ref import DLWP_PAD, conv3x3, rel_gap  # noqa: F401  (rel_gap is re-exported for the tests)


def _indices(params, prefix):
    """sorted Sequential indices with a weight under `prefix`"""
    idx = {int(k[len(prefix):].split(".")[0]) for k in params if k.startswith(prefix) and k.endswith(".weight")}
    return sorted(idx)


def _levels(params, side):
    n = 0
    while any(k.startswith(f"{side}.layers.{n}.") for k in params):
        n += 1
    return n


def network(params, x, modes, act):
    """x [B, C, H, W] -> [B, out, H, W]"""
    levels = _levels(params, "encoder")
    skips = []
    for lvl in range(levels):
        if lvl > 0:
            x = F.avg_pool2d(x, 2, 2)
        pre = f"encoder.layers.{lvl}."
        for i in _indices(params, pre):
            x = conv3x3(x, params[f"{pre}{i}.weight"], params.get(f"{pre}{i}.bias"), modes, act)
        skips.append(x)
    skips = skips[::-1]
    for lvl in range(levels):
        if lvl > 0:
            x = torch.cat([skips[lvl], x], dim=1)
        pre = f"decoder.layers.{lvl}."
        for i in _indices(params, pre):
            w, b = params[f"{pre}{i}.weight"], params.get(f"{pre}{i}.bias")
            if w.shape[-1] == 3:
                x = conv3x3(x, w, b, modes, act)
            else:
                x = F.conv_transpose2d(x, w, b, stride=2)
    return F.conv2d(x, params["decoder.output_layer.weight"], params.get("decoder.output_layer.bias"))


def ns_forward(params, x, teacher_forcing_steps, context_size, padding_mode, act):
    """x [B, T, D, H, W] -> [B, T, D, H, W]"""
    ctx, tf, modes = context_size, teacher_forcing_steps, (padding_mode, padding_mode)
    outs = []
    for t in range(x.shape[1]):
        if t < tf:
            win = x[:, max(0, t - (ctx - 1)):t + 1]
        else:
            ts = max(0, (tf - t - 1) + ctx)
            win = torch.cat([x[:, tf - ts:tf], torch.stack(outs[-(ctx - ts):], dim=1)], dim=1)
        out = win[:, -1] if t < ctx - 1 else win[:, -1] + network(params, win.flatten(1, 2), modes, act)
        outs.append(out)
    return torch.stack(outs, dim=1)


def dlwp_forward(params, constants, prescribed, prognostic, context_size, act):
    """constants [B, 1, C, H, W] | None, prescribed [B, T, C, H, W] | None, prognostic [B, T, C, H, W] -> [B, T - ctx, C, H, W]"""
    ctx, outs = context_size, []
    for t in range(ctx, prognostic.shape[1]):
        if t == ctx:
            win = prognostic[:, 0:ctx]
        else:
            win = torch.cat([prognostic[:, t - ctx:ctx], torch.stack(outs, dim=1)[:, -ctx:]], dim=1)
        parts = [constants[:, 0]] if constants is not None else []
        if prescribed is not None:
            parts.append(prescribed[:, t - ctx:t].flatten(1, 2))
        outs.append(win[:, -1] + network(params, torch.cat(parts + [win.flatten(1, 2)], dim=1), DLWP_PAD, act))
    return torch.stack(outs, dim=1)


ACT = {"th.nn.ReLU()": "relu", "th.nn.Tanh()": "tanh"}


def run_case(kind, params, inputs, target, dtype, cfg, roll):
    """forward + mse loss + backward in `dtype`; returns (output, loss, {name: gradient}) as tensors of that dtype"""
    p = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}
    cast = lambda v: None if v is None else torch.as_tensor(v).to(dtype)      # noqa: E731
    act = ACT[cfg.get("activation", "th.nn.ReLU()")]
    if kind == "ns":
        y = ns_forward(p, cast(inputs["x"]), roll["teacher_forcing_steps"], cfg["context_size"], cfg["padding_mode"], act)
    else:
        y = dlwp_forward(p, cast(inputs.get("constants")), cast(inputs.get("prescribed")), cast(inputs["prognostic"]),
                         cfg["context_size"], act)
    loss = F.mse_loss(y, cast(target))
    loss.backward()
    return y.detach(), loss.detach(), {k: v.grad for k, v in p.items()}


def _ns(hidden, pad, ctx, cin=1, n=2, act="th.nn.ReLU()"):
    return dict(in_channels=cin, hidden_channels=hidden, out_channels=cin, n_convolutions=n, activation=act, padding_mode=pad,
                context_size=ctx)


def _dlwp(const, presc, prog, hidden, ctx):
    return dict(constant_channels=const, prescribed_channels=presc, prognostic_channels=prog, hidden_channels=hidden,
                n_convolutions=2, activation="th.nn.ReLU()", context_size=ctx)


# the golden cases: name -> (kind, constructor keywords, (B, T, H, W), rollout keywords of forward)
CASES = {
    "ns_8-16-16_zeros_c2": ("ns", _ns([8, 16, 16], "zeros", 2), (2, 6, 16, 16), dict(teacher_forcing_steps=3)),
    "ns_3-5-8-12-16_circ_c3": ("ns", _ns([3, 5, 8, 12, 16], "circular", 3), (1, 7, 32, 32), dict(teacher_forcing_steps=3)),
    "ns_5-7_n4_c1_tf1": ("ns", _ns([5, 7], "circular", 1, n=4), (3, 4, 8, 12), dict(teacher_forcing_steps=1)),
    "ns_13-16_tanh_tfall": ("ns", _ns([13, 16], "zeros", 1, cin=2, act="th.nn.Tanh()"), (1, 3, 6, 10), dict(teacher_forcing_steps=50)),
    "dlwp_4-8-16-32_c1": ("dlwp", _dlwp(4, 1, 8, [4, 8, 16, 32], 1), (1, 4, 16, 32), {}),
    "dlwp_5-12_c2_noconst": ("dlwp", _dlwp(0, 0, 3, [5, 12], 2), (2, 6, 8, 16), {}),
    "dlwp_6-9-9_c2_presc": ("dlwp", _dlwp(2, 2, 4, [6, 9, 9], 2), (1, 6, 8, 12), {}),
}
GOLDEN = {"ns": "unet_ns_golden.npz", "dlwp": "unet_dlwp_golden.npz"}


def make_inputs(kind, cfg, shape, gen):
    """fresh random inputs and target of a case (the fixtures store their own)"""
    B, T, H, W = shape
    if kind == "ns":
        D = cfg["in_channels"]
        return {"x": torch.randn(B, T, D, H, W, generator=gen)}, torch.randn(B, T, D, H, W, generator=gen)
    inp = {"prognostic": torch.randn(B, T, cfg["prognostic_channels"], H, W, generator=gen)}
    if cfg["constant_channels"]:
        inp["constants"] = torch.randn(B, 1, cfg["constant_channels"], H, W, generator=gen)
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
