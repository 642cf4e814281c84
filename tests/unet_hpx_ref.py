"""Plain-torch restatement of the U-Net on the HEALPix mesh (helper module for the tests, not a conftest): CPU ops only,
dtype-generic, differentiable, written from the model's description:

* frames are `[B, C, 12, n, n]`, folded to `[(B 12), C, n, n]` for the network and back for the residual (tests/hpx_ref.py);
* every 3 x 3 convolution pads each face by one pixel from its neighbour faces (`hpx_ref.hpx_pad1`, which takes 1 x 1 faces as
  it is: a border row of a one-pixel face is that pixel) and is followed by the activation;
* encoder level l > 0 starts with a 2 x 2 average pool; every level runs `n_convolutions` convolutions, the bottom one half of
  them; the decoder runs bottom to top over `cat(skip, x)`, each level but the top ending in a 2 x 2 stride-2 transposed
  convolution; a 1 x 1 convolution gives the residual to the newest prognostic frame;
* the input of a step is `cat(constants, prescribed window, prognostic window)`, both windows `context_size` frames flattened
  over (time, channel); the prognostic window slides over the model's own frames.

`params` is a state_dict-like mapping with the reference's keys (`encoder.layers.{l}.{slot}.layers.1`,
`decoder.layers.{i}.{slot}.layers.1`, the up-convolution `decoder.layers.{i}.{slot}`, `decoder.output_layer`).
"""
import torch
import torch.nn.functional as F

from hpx_ref import FACES, fold, hpx_pad1, load_case, pad_input, rel_gap, unfold  # noqa: F401  (re-exported)

GOLDEN = "unet_hpx_golden.npz"
PAD_KEY = "pad_n1"

# the golden cases: name -> (constructor keywords, face size, spheres B, frames T)
CASES = {
    "unet_f8": (dict(constant_channels=2, prescribed_channels=1, prognostic_channels=3, hidden_channels=[4, 6, 8, 10],
                     n_convolutions=2, activation="th.nn.ReLU()", context_size=2), 8, 1, 4),
    "unet_f4": (dict(constant_channels=0, prescribed_channels=0, prognostic_channels=2, hidden_channels=[5, 17],
                     n_convolutions=2, activation="th.nn.Tanh()", context_size=1), 4, 2, 3),
}


def _act(name):
    return torch.relu if "ReLU" in name else torch.tanh


def _slots(params, prefix, suffix):
    """the Sequential indices under `prefix` that hold a parameter named `<index><suffix>`, ascending"""
    return sorted(int(k[len(prefix):-len(suffix)]) for k in params
                  if k.startswith(prefix) and k.endswith(suffix) and k[len(prefix):-len(suffix)].isdigit())


def _count(params, fmt):
    n = 0
    while any(k.startswith(fmt.format(n)) for k in params):
        n += 1
    return n


def _conv(params, key, x, act):
    return act(F.conv2d(hpx_pad1(x), params[key + ".layers.1.weight"], params[key + ".layers.1.bias"]))


def network(params, x, act):
    """x [(B 12), C, n, n] -> the residual [(B 12), Cout, n, n]"""
    levels = _count(params, "encoder.layers.{}.")
    skips = []
    for lvl in range(levels):
        pre = f"encoder.layers.{lvl}."
        if lvl:
            x = F.avg_pool2d(x, 2, 2)
        for s in _slots(params, pre, ".layers.1.weight"):
            x = _conv(params, pre + str(s), x, act)
        skips.append(x)
    skips = skips[::-1]
    for i in range(levels):
        pre = f"decoder.layers.{i}."
        if i:
            x = torch.cat([skips[i], x], dim=1)
        for s in _slots(params, pre, ".layers.1.weight"):
            x = _conv(params, pre + str(s), x, act)
        for s in _slots(params, pre, ".weight"):                 # the up-convolution sits in the Sequential itself
            x = F.conv_transpose2d(x, params[f"{pre}{s}.weight"], params[f"{pre}{s}.bias"], stride=2)
    return F.conv2d(x, params["decoder.output_layer.weight"], params["decoder.output_layer.bias"])


def unet_hpx_forward(params, constants, prescribed, prognostic, context_size, activation):
    """constants [B, 1, C, 12, n, n] | None, prescribed [B, T, C, 12, n, n] | None, prognostic [B, T, C, 12, n, n]
    -> [B, T - context_size, C, 12, n, n]"""
    act, ctx, B = _act(activation), context_size, prognostic.shape[0]
    outs = []
    for t in range(ctx, prognostic.shape[1]):
        frames = [prognostic[:, i] for i in range(t - ctx, ctx)] + outs[-ctx:]      # observed, then the model's own
        frames = frames[-ctx:]
        parts = [constants[:, 0]] if constants is not None else []
        if prescribed is not None:
            parts += [prescribed[:, i] for i in range(t - ctx, t)]
        x = fold(torch.cat(parts + frames, dim=1))
        outs.append(frames[-1] + unfold(network(params, x, act), B))
    return torch.stack(outs, dim=1)


def run_case(params, inputs, target, dtype, cfg):
    """forward + mse loss + backward in `dtype`; returns (output, loss, {name: gradient}) as tensors of that dtype"""
    p = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}
    cast = lambda v: None if v is None else torch.as_tensor(v).to(dtype)      # noqa: E731
    y = unet_hpx_forward(p, cast(inputs.get("constants")), cast(inputs.get("prescribed")), cast(inputs["prognostic"]),
                         cfg["context_size"], cfg["activation"])
    loss = F.mse_loss(y, cast(target))
    loss.backward()
    return y.detach(), loss.detach(), {k: v.grad for k, v in p.items()}


def make_inputs(cfg, n, B, T, gen):
    """fresh random inputs and target of a case (the fixture stores its own)"""
    shape = lambda t, c: (B, t, c, FACES, n, n)      # noqa: E731
    inp = {"prognostic": torch.randn(*shape(T, cfg["prognostic_channels"]), generator=gen)}
    if cfg["constant_channels"]:
        inp["constants"] = torch.randn(*shape(1, cfg["constant_channels"]), generator=gen)
    if cfg["prescribed_channels"]:
        inp["prescribed"] = torch.randn(*shape(T, cfg["prescribed_channels"]), generator=gen)
    return inp, torch.randn(*shape(T - cfg["context_size"], cfg["prognostic_channels"]), generator=gen)
