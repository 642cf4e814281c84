"""Plain-torch restatement of the HEALPix padding and of the ConvLSTM on the HEALPix mesh (helper module for the tests, not a
conftest): CPU ops only, dtype-generic, differentiable, written from the geometry's description:

* a sphere is 12 square faces of n x n pixels, folded into the batch axis with the face index fastest: 0 - 3 north, 4 - 7
  equator, 8 - 11 south, k = face mod 4 the position around the axis;
* a face is padded by one pixel with the border rows / columns of its eight neighbours.  Equatorial face 4 + k has north k
  above, north k - 1 to the left, south k to the right, south k - 1 below, its equatorial neighbours k + 1 / k - 1 at the top
  right / bottom left, and NO face at the top-left and bottom-right corners (three faces meet there): that corner cell is the
  mean of the two ring cells next to it.  North face k has north k + 1 above (turned by 90 degrees), north k + 2 across the pole
  at the top left (180), north k - 1 to the left (270) and at the bottom left, equator k below, equator k + 1 to the right,
  south k at the bottom right and north k + 1 again at the top right.  South face 8 + k mirrors that: equator k + 1 above,
  equator k to the left, north k at the top left, south k - 1 below (90) and at the bottom left, south k + 1 to the right (270)
  and at the top right, south k + 2 at the bottom right (180);
* the network is the ConvLSTM of tests/convlstm_ref.py with this padding in front of every convolution; frames are
  `[B, C, 12, n, n]`, folded to `[(B 12), C, n, n]` for the network and back for the residual.

`params` is a state_dict-like mapping with the reference's keys (`encoder.{0,2,4}.layers.1`, `clstm.{i}.conv.layers.1`,
`decoder.layers.1`).
"""
import torch
import torch.nn.functional as F

from convlstm_ref import load_case, rel_gap  # noqa: F401  (re-exported: the fixture layout and the measure are the ConvLSTM ones)

FACES = 12
GOLDEN = "convlstm_hpx_golden.npz"
PAD_GOLDEN = "hpx_pad_golden.npz"
PAD_SIZES = (2, 3, 4, 8)


def _neighbours(f):
    """(face, quarter turns) of the top, top-left, left, bottom-left, bottom, bottom-right, right, top-right neighbour of face f
    (None where three faces meet); quarter turns as torch.rot90 counts them on the last two axes"""
    band, k = divmod(f, 4)
    n_, e_, s_ = (lambda q: (k + q) % 4), (lambda q: 4 + (k + q) % 4), (lambda q: 8 + (k + q) % 4)
    if band == 0:
        return [(n_(1), 1), (n_(2), 2), (n_(3), -1), (n_(3), 0), (e_(0), 0), (s_(0), 0), (e_(1), 0), (n_(1), 0)]
    if band == 1:
        return [(n_(0), 0), None, (n_(3), 0), (e_(3), 0), (s_(3), 0), None, (s_(0), 0), (e_(1), 0)]
    return [(e_(1), 0), (n_(0), 0), (e_(0), 0), (s_(3), 0), (s_(3), 1), (s_(2), 2), (s_(1), -1), (s_(1), 0)]


def hpx_pad1(x):
    """x [(B 12), C, n, n] -> [(B 12), C, n + 2, n + 2]: every face padded by one pixel from its neighbour faces"""
    BF, C, n, _ = x.shape
    assert BF % FACES == 0 and x.shape[3] == n, tuple(x.shape)
    faces = x.reshape(BF // FACES, FACES, C, n, n)
    out = []
    for f in range(FACES):
        nb = [None if e is None else torch.rot90(faces[:, e[0]], e[1], (-2, -1)) for e in _neighbours(f)]
        t, tl, l, bl, b, br, r, tr = nb
        top, bottom, left, right = t[..., -1:, :], b[..., :1, :], l[..., :, -1:], r[..., :, :1]
        c_tl = tl[..., -1:, -1:] if tl is not None else 0.5 * top[..., :, :1] + 0.5 * left[..., :1, :]
        c_br = br[..., :1, :1] if br is not None else 0.5 * bottom[..., :, -1:] + 0.5 * right[..., -1:, :]
        rows = [torch.cat([c_tl, top, tr[..., -1:, :1]], dim=-1), torch.cat([left, faces[:, f], right], dim=-1),
                torch.cat([bl[..., :1, -1:], bottom, c_br], dim=-1)]
        out.append(torch.cat(rows, dim=-2))
    return torch.stack(out, dim=1).reshape(BF, C, n + 2, n + 2)


def conv3x3(x, w, b, act=None):
    y = F.conv2d(hpx_pad1(x), w, b)
    if act == "tanh":
        y = torch.tanh(y)
    elif act == "relu":
        y = torch.relu(y)
    return y


def cell(x, h_prev, c_prev, w, b):
    hid = w.shape[0] // 4
    z = conv3x3(torch.cat([x, h_prev], dim=1), w, b)
    zi, ii, ff, oo = torch.split(z, hid, dim=1)
    c = torch.sigmoid(ff) * c_prev + torch.sigmoid(ii) * torch.tanh(zi)
    return torch.sigmoid(oo) * torch.tanh(c), c


def fold(t):
    """[B, C, 12, n, n] -> [(B 12), C, n, n]"""
    B, C, Fc, n, m = t.shape
    return t.permute(0, 2, 1, 3, 4).reshape(B * Fc, C, n, m)


def unfold(t, B):
    """[(B 12), C, n, n] -> [B, C, 12, n, n]"""
    return t.reshape(B, FACES, *t.shape[1:]).permute(0, 2, 1, 3, 4)


def hpx_forward(params, constants, prescribed, prognostic, context_size):
    """constants [B, 1, C, 12, n, n] | None, prescribed [B, T, C, 12, n, n] | None, prognostic [B, T, C, 12, n, n]
    -> [B, T - context_size, C, 12, n, n]"""
    ncell = 0
    while f"clstm.{ncell}.conv.layers.1.weight" in params:
        ncell += 1
    B = prognostic.shape[0]
    states, outs, frame = [None] * ncell, [], None
    for t in range(prognostic.shape[1]):
        prog_t = prognostic[:, t] if t < context_size else frame
        parts = ([constants[:, 0]] if constants is not None else []) + ([prescribed[:, t]] if prescribed is not None else [])
        x = fold(torch.cat(parts + [prog_t], dim=1))
        for i, k in enumerate(("encoder.0", "encoder.2", "encoder.4")):
            x = conv3x3(x, params[k + ".layers.1.weight"], params.get(k + ".layers.1.bias"), "tanh" if i < 2 else None)
        for i in range(ncell):
            w = params[f"clstm.{i}.conv.layers.1.weight"]
            if states[i] is None:
                z = x.new_zeros(x.shape[0], w.shape[0] // 4, x.shape[2], x.shape[3])
                states[i] = (z, z)
            states[i] = cell(x, states[i][0], states[i][1], w, params.get(f"clstm.{i}.conv.layers.1.bias"))
            x = states[i][0]
        frame = prog_t + unfold(conv3x3(x, params["decoder.layers.1.weight"], params.get("decoder.layers.1.bias")), B)
        outs.append(frame)
    return torch.stack(outs[context_size:], dim=1)


def run_case(params, inputs, target, dtype, context_size):
    """forward + mse loss + backward in `dtype`; returns (output, loss, {name: gradient}) as tensors of that dtype"""
    p = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}
    cast = lambda v: None if v is None else torch.as_tensor(v).to(dtype)      # noqa: E731
    y = hpx_forward(p, cast(inputs.get("constants")), cast(inputs.get("prescribed")), cast(inputs["prognostic"]), context_size)
    loss = F.mse_loss(y, cast(target))
    loss.backward()
    return y.detach(), loss.detach(), {k: v.grad for k, v in p.items()}


# the golden cases: name -> (constructor keywords, spheres B, frames T); height = width = the face size
CASES = {
    "hpx_f8": (dict(constant_channels=4, prescribed_channels=1, prognostic_channels=8, hidden_sizes=[16, 16], height=8, width=8,
                    context_size=1), 1, 4),
    "hpx_f4": (dict(constant_channels=4, prescribed_channels=0, prognostic_channels=8, hidden_sizes=[8, 8, 8], height=4, width=4,
                    context_size=2), 2, 6),
}


def make_inputs(cfg, B, T, gen):
    """fresh random inputs and target of a case (the fixture stores its own)"""
    n = cfg["height"]
    shape = lambda t, c: (B, t, c, FACES, n, n)      # noqa: E731
    inp = {"constants": torch.randn(*shape(1, cfg["constant_channels"]), generator=gen),
           "prognostic": torch.randn(*shape(T, cfg["prognostic_channels"]), generator=gen)}
    if cfg["prescribed_channels"]:
        inp["prescribed"] = torch.randn(*shape(T, cfg["prescribed_channels"]), generator=gen)
    return inp, torch.randn(*shape(T - cfg["context_size"], cfg["prognostic_channels"]), generator=gen)


def pad_input(n):
    """the integer-valued float64 tensor [12, 1, n, n] of the padding fixture: all values distinct, so that every padded cell
    names its source, and small integers, so that the mean of two of them is exact"""
    return (2.0 * torch.arange(FACES * n * n, dtype=torch.float64) + 1.0).reshape(FACES, 1, n, n)
