"""3 x 3 convolutions and the ConvLSTM cell over libdlwpmi (csrc/conv3x3.hip; include/dlwpmi.h dlwp_conv3x3_* / dlwp_convlstm_*),
and the other U-Net layers (csrc/unet_ops.hip): 2 x 2 average pool, 2 x 2 stride-2 up-convolution, 1 x 1 convolution.

Activations are channels-last fp32 `[B, H, W, C]`.  The padding is a pair of per-axis modes (height, width), each "zeros" or
"circular", or "healpix" on both axes at once (`[12 * spheres, n, n, C]`, face index fastest: every face is padded with the
border pixels of its neighbour faces, `hpx_halo_map`); it is resolved inside the kernels, so neither a padded tensor nor
`cat(x, h_prev)` is ever written.  The weight
stays `nn.Conv2d`'s `[Cout, Cin, 3, 3]` parameter; the kernels read packed images of it (`pack_weight`), which a model refreshes
once per forward pass and shares between its time steps.  There is no CPU or torch fallback.

`pack_faces=True` (HEALPix padding, faces of 1, 2, 4 or 8 pixels) routes a convolution and both its gradients to the face-packed
kernels (csrc/conv3x3_hpx_packed.hip; dlwp_conv3x3_hpxp_*), whose tiles hold several whole faces: the levels of the HEALPix U-Net
below its top.  The default is False: one tile per face, the only form for larger faces and for the ConvLSTM cell.
"""
import numpy as np
import torch
import torch.nn as nn

from . import lib as L
from .token_ops import _grad_buffer, _grad_slot

PAD = {"zeros": 0, "circular": 1, "healpix": 2}
PAD_HEALPIX = PAD["healpix"]
ACT = {None: 0, "none": 0, "tanh": 1, "relu": 2}
IMG_FWD, IMG_GATES, IMG_DGRAD = 0, 1, 2


def _pad_codes(padding):
    if isinstance(padding, str):
        padding = (padding, padding)
    try:
        ph, pw = PAD[padding[0]], PAD[padding[1]]
    except (KeyError, IndexError, TypeError):
        raise ValueError("padding must be 'zeros' / 'circular' or a (height, width) pair of them, or 'healpix' (both axes), "
                         f"not {padding!r}") from None
    if (ph == PAD_HEALPIX) != (pw == PAD_HEALPIX):
        raise ValueError(f"'healpix' pads both axes at once: it cannot be mixed with another mode ({padding!r})")
    return ph, pw


# ---- HEALPix geometry (padding width 1)
def _hpx_ring(n):
    """(pr, pc) of the 4 n + 4 ring cells of a padded (n + 2) x (n + 2) face in table order: top row, bottom row, left column,
    right column (the columns without their corners)"""
    return ([(0, c) for c in range(n + 2)] + [(n + 1, c) for c in range(n + 2)] + [(r, 0) for r in range(1, n + 1)]
            + [(r, n + 1) for r in range(1, n + 1)])


def hpx_halo_map(n):
    """The HEALPix padding of width 1 as a linear map, pure numpy: for each of the 12 faces (0 - 3 north, 4 - 7 equator, 8 - 11
    south) and each of the `4 * (n + 1)` cells of the one-pixel ring around it, the at most two source pixels.

    Returns `(cells, sources)`: `cells [12, 4 n + 4, 2]` int, the (row, column) of each ring cell in the padded
    `(n + 2) x (n + 2)` face (top row, bottom row, left column, right column); `sources [12, 4 n + 4, 2, 4]` float64 with
    `(face, y, x, weight)` per source, weight 0 (and face -1) for an unused second slot.  Weights are 1, or 0.5 + 0.5 for the
    top-left and bottom-right corner cell of the four equatorial faces, where three faces meet and no corner neighbour exists.
    """
    n = int(n)
    if n < 1:
        raise ValueError(f"the face size must be positive, not {n}")
    m = n - 1
    ring = _hpx_ring(n)
    cells = np.tile(np.asarray(ring, dtype=np.int64), (12, 1, 1))
    src = np.zeros((12, len(ring), 2, 4))
    src[:, :, 1, 0] = -1
    for f in range(12):
        band, k = divmod(f, 4)
        N = lambda q: (k + q) % 4              # noqa: E731  (north, equator, south face q steps around the axis)
        E = lambda q: 4 + (k + q) % 4          # noqa: E731
        S = lambda q: 8 + (k + q) % 4          # noqa: E731
        for ci, (pr, pc) in enumerate(ring):
            i, j = pr - 1, pc - 1
            top, bot, left, right = pr == 0, pr == n + 1, pc == 0, pc == n + 1
            two = None
            if band == 0:      # the pole neighbours N(1), N(2), N(3) are seen rotated by 90, 180, 270 degrees
                if top:
                    one = (N(2), 0, 0) if left else (N(1), m, 0) if right else (N(1), j, 0)
                elif bot:
                    one = (N(3), 0, m) if left else (S(0), 0, 0) if right else (E(0), 0, j)
                else:
                    one = (N(3), 0, i) if left else (E(1), i, 0)
            elif band == 1:
                if top:
                    one = (N(0), m, 0) if left else (E(1), m, 0) if right else (N(0), m, j)
                    two = (N(3), 0, m) if left else None
                elif bot:
                    one = (E(3), 0, m) if left else (S(3), 0, m) if right else (S(3), 0, j)
                    two = (S(0), m, 0) if right else None
                else:
                    one = (N(3), i, m) if left else (S(0), i, 0)
            else:
                if top:
                    one = (N(0), m, m) if left else (S(1), m, 0) if right else (E(1), m, j)
                elif bot:
                    one = (S(3), 0, m) if left else (S(2), m, m) if right else (S(3), j, m)
                else:
                    one = (E(0), i, m) if left else (S(1), m, i)
            src[f, ci, 0] = (*one, 0.5 if two else 1.0)
            if two:
                src[f, ci, 1] = (*two, 0.5)
    return cells, src


def hpx_fold_table(n):
    """The inverse of `hpx_halo_map` in the form `dlwp_conv3x3_hpx_dgrad` reads, numpy int32 `[12, 4 n - 4, 4]`: per border pixel
    of a face (top row, bottom row, left column, right column without corners) the ring cells that read it, in ascending cell
    order, as `(cell << 1) | half` with `cell = (face * (n + 2) + row) * (n + 2) + column` and half = 1 for weight 0.5; -1 = none."""
    if n < 2:
        raise ValueError(f"HEALPix padding needs faces of at least 2 x 2 pixels, not {n}")
    cells, src = hpx_halo_map(n)
    readers = {}
    for f in range(12):
        for ci in range(cells.shape[1]):
            pr, pc = cells[f, ci]
            for sf, y, x, wgt in src[f, ci]:
                if wgt > 0:
                    readers.setdefault((int(sf), int(y), int(x)), []).append(((((f * (n + 2)) + int(pr)) * (n + 2) + int(pc)) << 1)
                                                                             | int(wgt == 0.5))
    pix = ([(0, x) for x in range(n)] + [(n - 1, x) for x in range(n)] + [(y, 0) for y in range(1, n - 1)]
           + [(y, n - 1) for y in range(1, n - 1)])
    table = np.full((12, 4 * n - 4, 4), -1, dtype=np.int32)
    for (f, y, x), ents in readers.items():
        if len(ents) > 4 or (y, x) not in pix:
            raise AssertionError(f"pixel {(f, y, x)} of face size {n} is read by {len(ents)} ring cells")
        table[f, pix.index((y, x)), :len(ents)] = sorted(ents)
    return table


def hpx_fold_rows(n):
    """The inverse of `hpx_halo_map` for every face size n >= 1, in the form `dlwp_conv3x3_hpxp_dgrad` reads, numpy int32
    `[12, n * n, R]`: per pixel of a face (row-major, interior pixels included) the ring cells that read it, in ascending cell
    order, entries as in `hpx_fold_table` (`(cell << 1) | half`), padded with -1.  R is the largest number of readers of one
    pixel, at least 1: 4 for n >= 2 and 10 at n = 1, where one pixel is all four edges and corners of its face."""
    n = int(n)
    cells, src = hpx_halo_map(n)
    readers = [[[] for _ in range(n * n)] for _ in range(12)]
    for f in range(12):
        for ci in range(cells.shape[1]):
            pr, pc = cells[f, ci]
            for sf, y, x, wgt in src[f, ci]:
                if wgt > 0:
                    readers[int(sf)][int(y) * n + int(x)].append(((((f * (n + 2)) + int(pr)) * (n + 2) + int(pc)) << 1)
                                                                  | int(wgt == 0.5))
    R = max(1, max(len(ents) for face in readers for ents in face))
    table = np.full((12, n * n, R), -1, dtype=np.int32)
    for f in range(12):
        for p, ents in enumerate(readers[f]):
            table[f, p, :len(ents)] = sorted(ents)
    return table


PACKED_FACE_SIZES = (1, 2, 4, 8)      # csrc/conv3x3_hpx_packed.hip
_HPX_TABLES = {}


def _hpx_table(n, device):
    """the fold table of face size n on `device`, built and uploaded once (so that a captured step only reads it)"""
    key = (int(n), str(device))
    if key not in _HPX_TABLES:
        _HPX_TABLES[key] = torch.from_numpy(hpx_fold_table(int(n))).to(device)
    return _HPX_TABLES[key]


def _hpx_rows(n, device):
    """`hpx_fold_rows(n)` on `device`, built and uploaded once"""
    key = ("rows", int(n), str(device))
    if key not in _HPX_TABLES:
        _HPX_TABLES[key] = torch.from_numpy(hpx_fold_rows(int(n))).to(device)
    return _HPX_TABLES[key]


def _check_pack_faces(ph, pw, n):
    """`pack_faces=True` is the HEALPix padding on faces of a packed size (ValueError otherwise)"""
    if ph != PAD_HEALPIX or pw != PAD_HEALPIX:
        raise ValueError("pack_faces=True needs padding='healpix': the packed kernels tile whole HEALPix faces")
    if n > 8:
        raise ValueError(f"pack_faces=True is for faces of at most 8 x 8 pixels, not {n} x {n}: larger faces fill the tiles of "
                         "the default kernels")
    if n not in PACKED_FACE_SIZES:
        raise ValueError(f"pack_faces=True: the packed kernels are built for faces of {PACKED_FACE_SIZES} pixels, not {n}")


def _input_grad(dz, dgrad_img, g1, g2, B, H, W, cout, C1, C2, pads, pack_faces=False):
    """the input gradient(s) of a convolution from dz: the flipped-weight product with the same padding for zeros / circular; for
    HEALPix that product over the padded domain of every face followed by the fold onto the pixels the ring cells read"""
    lib = L.load()
    if pack_faces:
        ws = L.workspace(lib.dlwp_conv3x3_hpxp_dgrad_ws_floats, B, H, C1 + C2, device=dz.device)
        table = _hpx_rows(H, dz.device)
        L.check(lib.dlwp_conv3x3_hpxp_dgrad(L.ptr(dz), L.ptr(dgrad_img), table.data_ptr(), table.shape[-1], L.ptr(ws), L.ptr(g1),
                                            L.ptr(g2), B, H, cout, C1, C2, L.stream()))
        return
    if pads[0] != PAD_HEALPIX:
        L.check(lib.dlwp_conv3x3_fwd(L.ptr(dz), None, L.ptr(dgrad_img), None, L.ptr(g1), L.ptr(g2), B, H, W, cout, 0, C1, C2,
                                     pads[0], pads[1], 0, L.stream()))
        return
    ws = L.workspace(lib.dlwp_conv3x3_hpx_dgrad_ws_floats, B, H, C1 + C2, device=dz.device)
    table = _hpx_table(H, dz.device)
    L.check(lib.dlwp_conv3x3_hpx_dgrad(L.ptr(dz), L.ptr(dgrad_img), table.data_ptr(), L.ptr(ws), L.ptr(g1), L.ptr(g2), B, H, cout,
                                       C1, C2, L.stream()))


def _check_weight(weight):
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"a [Cout, Cin, 3, 3] weight is needed, not {tuple(weight.shape)}")


def pack_weight(weight, kind):
    """The image of a `[Cout, Cin, 3, 3]` weight that the kernels read: IMG_FWD (forward), IMG_GATES (forward of a cell weight)
    or IMG_DGRAD (input gradient).  One launch; no gradient flows through it (the Functions below route it to `weight`)."""
    _check_weight(weight)
    lib = L.load()
    cout, cin = weight.shape[0], weight.shape[1]
    w = weight.detach()
    img = L.workspace(lib.dlwp_conv3x3_image_floats, cin, cout, kind, device=w.device)
    L.check(lib.dlwp_conv3x3_pack(L.ptr(w.contiguous()), L.ptr(img), cin, cout, kind, L.stream()))
    return img


class PackedWeight:
    """Forward and input-gradient images of one weight, packed at construction (two launches)."""

    def __init__(self, weight, cell=False, need_grad=True):
        self.fwd = pack_weight(weight, IMG_GATES if cell else IMG_FWD)
        self.dgrad = pack_weight(weight, IMG_DGRAD) if need_grad else None


def _cl(t, what):
    if t.dtype != torch.float32:
        raise L.DlwpError(f"{what}: fp32 needed, not {t.dtype}")
    return t.contiguous()


def _weight_grad(x1, x2, dz, weight_shape, wslot, bslot, has_bias, pads, pack_faces=False):
    """gW, gb of a convolution: straight into the gradient slots where they exist (returns None for those)."""
    lib = L.load()
    B, H, W, C1 = x1.shape
    C2 = x2.shape[-1] if x2 is not None else 0
    cout = weight_shape[0]
    gw, gw_out = _grad_buffer(wslot, weight_shape, dz.device)
    gb, gb_out = _grad_buffer(bslot, cout, dz.device) if has_bias else (None, None)
    if pack_faces:
        ws = L.workspace(lib.dlwp_conv3x3_hpxp_wgrad_ws_floats, B, H, C1 + C2, cout, device=dz.device)
        L.check(lib.dlwp_conv3x3_hpxp_wgrad(L.ptr(x1), L.ptr(x2), L.ptr(dz), L.ptr(ws), L.ptr(gw), L.ptr(gb), B, H, C1, C2, cout,
                                            L.stream()))
        return gw_out, gb_out
    ws = L.workspace(lib.dlwp_conv3x3_wgrad_ws_floats, B, H, W, C1 + C2, cout, device=dz.device)
    L.check(lib.dlwp_conv3x3_wgrad(L.ptr(x1), L.ptr(x2), L.ptr(dz), L.ptr(ws), L.ptr(gw), L.ptr(gb), B, H, W, C1, C2, cout,
                                   pads[0], pads[1], L.stream()))
    return gw_out, gb_out


class _Conv3x3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, weight, bias, packed, pad_h, pad_w, act, pack_faces=False):
        lib = L.load()
        x1 = _cl(x1, "conv3x3")
        x2 = _cl(x2, "conv3x3") if x2 is not None else None
        B, H, W, C1 = x1.shape
        C2 = x2.shape[-1] if x2 is not None else 0
        cout = weight.shape[0]
        if weight.shape[1] != C1 + C2 or (x2 is not None and x2.shape[:3] != x1.shape[:3]):
            raise L.DlwpError(f"conv3x3: weight {tuple(weight.shape)} does not fit inputs with {C1} + {C2} channels")
        y = torch.empty(B, H, W, cout, device=x1.device)
        if pack_faces:
            if H != W:
                raise ValueError(f"HEALPix faces are square, not {H} x {W}")
            _check_pack_faces(pad_h, pad_w, H)
            L.check(lib.dlwp_conv3x3_hpxp_fwd(L.ptr(x1), L.ptr(x2), L.ptr(packed.fwd), L.ptr(bias), L.ptr(y), None, B, H, W, C1, C2,
                                              cout, 0, act, L.stream()))
        else:
            L.check(lib.dlwp_conv3x3_fwd(L.ptr(x1), L.ptr(x2), L.ptr(packed.fwd), L.ptr(bias), L.ptr(y), None, B, H, W, C1, C2, cout, 0,
                                         pad_h, pad_w, act, L.stream()))
        ctx.save_for_backward(x1, x2, y if act else None)
        ctx.packed, ctx.pads, ctx.act, ctx.pack_faces = packed, (pad_h, pad_w), act, pack_faces
        ctx.wshape, ctx.has_bias = weight.shape, bias is not None
        ctx.wslot = _grad_slot(weight)
        ctx.bslot = _grad_slot(bias) if bias is not None else None
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = L.load()
        x1, x2, y = ctx.saved_tensors
        B, H, W, C1 = x1.shape
        C2 = x2.shape[-1] if x2 is not None else 0
        cout = ctx.wshape[0]
        dz = _cl(gy, "conv3x3 backward")
        if ctx.act:
            g = dz
            dz = torch.empty_like(g)
            L.check(lib.dlwp_conv3x3_act_bwd(L.ptr(y), L.ptr(g), L.ptr(dz), g.numel(), ctx.act, L.stream()))
        need1, need2 = ctx.needs_input_grad[0], (x2 is not None and ctx.needs_input_grad[1])
        g1 = torch.empty_like(x1) if need1 else None
        g2 = torch.empty_like(x2) if need2 else None
        if need1 or need2:
            if ctx.packed.dgrad is None:
                raise L.DlwpError("conv3x3: this weight was packed without its input-gradient image")
            _input_grad(dz, ctx.packed.dgrad, g1, g2, B, H, W, cout, C1, C2, ctx.pads, ctx.pack_faces)
        gw = gb = None
        if ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3]):
            gw, gb = _weight_grad(x1, x2, dz, ctx.wshape, ctx.wslot, ctx.bslot, ctx.has_bias, ctx.pads, ctx.pack_faces)
        return g1, g2, gw, gb, None, None, None, None, None


def conv3x3(x, weight, bias=None, padding="zeros", act=None, x2=None, packed=None, pack_faces=False):
    """`act(conv2d(cat(x, x2), weight, bias))`, 3 x 3, stride 1, same size, on channels-last `[B, H, W, C]` tensors.
    padding: "zeros" / "circular" or a (height, width) pair, or "healpix" (`B = 12 * spheres` square faces); act: None / "tanh" /
    "relu"; packed: the weight's PackedWeight
    (built here when absent: two more launches).  pack_faces=True (HEALPix padding, faces of 1, 2, 4 or 8 pixels; ValueError
    otherwise): forward, input gradient and weight gradient run the face-packed kernels (csrc/conv3x3_hpx_packed.hip), whose
    tiles hold several whole faces -- the same weight images, the same results up to the order of the fold's additions."""
    _check_weight(weight)
    ph, pw = _pad_codes(padding)
    if act not in ACT:
        raise ValueError(f"act must be None, 'tanh' or 'relu', not {act!r}")
    if pack_faces:
        if x.dim() != 4 or x.shape[1] != x.shape[2]:
            raise ValueError(f"pack_faces=True needs square faces [12 * spheres, n, n, C], not {tuple(x.shape)}")
        _check_pack_faces(ph, pw, x.shape[1])
    if packed is None:
        packed = PackedWeight(weight, need_grad=torch.is_grad_enabled())
    return _Conv3x3Fn.apply(x, x2, weight, bias, packed, ph, pw, ACT[act], bool(pack_faces))


class _ConvLSTMCellFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h_prev, c_prev, weight, bias, packed, pad_h, pad_w):
        lib = L.load()
        x = _cl(x, "convlstm_cell")
        h_prev = _cl(h_prev, "convlstm_cell") if h_prev is not None else None
        c_prev = _cl(c_prev, "convlstm_cell") if c_prev is not None else None
        B, H, W, Cx = x.shape
        hid = weight.shape[0] // 4
        if weight.shape[0] != 4 * hid or weight.shape[1] != Cx + hid:
            raise L.DlwpError(f"convlstm_cell: weight {tuple(weight.shape)} does not fit {Cx} input and {hid} hidden channels")
        for s in (h_prev, c_prev):
            if s is not None and tuple(s.shape) != (B, H, W, hid):
                raise L.DlwpError(f"convlstm_cell: state {tuple(s.shape)} where {(B, H, W, hid)} is needed")
        keep = any(ctx.needs_input_grad)
        h = torch.empty(B, H, W, hid, device=x.device)
        c = torch.empty_like(h)
        gates = torch.empty(B, H, W, 4 * hid, device=x.device) if keep else None
        L.check(lib.dlwp_convlstm_cell_fwd(L.ptr(x), L.ptr(h_prev), L.ptr(packed.fwd), L.ptr(bias), L.ptr(c_prev), L.ptr(h), L.ptr(c),
                                           L.ptr(gates), B, H, W, Cx, hid, pad_h, pad_w, L.stream()))
        if keep:
            ctx.save_for_backward(x, h_prev, c_prev, c, gates)
        ctx.packed, ctx.pads, ctx.wshape, ctx.has_bias = packed, (pad_h, pad_w), weight.shape, bias is not None
        ctx.wslot = _grad_slot(weight)
        ctx.bslot = _grad_slot(bias) if bias is not None else None
        return h, c

    @staticmethod
    def backward(ctx, gh, gc):
        lib = L.load()
        x, h_prev, c_prev, c, gates = ctx.saved_tensors
        B, H, W, Cx = x.shape
        hid = c.shape[-1]
        gh = _cl(gh, "convlstm_cell backward") if gh is not None else None
        gc = _cl(gc, "convlstm_cell backward") if gc is not None else None
        dz = torch.empty_like(gates)
        dc_prev = torch.empty_like(c)
        L.check(lib.dlwp_convlstm_gate_bwd(L.ptr(gh), L.ptr(gc), L.ptr(gates), L.ptr(c_prev), L.ptr(c), L.ptr(dz), L.ptr(dc_prev),
                                           B * H * W, hid, L.stream()))
        needx, needh = ctx.needs_input_grad[0], (h_prev is not None and ctx.needs_input_grad[1])
        gx = torch.empty_like(x) if needx else None
        ghp = torch.empty_like(h_prev) if needh else None
        if needx or needh:
            if ctx.packed.dgrad is None:
                raise L.DlwpError("convlstm_cell: this weight was packed without its input-gradient image")
            _input_grad(dz, ctx.packed.dgrad, gx, ghp, B, H, W, 4 * hid, Cx, hid, ctx.pads)
        gw = gb = None
        if ctx.needs_input_grad[3] or (ctx.has_bias and ctx.needs_input_grad[4]):
            if h_prev is None:
                # zero state: the recurrent half of the weight gets no gradient -- the product runs over cat(x, 0)
                h_prev = torch.zeros_like(c)
            gw, gb = _weight_grad(x, h_prev, dz, ctx.wshape, ctx.wslot, ctx.bslot, ctx.has_bias, ctx.pads)
        return gx, ghp, (dc_prev if (c_prev is not None and ctx.needs_input_grad[2]) else None), gw, gb, None, None, None


def convlstm_cell(x, h_prev, c_prev, weight, bias=None, padding="circular", packed=None):
    """One ConvLSTM step on channels-last tensors: `z = conv3x3(cat(x, h_prev), weight) + bias` with the output channels
    (input, i, f, o) in blocks of `hidden`; `c = sigmoid(f) * c_prev + sigmoid(i) * tanh(input)`, `h = sigmoid(o) * tanh(c)`.
    Returns (h, c).  h_prev / c_prev None = zero state.  Under `torch.no_grad()` nothing is kept for a backward pass."""
    _check_weight(weight)
    ph, pw = _pad_codes(padding)
    if packed is None:
        packed = PackedWeight(weight, cell=True, need_grad=torch.is_grad_enabled())
    return _ConvLSTMCellFn.apply(x, h_prev, c_prev, weight, bias, packed, ph, pw)


class Conv3x3(nn.Conv2d):
    """`nn.Conv2d(cin, cout, 3, padding=1)` on the hand-written kernel: parameter names and shapes are nn.Conv2d's, so a
    checkpoint of the torch layer loads as it is.  `forward` takes and returns channels-FIRST `[B, C, H, W]` like nn.Conv2d
    (two permute copies); `forward_cl` is the channels-last form the models chain.  `pad_modes`: per-axis (height, width)
    padding, default from `padding_mode` ("zeros" / "circular" on both axes); `("healpix", "healpix")` for a HEALPix layer."""

    def __init__(self, in_channels, out_channels, kernel_size=3, padding=1, padding_mode="zeros", bias=True, pad_modes=None,
                 act=None, pack_faces=False, **kw):
        ks = kernel_size if isinstance(kernel_size, int) else kernel_size[0]
        if ks != 3 or padding not in (1, (1, 1)) or padding_mode not in ("zeros", "circular"):
            raise ValueError("Conv3x3: kernel_size 3, padding 1 and padding_mode 'zeros' / 'circular' only")
        super().__init__(in_channels, out_channels, 3, padding=1, padding_mode=padding_mode, bias=bias, **kw)
        if tuple(self.stride) != (1, 1) or tuple(self.dilation) != (1, 1) or self.groups != 1:
            raise ValueError("Conv3x3: stride 1, dilation 1, groups 1 only")
        self.pad_modes = tuple(pad_modes) if pad_modes is not None else (padding_mode, padding_mode)
        _pad_codes(self.pad_modes)
        if act not in ACT:
            raise ValueError(f"act must be None, 'tanh' or 'relu', not {act!r}")
        self.act = act
        if pack_faces and _pad_codes(self.pad_modes) != (PAD_HEALPIX, PAD_HEALPIX):
            raise ValueError("Conv3x3: pack_faces=True needs pad_modes=('healpix', 'healpix')")
        self.pack_faces = bool(pack_faces)

    def pack(self, cell=False):
        return PackedWeight(self.weight, cell=cell, need_grad=torch.is_grad_enabled())

    def forward_cl(self, x, x2=None, packed=None):
        return conv3x3(x, self.weight, self.bias, self.pad_modes, self.act, x2=x2, packed=packed, pack_faces=self.pack_faces)

    def forward(self, x):
        return self.forward_cl(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


# ---- the U-Net layers that are not 3 x 3 convolutions (csrc/unet_ops.hip)
class _AvgPool2x2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _cl(x, "avg_pool2x2")
        if x.dim() != 4:
            raise L.DlwpError(f"avg_pool2x2: a [B, H, W, C] tensor is needed, not {tuple(x.shape)}")
        B, H, W, C = x.shape
        y = torch.empty(B, H // 2, W // 2, C, device=x.device)
        L.check(L.load().dlwp_avgpool2x2_fwd(L.ptr(x), L.ptr(y), B, H, W, C, L.stream()))
        ctx.shape = (B, H, W, C)
        return y

    @staticmethod
    def backward(ctx, gy):
        B, H, W, C = ctx.shape
        gy = _cl(gy, "avg_pool2x2 backward")
        gx = torch.empty(B, H, W, C, device=gy.device)
        L.check(L.load().dlwp_avgpool2x2_bwd(L.ptr(gy), L.ptr(gx), B, H, W, C, L.stream()))
        return gx


def avg_pool2x2(x):
    """`avg_pool2d(x, 2, 2)` on a channels-last `[B, H, W, C]` tensor (H and W even) -> `[B, H/2, W/2, C]`."""
    return _AvgPool2x2Fn.apply(x)


def _pixel_weight_grad(up, x, dy, weight_shape, wslot, bslot, has_bias):
    """gW, gb of a 1 x 1 convolution or (up) a 2 x 2 up-convolution: straight into the gradient slots where they exist
    (returns None for those)."""
    lib = L.load()
    B, H, W, cin = x.shape
    cout = weight_shape[1] if up else weight_shape[0]
    gw, gw_out = _grad_buffer(wslot, weight_shape, dy.device)
    gb, gb_out = _grad_buffer(bslot, cout, dy.device) if has_bias else (None, None)
    if up:
        ws = L.workspace(lib.dlwp_upconv2x2_wgrad_ws_floats, B, H, W, cin, cout, device=dy.device)
        L.check(lib.dlwp_upconv2x2_wgrad(L.ptr(x), L.ptr(dy), L.ptr(ws), L.ptr(gw), L.ptr(gb), B, H, W, cin, cout, L.stream()))
    else:
        ws = L.workspace(lib.dlwp_conv1x1_wgrad_ws_floats, B * H * W, cin, cout, device=dy.device)
        L.check(lib.dlwp_conv1x1_wgrad(L.ptr(x), L.ptr(dy), L.ptr(ws), L.ptr(gw), L.ptr(gb), B * H * W, cin, cout, L.stream()))
    return gw_out, gb_out


class _PixelConvFn(torch.autograd.Function):
    """up = False: the 1 x 1 convolution; up = True: the 2 x 2 stride-2 transposed convolution (one kernel family)."""

    @staticmethod
    def forward(ctx, x, weight, bias, up):
        lib = L.load()
        what = "upconv2x2" if up else "conv1x1"
        x = _cl(x, what)
        w = _cl(weight.detach(), what)
        if x.dim() != 4 or weight.shape[0 if up else 1] != x.shape[-1]:
            raise L.DlwpError(f"{what}: weight {tuple(weight.shape)} does not fit an input of shape {tuple(x.shape)}")
        B, H, W, cin = x.shape
        if up:
            cout = weight.shape[1]
            y = torch.empty(B, 2 * H, 2 * W, cout, device=x.device)
            L.check(lib.dlwp_upconv2x2_fwd(L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(y), B, H, W, cin, cout, L.stream()))
        else:
            cout = weight.shape[0]
            y = torch.empty(B, H, W, cout, device=x.device)
            L.check(lib.dlwp_conv1x1_fwd(L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(y), B * H * W, cin, cout, L.stream()))
        ctx.save_for_backward(x, w)
        ctx.up, ctx.cout, ctx.wshape, ctx.has_bias = up, cout, weight.shape, bias is not None
        ctx.wslot = _grad_slot(weight)
        ctx.bslot = _grad_slot(bias) if bias is not None else None
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = L.load()
        x, w = ctx.saved_tensors
        B, H, W, cin = x.shape
        gy = _cl(gy, "upconv2x2 backward" if ctx.up else "conv1x1 backward")
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            if ctx.up:
                L.check(lib.dlwp_upconv2x2_dgrad(L.ptr(gy), L.ptr(w), L.ptr(gx), B, H, W, cin, ctx.cout, L.stream()))
            else:
                L.check(lib.dlwp_conv1x1_dgrad(L.ptr(gy), L.ptr(w), L.ptr(gx), B * H * W, cin, ctx.cout, L.stream()))
        gw = gb = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gw, gb = _pixel_weight_grad(ctx.up, x, gy, ctx.wshape, ctx.wslot, ctx.bslot, ctx.has_bias)
        return gx, gw, gb, None


def upconv2x2(x, weight, bias=None):
    """`conv_transpose2d(x, weight, bias, stride=2)` with a `[Cin, Cout, 2, 2]` weight on a channels-last `[B, H, W, Cin]`
    tensor -> `[B, 2H, 2W, Cout]`.  The kernels read the parameter's own layout: nothing is packed."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (2, 2):
        raise ValueError(f"a [Cin, Cout, 2, 2] weight is needed, not {tuple(weight.shape)}")
    return _PixelConvFn.apply(x, weight, bias, True)


def conv1x1(x, weight, bias=None):
    """`conv2d(x, weight, bias)` with a `[Cout, Cin, 1, 1]` weight on a channels-last `[B, H, W, Cin]` tensor."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (1, 1):
        raise ValueError(f"a [Cout, Cin, 1, 1] weight is needed, not {tuple(weight.shape)}")
    return _PixelConvFn.apply(x, weight, bias, False)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class UpConv2x2(nn.ConvTranspose2d):
    """`nn.ConvTranspose2d(cin, cout, kernel_size=2, stride=2)` on the hand-written kernel; parameter names and shapes are
    torch's.  `forward` is channels-first like the torch layer (two permute copies), `forward_cl` channels-last."""

    def __init__(self, in_channels, out_channels, kernel_size=2, stride=2, bias=True, **kw):
        if _pair(kernel_size) != (2, 2) or _pair(stride) != (2, 2):
            raise ValueError("UpConv2x2: kernel_size 2 and stride 2 only")
        super().__init__(in_channels, out_channels, 2, stride=2, bias=bias, **kw)
        if (tuple(self.padding) != (0, 0) or tuple(self.output_padding) != (0, 0) or tuple(self.dilation) != (1, 1) or self.groups != 1
                or self.padding_mode != "zeros"):
            raise ValueError("UpConv2x2: padding 0, output_padding 0, dilation 1, groups 1 only")

    def forward_cl(self, x):
        return upconv2x2(x, self.weight, self.bias)

    def forward(self, x, output_size=None):
        if output_size is not None:
            raise ValueError("UpConv2x2: the output size is always twice the input size")
        return self.forward_cl(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


class Conv1x1(nn.Conv2d):
    """`nn.Conv2d(cin, cout, kernel_size=1)` on the hand-written kernel; parameter names and shapes are torch's."""

    def __init__(self, in_channels, out_channels, kernel_size=1, bias=True, **kw):
        if _pair(kernel_size) != (1, 1):
            raise ValueError("Conv1x1: kernel_size 1 only")
        super().__init__(in_channels, out_channels, 1, bias=bias, **kw)
        if (tuple(self.stride) != (1, 1) or self.padding not in (0, (0, 0)) or tuple(self.dilation) != (1, 1) or self.groups != 1):
            raise ValueError("Conv1x1: stride 1, padding 0, dilation 1, groups 1 only")

    def forward_cl(self, x):
        return conv1x1(x, self.weight, self.bias)

    def forward(self, x):
        return self.forward_cl(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
