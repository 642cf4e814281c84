"""ConvLSTM baseline of the weather benchmark (src/dlwpbench/models/convlstm/convlstm.py) on the hand-written 3 x 3 convolution
kernels: the reference's constructor keywords, `forward(constants, prescribed, prognostic)` and `state_dict` keys
(`encoder.{1,4,7}`, `clstm.{i}.conv.1`, `decoder.1`).  The reference's CylinderPad (circular in longitude, zeros in latitude)
is the kernels' per-axis padding mode, so no padded tensor is written.

`ConvLSTMHPX` is the same network on the HEALPix mesh: `[B, T, C, 12, n, n]` tensors, every convolution behind the reference's
HEALPixPadding (src/dlwpbench/utils/healpix.py), which is the kernels' "healpix" padding mode; `state_dict` keys
`encoder.{0,2,4}.layers.1`, `clstm.{i}.conv.layers.1`, `decoder.layers.1`.
"""
import torch
import torch.nn as nn

from ..conv_ops import Conv3x3
from ..nsbench.convlstm import ConvLSTMCell, Layers, _Slot, check_hidden_sizes
from ..rollout_ops import advance

CYLINDER = ("zeros", "circular")          # (latitude, longitude)
HEALPIX = ("healpix", "healpix")
FACES = 12


class ConvLSTM(nn.Module):
    """The input of a step is `cat(constants, prescribed_t, prognostic_t)` of ONE frame; the network output is a residual to
    `prognostic_t`.  Teacher forcing while `t < context_size`, the model's own previous frame afterwards; the cell states are
    carried across all lead times.  Returns the frames from `context_size` on: `[B, T - context_size, C, H, W]`.

    hidden_sizes must all be equal (ValueError at construction; the reference fails in its first forward pass instead).
    `mesh="healpix"` raises NotImplementedError (the reference's class prepares 5-D inputs there too): ConvLSTMHPX is that model.  `batch_size`, `height`, `width`, `device` are accepted for compatibility
    (states are allocated per call); extra keywords are ignored."""

    def __init__(self, batch_size=16, constant_channels=4, prescribed_channels=0, prognostic_channels=1, hidden_sizes=(16, 16),
                 height=32, width=64, device=None, bias=True, context_size=1, mesh="equirectangular", **kwargs):
        super().__init__()
        if mesh != "equirectangular":
            raise NotImplementedError("ConvLSTM is the equirectangular model; the HEALPix mesh is ConvLSTMHPX")
        hs = check_hidden_sizes(hidden_sizes)
        if context_size < 1:
            raise ValueError("context_size must be >= 1: the first frame has no previous output to feed back")
        self.batch_size, self.hidden_sizes, self.height, self.width = batch_size, hs, height, width
        self.bias, self.context_size, self.mesh = bias, context_size, mesh
        self.prognostic_channels = prognostic_channels
        in_size = constant_channels + prescribed_channels + prognostic_channels
        h = hs[0]
        cyl = dict(pad_modes=CYLINDER)
        self.encoder = nn.Sequential(_Slot(), Conv3x3(in_size, h, act="tanh", **cyl), _Slot(),
                                     _Slot(), Conv3x3(h, h, act="tanh", **cyl), _Slot(),
                                     _Slot(), Conv3x3(h, h, **cyl))
        self.clstm = nn.Sequential(*[ConvLSTMCell(hh, hh, bias=bias, pad_modes=CYLINDER, wrap_conv=True) for hh in hs])
        self.decoder = nn.Sequential(_Slot(), Conv3x3(hs[-1], prognostic_channels, **cyl))
        if device is not None:
            self.to(device)

    def reset(self, batch_size=None):
        for cell in self.clstm:
            cell.reset_states(batch_size)

    def forward(self, constants=None, prescribed=None, prognostic=None):
        """constants [B, 1, C, H, W] | None, prescribed [B, T, C, H, W] | None, prognostic [B, T, C, H, W]"""
        B, T = prognostic.shape[:2]
        if T <= self.context_size:
            raise ValueError(f"prognostic has {T} frames: more than context_size = {self.context_size} are needed")
        self.reset(B)
        enc = [m for m in self.encoder if isinstance(m, Conv3x3)]
        dec = self.decoder[1]
        packs = [c.pack() for c in enc]
        cpacks = [cell.layer.pack(cell=True) for cell in self.clstm]
        dpack = dec.pack()
        outs, frame = [], None
        for t in range(T):
            prog_t = prognostic[:, t] if t < self.context_size else frame
            parts = ([constants[:, 0]] if constants is not None else []) + ([prescribed[:, t]] if prescribed is not None else [])
            x = torch.cat(parts + [prog_t], dim=1).permute(0, 2, 3, 1)        # channels-last frame (one copy)
            for conv, p in zip(enc, packs):
                x = conv.forward_cl(x, packed=p)
            for cell, p in zip(self.clstm, cpacks):
                x, _ = cell(x, packed=p)
            delta = dec.forward_cl(x, packed=dpack).permute(0, 3, 1, 2)
            frame = advance(prog_t.unsqueeze(1), delta, want_next=False)[2]   # prognostic_t + delta (dlwp_window_advance_fwd)
            outs.append(frame)
        self.reset(B)
        return torch.stack(outs[self.context_size:], dim=1)


class ConvLSTMHPX(nn.Module):
    """ConvLSTM on the HEALPix mesh: tensors are `[B, T, C, 12, n, n]` (12 square faces per sphere), one network call per frame
    runs on the folded `[(B * 12), n, n, C]` channels-last frame (face index fastest, the reference's `(b f)`), and every
    convolution pads each face with the border pixels of its neighbour faces inside the kernel.  Input, residual output, teacher
    forcing and carried states as in `ConvLSTM`.  Returns `[B, T - context_size, C, 12, n, n]`.

    As in the reference the cells' convolutions always have a bias (its HEALPix cell does not pass `bias` on); `height` /
    `width` are accepted for compatibility (the face size is the input's).  ValueError for unequal hidden_sizes at construction
    and, in `forward`, for a face count other than 12 or faces that are not square."""

    def __init__(self, batch_size=16, constant_channels=4, prescribed_channels=0, prognostic_channels=1, hidden_sizes=(16, 16),
                 height=32, width=64, device=None, bias=True, context_size=1, mesh="healpix", **kwargs):
        super().__init__()
        if mesh != "healpix":
            raise NotImplementedError("ConvLSTMHPX is the HEALPix model; the equirectangular mesh is ConvLSTM")
        hs = check_hidden_sizes(hidden_sizes)
        if context_size < 1:
            raise ValueError("context_size must be >= 1: the first frame has no previous output to feed back")
        self.batch_size, self.hidden_sizes, self.height, self.width = batch_size, hs, height, width
        self.bias, self.context_size, self.mesh = bias, context_size, mesh
        self.prognostic_channels = prognostic_channels
        in_size = constant_channels + prescribed_channels + prognostic_channels
        h = hs[0]
        hpx = dict(pad_modes=HEALPIX)
        self.encoder = nn.Sequential(Layers(Conv3x3(in_size, h, act="tanh", **hpx)), _Slot(),
                                     Layers(Conv3x3(h, h, act="tanh", **hpx)), _Slot(),
                                     Layers(Conv3x3(h, h, **hpx)))
        self.clstm = nn.Sequential(*[ConvLSTMCell(hh, hh, bias=True, pad_modes=HEALPIX, wrap_conv="layers") for hh in hs])
        self.decoder = Layers(Conv3x3(hs[-1], prognostic_channels, **hpx))
        if device is not None:
            self.to(device)

    def reset(self, batch_size=None):
        for cell in self.clstm:
            cell.reset_states(batch_size)

    def forward(self, constants=None, prescribed=None, prognostic=None):
        """constants [B, 1, C, 12, n, n] | None, prescribed [B, T, C, 12, n, n] | None, prognostic [B, T, C, 12, n, n]"""
        if prognostic.dim() != 6 or prognostic.shape[3] != FACES:
            raise ValueError(f"prognostic must be [B, T, C, 12, n, n] (12 HEALPix faces), not {tuple(prognostic.shape)}")
        B, T, C, _, n, n2 = prognostic.shape
        if n != n2:
            raise ValueError(f"HEALPix faces are square: prognostic has {n} x {n2} faces")
        if n < 2:
            raise ValueError("HEALPix faces of at least 2 x 2 pixels are needed")
        if T <= self.context_size:
            raise ValueError(f"prognostic has {T} frames: more than context_size = {self.context_size} are needed")
        self.reset(B * FACES)
        enc = [m.conv for m in self.encoder if isinstance(m, Layers)]
        dec = self.decoder.conv
        packs = [c.pack() for c in enc]
        cpacks = [cell.layer.pack(cell=True) for cell in self.clstm]
        dpack = dec.pack()
        outs, frame = [], None
        for t in range(T):
            prog_t = prognostic[:, t] if t < self.context_size else frame
            parts = ([constants[:, 0]] if constants is not None else []) + ([prescribed[:, t]] if prescribed is not None else [])
            x = torch.cat(parts + [prog_t], dim=1)                              # [B, C, 12, n, n]
            x = x.permute(0, 2, 3, 4, 1).reshape(B * FACES, n, n, x.shape[1])   # folded channels-last frame (one copy)
            for conv, p in zip(enc, packs):
                x = conv.forward_cl(x, packed=p)
            for cell, p in zip(self.clstm, cpacks):
                x, _ = cell(x, packed=p)
            delta = dec.forward_cl(x, packed=dpack).view(B, FACES, n, n, C).permute(0, 4, 1, 2, 3)
            frame = advance(prog_t.unsqueeze(1), delta, want_next=False)[2]     # prognostic_t + delta (dlwp_window_advance_fwd)
            outs.append(frame)
        self.reset(B * FACES)
        return torch.stack(outs[self.context_size:], dim=1)
