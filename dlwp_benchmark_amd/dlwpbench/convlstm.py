"""ConvLSTM baseline of the weather benchmark (src/dlwpbench/models/convlstm/convlstm.py) on the hand-written 3 x 3 convolution
kernels: the reference's constructor keywords, `forward(constants, prescribed, prognostic)` and `state_dict` keys
(`encoder.{1,4,7}`, `clstm.{i}.conv.1`, `decoder.1`).  The reference's CylinderPad (circular in longitude, zeros in latitude)
is the kernels' per-axis padding mode, so no padded tensor is written.  Only the equirectangular mesh is built.
"""
import torch
import torch.nn as nn

from ..conv_ops import Conv3x3
from ..nsbench.convlstm import ConvLSTMCell, _Slot, check_hidden_sizes
from ..rollout_ops import advance

CYLINDER = ("zeros", "circular")          # (latitude, longitude)


class ConvLSTM(nn.Module):
    """The input of a step is `cat(constants, prescribed_t, prognostic_t)` of ONE frame; the network output is a residual to
    `prognostic_t`.  Teacher forcing while `t < context_size`, the model's own previous frame afterwards; the cell states are
    carried across all lead times.  Returns the frames from `context_size` on: `[B, T - context_size, C, H, W]`.

    hidden_sizes must all be equal (ValueError at construction; the reference fails in its first forward pass instead).
    `mesh="healpix"` raises NotImplementedError.  `batch_size`, `height`, `width`, `device` are accepted for compatibility
    (states are allocated per call); extra keywords are ignored."""

    def __init__(self, batch_size=16, constant_channels=4, prescribed_channels=0, prognostic_channels=1, hidden_sizes=(16, 16),
                 height=32, width=64, device=None, bias=True, context_size=1, mesh="equirectangular", **kwargs):
        super().__init__()
        if mesh != "equirectangular":
            raise NotImplementedError("only the equirectangular mesh is on the MI355X hot path (healpix needs dgl)")
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
