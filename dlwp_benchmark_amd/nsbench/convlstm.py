"""ConvLSTM baseline of the Navier-Stokes benchmark (src/nsbench/models/convlstm/convlstm.py) on the hand-written 3 x 3
convolution kernels (conv_ops): constructor keywords, `forward` signature and `state_dict` keys are the reference's, so its
checkpoints load with `load_state_dict(strict=True)`.

Inside, activations are channels-last `[B, H, W, C]`; every convolution pads circularly on both axes inside the kernel, a
cell step is ONE launch (convolution over `x | h_prev` + gates + state update), and the packed weight images are refreshed once
per forward pass and shared by all time steps.
"""
import torch
import torch.nn as nn

from ..conv_ops import Conv3x3, convlstm_cell


class _Slot(nn.Module):
    """Parameter-free placeholder at the Sequential indices where the reference has its Tanh / padding modules (the
    activation and the padding run inside the neighbouring convolution kernel); keeps the `state_dict` keys aligned."""

    def forward(self, x):
        return x


class Layers(nn.Module):
    """The shape of the reference's HEALPixLayer: the convolution at index 1 of a Sequential NAMED `layers`, behind its padding
    module (key `layers.1.weight`)."""

    def __init__(self, conv):
        super().__init__()
        self.layers = nn.Sequential(_Slot(), conv)

    @property
    def conv(self):
        return self.layers[1]


class ConvLSTMCell(nn.Module):
    """One cell: `conv` is the 3 x 3 convolution `2 hidden -> 4 hidden` over `cat(x, h_prev)`; the states are plain
    attributes (not buffers), zeroed by `reset_states`.  wrap_conv: the reference's dlwpbench cell keeps the convolution at
    index 1 of a Sequential behind its padding module (key `conv.1.weight`); wrap_conv="layers": its HEALPix cell keeps it in a
    HEALPixLayer (key `conv.layers.1.weight`)."""

    def __init__(self, input_size, hidden_size, bias=True, pad_modes=("circular", "circular"), wrap_conv=False):
        super().__init__()
        self.input_size, self.hidden_size, self.pad_modes = input_size, hidden_size, tuple(pad_modes)
        conv = Conv3x3(input_size + hidden_size, 4 * hidden_size, bias=bias, pad_modes=pad_modes)
        self.conv = Layers(conv) if wrap_conv == "layers" else (nn.Sequential(_Slot(), conv) if wrap_conv else conv)
        self.h = self.c = None

    @property
    def layer(self):
        if isinstance(self.conv, Layers):
            return self.conv.conv
        return self.conv[1] if isinstance(self.conv, nn.Sequential) else self.conv

    def reset_states(self, batch_size=None):
        self.h = self.c = None           # None = zero state: the first step skips the recurrent half of the product

    def forward(self, x, packed=None):
        conv = self.layer
        self.h, self.c = convlstm_cell(x, self.h, self.c, conv.weight, conv.bias, self.pad_modes, packed=packed)
        return self.h, self.c


def check_hidden_sizes(hidden_sizes):
    hs = [int(h) for h in hidden_sizes]
    if not hs or any(h < 1 for h in hs):
        raise ValueError(f"hidden_sizes must be a non-empty list of positive widths, not {hidden_sizes!r}")
    if any(h != hs[0] for h in hs):
        raise ValueError(f"hidden_sizes must all be equal (got {hs}): every cell is built with input_size = hidden_size = "
                         "hidden_sizes[i], so the reference fails in its first forward pass for unequal entries")
    return hs


class ConvLSTM(nn.Module):
    """encoder (three 3 x 3 convolutions 1 -> h -> h -> h, tanh after the first two) -> len(hidden_sizes) ConvLSTM cells ->
    decoder (3 x 3, h -> input_size); circular padding everywhere.  As in the reference the encoder reads ONE channel, so
    `input_size` must be 1 for the closed loop to feed the output back.

    hidden_sizes must all be equal: a ValueError is raised here at construction (the reference builds such a model and fails
    in its first forward pass).  `batch_size`, `height`, `width` and `device` are accepted for compatibility: the states are
    allocated per forward call at the batch size and grid of the input.  Extra keywords (`type`, `name`, ...) are ignored."""

    def __init__(self, batch_size=None, input_size=1, hidden_sizes=(16, 16), height=None, width=None, device=None, bias=True,
                 **kwargs):
        super().__init__()
        hs = check_hidden_sizes(hidden_sizes)
        self.batch_size, self.input_size, self.hidden_sizes = batch_size, input_size, hs
        self.height, self.width, self.bias = height, width, bias
        h = hs[0]
        circ = dict(padding_mode="circular")
        self.encoder = nn.Sequential(Conv3x3(1, h, act="tanh", **circ), _Slot(), Conv3x3(h, h, act="tanh", **circ), _Slot(),
                                     Conv3x3(h, h, **circ))
        self.clstm = nn.Sequential(*[ConvLSTMCell(hh, hh, bias=bias) for hh in hs])
        self.decoder = nn.Sequential(Conv3x3(hs[-1], input_size, **circ))
        if device is not None:
            self.to(device)

    def reset(self, batch_size=None):
        for cell in self.clstm:
            cell.reset_states(batch_size)

    def _pack(self):
        convs = [m for m in self.encoder if isinstance(m, Conv3x3)] + [m for m in self.decoder if isinstance(m, Conv3x3)]
        return [c.pack() for c in convs], [cell.layer.pack(cell=True) for cell in self.clstm]

    def _net(self, x_cl, packs):
        """one network call on a channels-last frame [B, H, W, 1] -> [B, H, W, input_size]"""
        pc, pl = packs
        convs = [m for m in self.encoder if isinstance(m, Conv3x3)]
        for conv, p in zip(convs, pc):
            x_cl = conv.forward_cl(x_cl, packed=p)
        for cell, p in zip(self.clstm, pl):
            x_cl, _ = cell(x_cl, packed=p)
        return self.decoder[0].forward_cl(x_cl, packed=pc[-1])

    def forward(self, x, teacher_forcing_steps=50):
        """x [B, T, D, H, W] (D = 1) -> [B, T, D, H, W]: states zeroed, one network call per time step; the input is x[:, t]
        while t < teacher_forcing_steps and the previous output afterwards."""
        if teacher_forcing_steps < 1:
            raise ValueError("teacher_forcing_steps must be >= 1: the first frame has no previous output to feed back")
        B, T, D, H, W = x.shape
        if D != 1:
            raise ValueError(f"the encoder reads one channel (as the reference's does): x has D = {D}")
        self.reset(B)
        packs = self._pack()
        outs, out = [], None
        for t in range(T):
            # D = 1: a [B, 1, H, W] frame and its channels-last form [B, H, W, 1] are the same memory
            x_t = x[:, t].reshape(B, H, W, 1) if t < teacher_forcing_steps else out
            out = self._net(x_t, packs)
            outs.append(out)
        self.reset(B)                        # states are per call: nothing of the graph is kept alive on the module
        y = torch.stack(outs, dim=1)         # [B, T, H, W, input_size]
        return y.permute(0, 1, 4, 2, 3) if self.input_size != 1 else y.reshape(B, T, 1, H, W)
