"""U-Net baseline of the Navier-Stokes benchmark (src/nsbench/models/unet/unet.py) on the hand-written convolution kernels
(conv_ops): constructor keywords, `forward` signature and `state_dict` keys are the reference's, so its checkpoints load with
`load_state_dict(strict=True)`.

Inside, activations are channels-last `[B, H, W, C]`.  Every 3 x 3 convolution and its activation is one launch with the padding
resolved in the kernel; the decoder's `cat([skip, x])` is never written (the convolution reads its input channels from two
tensors); pool, up-convolution and the 1 x 1 output layer are the kernels of csrc/unet_ops.hip.  The packed weight images are
refreshed once per forward pass and shared by all time steps.
"""
import torch.nn as nn

from ..conv_ops import PAD, Conv1x1, Conv3x3, UpConv2x2, avg_pool2x2
from ..rollout_ops import ns_rollout
from .convlstm import Layers, _Slot

ACTIVATIONS = {"th.nn.ReLU()": "relu", "torch.nn.ReLU()": "relu", "nn.ReLU()": "relu",
               "th.nn.Tanh()": "tanh", "torch.nn.Tanh()": "tanh", "nn.Tanh()": "tanh"}


def activation_name(activation):
    """"relu" / "tanh" of an nn.ReLU / nn.Tanh instance or of the config strings of the reference's YAML files (matched by
    table: the reference evaluates the string)."""
    if isinstance(activation, str) and activation.replace(" ", "") in ACTIVATIONS:
        return ACTIVATIONS[activation.replace(" ", "")]
    if isinstance(activation, nn.ReLU):
        return "relu"
    if isinstance(activation, nn.Tanh):
        return "tanh"
    raise NotImplementedError(f"activation {activation!r}: the convolution kernels fuse nn.ReLU() and nn.Tanh() only")


def check_unet_config(hidden_channels, n_convolutions):
    hs = [int(h) for h in hidden_channels]
    if not hs or any(h < 1 for h in hs):
        raise ValueError(f"hidden_channels must be a non-empty list of positive widths, not {hidden_channels!r}")
    if int(n_convolutions) < 2:
        raise ValueError(f"n_convolutions must be >= 2 (got {n_convolutions}): the bottom level runs n_convolutions // 2 of them "
                         "in the encoder and as many in the decoder, and with none the reference builds a channel mismatch")
    return hs, int(n_convolutions)


def check_grid(H, W, levels):
    for lvl in range(1, levels):
        if H % (1 << lvl) or W % (1 << lvl):
            raise ValueError(f"a {H} x {W} grid cannot be pooled to level {lvl} of {levels}: height and width must be divisible "
                             f"by {1 << (levels - 1)} (the skip connection of level {lvl - 1} would not fit its up-convolution)")


class _Pool(_Slot):
    """Placeholder at the index of the reference's AvgPool2d; the encoder runs `avg_pool2x2` there."""


def run_level(layer, x, packs, skip=None):
    """The modules of one level's Sequential on a channels-last tensor; with `skip` the first convolution reads
    `skip | x` as two tensors (the decoder's concatenation)."""
    for m in layer:
        if isinstance(m, Layers):
            m = m.conv
        if isinstance(m, _Pool):
            x = avg_pool2x2(x)
        elif isinstance(m, Conv3x3):
            x = m.forward_cl(x, packed=packs[m]) if skip is None else m.forward_cl(skip, x2=x, packed=packs[m])
            skip = None
        elif isinstance(m, UpConv2x2):
            x = m.forward_cl(x)
    return x


class UNetEncoder(nn.Module):
    """levels of [pool (not at the top),] n x (3 x 3 convolution + activation); the bottom level runs n // 2 of them.
    slots_before: parameter-free modules in front of every convolution (1 in dlwpbench: the reference's CylinderPad).
    wrap: a module class that takes the convolution's slot and holds it (Layers: the reference's HEALPixLayer)."""

    def __init__(self, in_channels, hidden_channels, n_convolutions, act, conv_kw, slots_before=0, wrap=None):
        super().__init__()
        channels = [in_channels] + list(hidden_channels)
        layers = []
        for i in range(len(hidden_channels)):
            layer = [_Pool()] if i > 0 else []
            n = n_convolutions // 2 if i == len(hidden_channels) - 1 else n_convolutions
            for k in range(n):
                layer += [_Slot() for _ in range(slots_before)]
                conv = Conv3x3(channels[i] if k == 0 else channels[i + 1], channels[i + 1], act=act, **conv_kw)
                layer += [wrap(conv) if wrap else conv, _Slot()]
            layers.append(nn.Sequential(*layer))
        self.layers = nn.ModuleList(layers)

    def forward(self, x, packs):
        """channels-last x -> the output of every level (top first)"""
        outs = []
        for layer in self.layers:
            x = run_level(layer, x, packs)
            outs.append(x)
        return outs


class UNetDecoder(nn.Module):
    """bottom to top: n x (3 x 3 convolution + activation) [+ 2 x 2 up-convolution (not at the top)], then the 1 x 1 output
    layer.  Above the bottom the first convolution of a level reads `skip | upsampled` as two tensors."""

    def __init__(self, hidden_channels, out_channels, n_convolutions, act, conv_kw, slots_before=0, wrap=None):
        super().__init__()
        hs = list(hidden_channels)[::-1]
        layers = []
        for i, h in enumerate(hs):
            layer = []
            n = n_convolutions // 2 if i == 0 else n_convolutions
            for k in range(n):
                layer += [_Slot() for _ in range(slots_before)]
                conv = Conv3x3((h if i == 0 else 2 * h) if k == 0 else h, h, act=act, **conv_kw)
                layer += [wrap(conv) if wrap else conv, _Slot()]
            if i < len(hs) - 1:
                layer.append(UpConv2x2(h, hs[i + 1]))
            layers.append(nn.Sequential(*layer))
        self.layers = nn.ModuleList(layers)
        self.output_layer = Conv1x1(hs[-1], out_channels)

    def forward(self, x, skips, packs):
        for i, layer in enumerate(self.layers):
            x = run_level(layer, x, packs, skip=skips[i] if i > 0 else None)
        return self.output_layer.forward_cl(x)


def unet_call(encoder, decoder, x_cf, packs):
    """one network call: channels-first [B, C, H, W] in (one permute copy to channels-last), channels-first view out"""
    enc = encoder(x_cf.permute(0, 2, 3, 1).contiguous(), packs)
    return decoder(enc[-1], enc[::-1], packs).permute(0, 3, 1, 2)


def pack_all(*modules):
    return {m: m.pack() for mod in modules for m in mod.modules() if isinstance(m, Conv3x3)}


class UNet(nn.Module):
    """`forward(x [B, T, D, H, W], teacher_forcing_steps)` -> `[B, T, D, H, W]`.  The network sees the last `context_size`
    frames flattened over (time, channel) and predicts a residual to the newest of them:
    * frames t < context_size - 1 pass the input through (the window is not full yet);
    * while t < teacher_forcing_steps the window holds observations, afterwards the model's own frames; in between the
      reference's mixed window `observations | own frames`;
    so `out_channels` must equal `in_channels`.  `padding_mode`: "zeros" or "circular" (both axes).  `activation`: an nn.ReLU /
    nn.Tanh instance or the YAML string of one.  H and W must be divisible by 2 ** (levels - 1).  Extra keywords (`type`,
    `name`, ...) are ignored; `device` moves the parameters."""

    def __init__(self, in_channels=2, hidden_channels=(8, 16, 32), out_channels=1, n_convolutions=2, activation="th.nn.ReLU()",
                 padding_mode="zeros", context_size=1, device=None, **kwargs):
        super().__init__()
        hs, n = check_unet_config(hidden_channels, n_convolutions)
        if padding_mode not in PAD:
            raise ValueError(f"padding_mode must be 'zeros' or 'circular', not {padding_mode!r}")
        act = activation_name(activation)
        self.in_channels, self.out_channels, self.hidden_channels = in_channels, out_channels, hs
        self.n_convolutions, self.padding_mode, self.context_size = n, padding_mode, context_size
        kw = dict(padding_mode=padding_mode)
        self.encoder = UNetEncoder(in_channels * context_size, hs, n, act, kw)
        self.decoder = UNetDecoder(hs, out_channels, n, act, kw)
        if device is not None:
            self.to(device)

    def forward(self, x, teacher_forcing_steps=50):
        check_grid(x.shape[-2], x.shape[-1], len(self.hidden_channels))
        packs = pack_all(self.encoder, self.decoder)
        return ns_rollout(lambda x_t: unet_call(self.encoder, self.decoder, x_t, packs), x, teacher_forcing_steps, self.context_size)
