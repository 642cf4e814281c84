"""U-Net baseline of the weather benchmark (src/dlwpbench/models/unet/unet.py) on the hand-written convolution kernels: the
reference's constructor keywords, `forward(constants, prescribed, prognostic)` and `state_dict` keys (its CylinderPad takes a
Sequential slot of its own in front of every 3 x 3 convolution: `encoder.layers.0.1`, `encoder.layers.0.4`,
`encoder.layers.1.2`, `decoder.layers.0.1`, ...).  CylinderPad (circular in longitude, zeros in latitude) is the kernels'
per-axis padding mode, so no padded tensor is written.  Only the equirectangular mesh is built.
"""
import torch.nn as nn

from ..nsbench.unet import UNetDecoder, UNetEncoder, activation_name, check_grid, check_unet_config, pack_all, unet_call
from .convlstm import CYLINDER
from .rollout import rollout


class UNet(nn.Module):
    """The input of a step is `cat(constants, prescribed window, prognostic window)` with both windows `context_size` frames
    long and flattened over (time, channel); the output is a residual to the newest prognostic frame.  The prognostic window
    starts as `prognostic[:, :context_size]` and slides over the model's own frames (`prognostic[:, t_start:context_size] |
    outs[-context_size:]`); the prescribed window is always observed.  Returns the frames from `context_size` on:
    `[B, T - context_size, C, H, W]`.

    `mesh="healpix"` raises NotImplementedError.  `activation`: an nn.ReLU / nn.Tanh instance or the YAML string of one.
    H and W must be divisible by 2 ** (levels - 1).  Extra keywords are ignored; `device` moves the parameters."""

    def __init__(self, constant_channels=4, prescribed_channels=0, prognostic_channels=1, hidden_channels=(8, 16, 32),
                 n_convolutions=2, activation="th.nn.ReLU()", context_size=1, mesh="equirectangular", device=None, **kwargs):
        super().__init__()
        if mesh != "equirectangular":
            raise NotImplementedError("UNet is built on the equirectangular mesh only (the HEALPix U-Net is not built yet)")
        hs, n = check_unet_config(hidden_channels, n_convolutions)
        if context_size < 1:
            raise ValueError("context_size must be >= 1: the first frame needs an initial condition")
        act = activation_name(activation)
        self.hidden_channels, self.n_convolutions, self.context_size, self.mesh = hs, n, context_size, mesh
        self.prognostic_channels = prognostic_channels
        in_channels = constant_channels + (prescribed_channels + prognostic_channels) * context_size
        kw = dict(pad_modes=CYLINDER)
        self.encoder = UNetEncoder(in_channels, hs, n, act, kw, slots_before=1)
        self.decoder = UNetDecoder(hs, prognostic_channels, n, act, kw, slots_before=1)
        if device is not None:
            self.to(device)

    def forward(self, constants=None, prescribed=None, prognostic=None):
        """constants [B, 1, C, H, W] | None, prescribed [B, T, C, H, W] | None, prognostic [B, T, C, H, W]"""
        if prognostic.shape[1] <= self.context_size:
            raise ValueError(f"prognostic has {prognostic.shape[1]} frames: more than context_size = {self.context_size} are needed")
        check_grid(prognostic.shape[-2], prognostic.shape[-1], len(self.hidden_channels))
        packs = pack_all(self.encoder, self.decoder)
        return rollout(lambda x_t: unet_call(self.encoder, self.decoder, x_t, packs), self.context_size, constants, prescribed,
                       prognostic)


class UNetHPX(UNet):
    """The reference's HEALPix variant: not built yet (the 3 x 3 kernels have the padding, conv_ops "healpix"; the class is a follow-up)."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("UNetHPX, the U-Net on the HEALPix mesh, is not built yet")
