"""U-Net baseline of the weather benchmark (src/dlwpbench/models/unet/unet.py) on the hand-written convolution kernels: the
reference's constructor keywords, `forward(constants, prescribed, prognostic)` and `state_dict` keys (its CylinderPad takes a
Sequential slot of its own in front of every 3 x 3 convolution: `encoder.layers.0.1`, `encoder.layers.0.4`,
`encoder.layers.1.2`, `decoder.layers.0.1`, ...).  CylinderPad (circular in longitude, zeros in latitude) is the kernels'
per-axis padding mode, so no padded tensor is written.

`UNetHEALPix` is the reference's `UNetHPX` (same file): `[B, T, C, 12, n, n]` tensors, every 3 x 3 convolution in a
HEALPixLayer (`encoder.layers.{lvl}.{slot}.layers.1`), whose HEALPixPadding is the kernels' "healpix" padding mode.  Its levels
run on faces of n, n / 2, n / 4, ... pixels, down to 1 x 1 at the published HPX8 width: the small ones on the face-packed
kernels (conv_ops `pack_faces`).
"""
import torch.nn as nn

from ..conv_ops import PACKED_FACE_SIZES, Conv3x3
from ..nsbench.convlstm import Layers
from ..nsbench.unet import UNetDecoder, UNetEncoder, activation_name, check_grid, check_unet_config, pack_all, unet_call
from .convlstm import CYLINDER, FACES, HEALPIX
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
            raise NotImplementedError("UNet is the equirectangular model; the HEALPix mesh is UNetHEALPix")
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


# Largest face size that runs the face-packed kernels.  Faces of 1, 2 and 4 pixels always do (the default kernels refuse n = 1
# and multiply 4 and 16 useful rows of 128 at n = 2 and 4); n = 8 follows the measurement in docs/kernels/conv.md ("Face-packed
# HEALPix kernels", rule: packed only if its median is below the default kernel's by more than that kernel's own spread -- it is,
# for forward, input gradient and weight gradient at both measured widths: 0.59 - 0.81 of the default kernels' time).
PACK_FACES_UP_TO = 8


def packs_faces(n):
    """whether a level with n x n faces runs the face-packed 3 x 3 kernels"""
    return n in PACKED_FACE_SIZES and n <= PACK_FACES_UP_TO


class UNetHEALPix(nn.Module):
    """The reference's `UNetHPX`: `dlwpbench.UNet` on the HEALPix mesh.  Tensors are `[B, T | 1, C, 12, n, n]`; a network call
    runs on the folded `[(B * 12), n, n, C]` channels-last tensor (face index fastest, the reference's `(b f)`); pooling,
    up-convolution and the 1 x 1 output layer never cross a face, and every 3 x 3 convolution pads each face with the border
    pixels of its neighbour faces inside the kernel.  Level l has faces of n / 2^l pixels: `packs_faces` picks the face-packed
    kernels for the small ones.  Input window, residual output and rollout as in `UNet`.  Returns
    `[B, T - context_size, C, 12, n, n]`.

    ValueError in `forward` for a face count other than 12, faces that are not square and a face size that is not divisible by
    2 ** (levels - 1) (the reference fails in a `cat` there)."""

    def __init__(self, constant_channels=4, prescribed_channels=0, prognostic_channels=1, hidden_channels=(8, 16, 32),
                 n_convolutions=2, activation="th.nn.ReLU()", context_size=1, mesh="healpix", device=None, **kwargs):
        super().__init__()
        if mesh != "healpix":
            raise NotImplementedError("UNetHEALPix is the HEALPix model; the equirectangular mesh is UNet")
        hs, n = check_unet_config(hidden_channels, n_convolutions)
        if context_size < 1:
            raise ValueError("context_size must be >= 1: the first frame needs an initial condition")
        act = activation_name(activation)
        self.hidden_channels, self.n_convolutions, self.context_size, self.mesh = hs, n, context_size, mesh
        self.prognostic_channels = prognostic_channels
        in_channels = constant_channels + (prescribed_channels + prognostic_channels) * context_size
        kw = dict(pad_modes=HEALPIX)
        self.encoder = UNetEncoder(in_channels, hs, n, act, kw, wrap=Layers)
        self.decoder = UNetDecoder(hs, prognostic_channels, n, act, kw, wrap=Layers)
        if device is not None:
            self.to(device)

    def _dispatch(self, n):
        """every convolution of the level with faces of n / 2^l pixels gets that level's kernel family"""
        levels = len(self.hidden_channels)
        for lvl in range(levels):
            for layer in (self.encoder.layers[lvl], self.decoder.layers[levels - 1 - lvl]):
                for m in layer.modules():
                    if isinstance(m, Conv3x3):
                        m.pack_faces = packs_faces(n >> lvl)

    def forward(self, constants=None, prescribed=None, prognostic=None):
        """constants [B, 1, C, 12, n, n] | None, prescribed [B, T, C, 12, n, n] | None, prognostic [B, T, C, 12, n, n]"""
        if prognostic.dim() != 6 or prognostic.shape[3] != FACES:
            raise ValueError(f"prognostic must be [B, T, C, 12, n, n] (12 HEALPix faces), not {tuple(prognostic.shape)}")
        B, T, C, _, n, n2 = prognostic.shape
        if n != n2:
            raise ValueError(f"HEALPix faces are square: prognostic has {n} x {n2} faces")
        levels = len(self.hidden_channels)
        if n % (1 << (levels - 1)):
            raise ValueError(f"faces of {n} x {n} pixels cannot be pooled through {levels} levels: the face size must be divisible "
                             f"by {1 << (levels - 1)} (a skip connection would not fit its up-convolution)")
        if T <= self.context_size:
            raise ValueError(f"prognostic has {T} frames: more than context_size = {self.context_size} are needed")
        self._dispatch(n)
        packs = pack_all(self.encoder, self.decoder)

        def one_step(x_t):                                                          # [B, C, 12, n, n]
            x = x_t.permute(0, 2, 3, 4, 1).reshape(B * FACES, n, n, x_t.shape[1])    # folded channels-last frame (one copy)
            enc = self.encoder(x, packs)
            out = self.decoder(enc[-1], enc[::-1], packs)
            return out.view(B, FACES, n, n, out.shape[-1]).permute(0, 4, 1, 2, 3)

        return rollout(one_step, self.context_size, constants, prescribed, prognostic)


def model_class(type_name):
    """The class for a `type` string of the reference's YAML files: "UNetHPX" is `UNetHEALPix` (the name `UNetHPX` still raises
    here); every other name is the attribute of the same name of this package."""
    from .. import dlwpbench
    if type_name == "UNetHPX":
        return UNetHEALPix
    try:
        return getattr(dlwpbench, type_name)
    except AttributeError:
        raise ValueError(f"no model class {type_name!r} in dlwpbench ({', '.join(dlwpbench.__all__)})") from None


class UNetHPX(UNet):
    """The reference's name of the HEALPix variant.  The model is `UNetHEALPix` (`model_class("UNetHPX")`); this name still raises."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("UNetHPX: the U-Net on the HEALPix mesh is built as UNetHEALPix (dlwpbench.model_class('UNetHPX'))")
