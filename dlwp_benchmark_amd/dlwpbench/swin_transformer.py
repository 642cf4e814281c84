"""dlwpbench SwinTransformer on libdlwpmi: constructor keys, forward signature and state_dict keys of
src/dlwpbench/models/swintransformer/swin_transformer.py:494-737.

Layers are the nsbench ones (../nsbench/swin_transformer.py: fused window attention, LayerNorm / MLP / merging GEMMs)
with (h, w) window pairs: every stage attends over its whole feature map (window = (H/p, W/p) halved per stage,
reference :542-571) with a half-map cyclic shift in the odd blocks.  Grids that would need window padding are refused:
the reference pads the wrong axes there (:218-222) and its BasicLayer raises.  Patch embedding pads
longitude circularly and latitude with zeros (:446-451).  The rollout is the dlwpbench loop in its working form
(rollout.py).
"""
import torch
import torch.nn as nn

from ..hpx_ops import faces_to_tokens, tokens_to_faces
from ..nsbench.swin_transformer import _NORMS, BasicLayer, PatchEmbed, PatchMerging, absolute_position_tokens
from ..rollout_ops import advance
from ..token_ops import DropPathPool, PatchConv2d, UpConvT2d
from .rollout import rollout


class SwinTransformer(nn.Module):
    def __init__(self, constant_channels: int = 4, prescribed_channels: int = 0, prognostic_channels: int = 1,
                 context_size: int = 1, img_height=224, img_width=196, patch_size=4, embed_dim=96, depths=[2, 2, 6, 2],
                 num_heads=[3, 6, 12, 24], mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0.2, norm_layer="nn.LayerNorm", ape=False, patch_norm=True, frozen_stages=-1,
                 use_checkpoint=False, mesh="equirectangular", window_size=None, **kwargs):
        """window_size (extra kwarg, not in the reference): None = the reference behaviour (whole-map windows); an int or
        (h, w) pair gives classic Swin windows with the CORRECT per-axis padding (constant latitude, circular longitude) --
        the reference's own block cannot run that case."""
        super().__init__()
        if mesh != "equirectangular":
            raise NotImplementedError(f"mesh {mesh!r}: this class runs the equirectangular mesh (5-D inputs, as the reference's); "
                                      "the HEALPix mesh is SwinTransformerHPX")
        self._build(constant_channels, prescribed_channels, prognostic_channels, context_size, img_height, img_width, patch_size,
                    embed_dim, depths, num_heads, mlp_ratio, qkv_bias, qk_scale, drop_rate, attn_drop_rate, drop_path_rate,
                    norm_layer, ape, patch_norm, frozen_stages, mesh, window_size, ("constant", "circular"))

    def _build(self, constant_channels, prescribed_channels, prognostic_channels, context_size, img_height, img_width, patch_size,
               embed_dim, depths, num_heads, mlp_ratio, qkv_bias, qk_scale, drop_rate, attn_drop_rate, drop_path_rate, norm_layer,
               ape, patch_norm, frozen_stages, mesh, window_size, pad_modes):
        """The module tree both meshes share (reference :520-607).  pad_modes: (latitude, longitude) padding of the patch embedding
        and the windows; the HEALPix class never pads (it refuses the sizes that would need it)."""
        if frozen_stages >= 0:
            raise NotImplementedError("frozen_stages >= 0 (a fine-tuning option: stop gradients of the first stages) is not "
                                      "built; the shipped configs use -1")
        if drop_rate or attn_drop_rate:
            raise NotImplementedError("dropout is not on the MI355X hot path (the shipped config uses drop_rate 0 and "
                                      "attn_drop_rate 0)")
        norm = _NORMS[norm_layer] if isinstance(norm_layer, str) else norm_layer
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]    # stochastic depth decay rule (:552)
        self.context_size, self.num_layers, self.embed_dim = context_size, len(depths), embed_dim
        self.img_height, self.img_width, self.mesh = img_height, img_width, mesh
        in_chans = constant_channels + (prescribed_channels + prognostic_channels) * context_size
        self.patch_embed = PatchEmbed(patch_size, in_chans, embed_dim, norm if patch_norm else None, pad_modes)
        res = (img_height // patch_size, img_width // patch_size)
        self.ape = ape
        if ape:     # learned [1, E, Wh0, Ww0] embedding added to the embedded patches (reference :540-547)
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, embed_dim, res[0], res[1]))
            nn.init.trunc_normal_(self.absolute_pos_embed, std=.02)
        self.layers = nn.ModuleList()
        for i in range(self.num_layers):
            if mesh == "equirectangular" and window_size is None and i < self.num_layers - 1 and (res[0] % 2 or res[1] % 2):
                raise NotImplementedError(f"stage {i} feature map {res} is odd: the reference's window padding is broken "
                                          "there (swin_transformer.py:218-222, SURVEY App. B-6)")
            self.layers.append(BasicLayer(int(embed_dim * 2 ** i), depths[i], num_heads[i],
                                          res if window_size is None else window_size, mlp_ratio, qkv_bias,
                                          qk_scale, drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm,
                                          downsample=PatchMerging if i < self.num_layers - 1 else None,
                                          padding_mode=pad_modes))
            res = (res[0] // 2, res[1] // 2)
        self.num_features = [int(embed_dim * 2 ** i) for i in range(self.num_layers)]
        for i, nf in enumerate(self.num_features):
            self.add_module(f"norm{i}", norm(nf))
        self.decoder = nn.ModuleList()
        for idx, i in enumerate(reversed(range(self.num_layers))):
            ch = int(embed_dim * 2 ** i)
            k = patch_size if i == 0 else 2
            self.decoder.append(nn.Sequential(
                UpConvT2d(ch if idx == 0 else 2 * ch, ch if i == 0 else ch // 2, kernel_size=k, stride=k), nn.GELU()))
        self.final = PatchConv2d(embed_dim, prognostic_channels, kernel_size=1)

    def one_step(self, x):
        if getattr(self, "_drop_pool", None) is None:      # built lazily: after construction, copies and loads
            object.__setattr__(self, "_drop_pool", DropPathPool(self))
        self._drop_pool.draw(x.shape[0], x.device)        # every block's stochastic-depth mask for this call, one draw
        x = self.patch_embed(x)
        Wh, Ww = x.shape[2], x.shape[3]
        x = x.flatten(2).transpose(1, 2)
        if self.ape:
            x = x + absolute_position_tokens(self.absolute_pos_embed, Wh, Ww).to(x.dtype)
        # U-decoder on channels-last tokens (reference :580-591 / one_step): stage outputs stay [B, H, W, C], the transposed
        # convolutions are a GEMM + one interleave kernel each, the 1 x 1 head is a GEMM; NCHW only for the returned frame
        feats = []
        for i, layer in enumerate(self.layers):
            x_out, H, W, x, Wh, Ww = layer(x, Wh, Ww)
            x_out = getattr(self, f"norm{i}")(x_out)
            feats.append(x_out.reshape(-1, H, W, self.num_features[i]))
        feats.reverse()
        y = None
        for idx, up in enumerate(self.decoder):
            y = up[0].forward_tokens(feats[idx] if idx == 0 else torch.cat([feats[idx], y], dim=-1), act=1)   # GELU fused
        y = self.final.forward_tokens(y)                      # [B, H, W, out]
        return y.permute(0, 3, 1, 2)

    def forward(self, constants: torch.Tensor = None, prescribed: torch.Tensor = None,
                prognostic: torch.Tensor = None) -> torch.Tensor:
        return rollout(self.one_step, self.context_size, constants, prescribed, prognostic)


class SwinTransformerHPX(SwinTransformer):
    """SwinTransformerHPX (reference :745-896): the same network on the HEALPix mesh.  Tensors are [B, T, C, 12, n, n]; the 12 faces
    of a frame form a 3n x 4n canvas (_faces2rect :826-834: north faces 0-3 on top, equator, south) that the network reads as an
    image.  Stage i attends in windows of (img_height // patch, img_width // patch) // 2^i -- the CONSTRUCTOR's sizes, with
    img_height = img_width = n and patch 1 exactly one face -- on the token map (3n / patch, 4n / patch) // 2^i of the INPUT, with a
    torch.roll cyclic shift of window // 2 on both canvas axes in the odd blocks and no padding anywhere on this mesh (:220-230).

    Per lead time: ONE gather launch builds the patch-embedding rows from the face tensors (hpx_ops.faces_to_tokens replaces three
    _faces2rect calls, the cat and the convolution's unfold; the sliding windows are read in place), ONE scatter launch turns the
    head's canvas into the frame-layout residual (hpx_ops.tokens_to_faces, _reshape_output :867-879), rollout_ops.advance slides the
    window.  The rollout is the loop of UNet.forward around this (the reference's own forward() raises at the second lead time,
    SURVEY App. B-1).

    Refused with a ValueError that names the sizes, where the reference fails with a shape error or a missing method (hpx_pad,
    :454): a canvas not divisible by the patch, a stage whose map is not a multiple of its window, an odd map in front of a
    PatchMerging, a window axis that reaches 0."""

    def __init__(self, constant_channels: int = 4, prescribed_channels: int = 0, prognostic_channels: int = 1,
                 context_size: int = 10, img_height=224, img_width=196, patch_size=4, embed_dim=96, depths=[2, 2, 6, 2],
                 num_heads=[3, 6, 12, 24], mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0.2, norm_layer="nn.LayerNorm", ape=False, patch_norm=True, frozen_stages=-1,
                 use_checkpoint=False, mesh="healpix", **kwargs):
        nn.Module.__init__(self)
        if mesh != "healpix":
            raise NotImplementedError(f"mesh {mesh!r}: this class runs the HEALPix mesh (6-D inputs); the equirectangular mesh is "
                                      "SwinTransformer")
        if "window_size" in kwargs:
            raise ValueError("window_size is the equirectangular SwinTransformer's keyword: on the HEALPix mesh the windows are "
                             "(img_height // patch_size, img_width // patch_size) // 2^stage, as in the reference")
        res = (img_height // patch_size, img_width // patch_size)
        self.windows = [(res[0] >> i, res[1] >> i) for i in range(len(depths))]
        for i, w in enumerate(self.windows):
            if w[0] < 1 or w[1] < 1:
                raise ValueError(f"stage {i} window {w} = (img_height {img_height}, img_width {img_width}) // patch_size {patch_size} "
                                 f"// 2^{i} has an empty axis")
        self._build(constant_channels, prescribed_channels, prognostic_channels, context_size, img_height, img_width, patch_size,
                    embed_dim, depths, num_heads, mlp_ratio, qkv_bias, qk_scale, drop_rate, attn_drop_rate, drop_path_rate,
                    norm_layer, ape, patch_norm, frozen_stages, mesh, None, ("constant", "constant"))
        self.channels = (constant_channels, prescribed_channels, prognostic_channels)

    def check_sizes(self, n):
        """The token map of every stage for faces of n x n; ValueError where the reference cannot run them."""
        ph, pw = self.patch_embed.patch_size
        if (3 * n) % ph or (4 * n) % pw:
            raise ValueError(f"canvas {3 * n} x {4 * n} (faces of {n} x {n}) is not divisible by the patch {ph} x {pw}")
        m, maps = (3 * n // ph, 4 * n // pw), []
        for i, w in enumerate(self.windows):
            if m[0] < 1 or m[1] < 1 or m[0] % w[0] or m[1] % w[1]:
                raise ValueError(f"stage {i} token map {m} (faces of {n} x {n}) is not a multiple of its window {w}: nothing pads "
                                 "on the HEALPix mesh")
            maps.append(m)
            if i < self.num_layers - 1:
                if m[0] % 2 or m[1] % 2:
                    raise ValueError(f"stage {i} token map {m} (faces of {n} x {n}) is odd in front of its PatchMerging")
                m = (m[0] // 2, m[1] // 2)
        return maps

    def one_step(self, sources, n):
        """sources: the face tensors [B, C_k, 12, n, n] in channel order (constants, prescribed window, prognostic window)
        -> the residual in frame layout [B, C, 12, n, n]"""
        B = sources[-1].shape[0]
        if getattr(self, "_drop_pool", None) is None:
            object.__setattr__(self, "_drop_pool", DropPathPool(self))
        self._drop_pool.draw(B, sources[-1].device)
        rows = faces_to_tokens(sources, n, self.patch_embed.patch_size)       # [B, Wh, Ww, Cin*ph*pw]
        Wh, Ww = rows.shape[1], rows.shape[2]
        x = self.patch_embed.forward_rows(rows.reshape(B * Wh * Ww, -1)).reshape(B, Wh * Ww, self.embed_dim)
        if self.ape:
            x = x + absolute_position_tokens(self.absolute_pos_embed, Wh, Ww).to(x.dtype)
        feats = []
        for i, layer in enumerate(self.layers):
            x_out, H, W, x, Wh, Ww = layer(x, Wh, Ww)
            x_out = getattr(self, f"norm{i}")(x_out)
            feats.append(x_out.reshape(-1, H, W, self.num_features[i]))
        feats.reverse()
        y = None
        for idx, up in enumerate(self.decoder):
            y = up[0].forward_tokens(feats[idx] if idx == 0 else torch.cat([feats[idx], y], dim=-1), act=1)   # GELU fused
        return tokens_to_faces(self.final.forward_tokens(y), n)               # [B, 3n, 4n, C] -> [B, C, 12, n, n]

    def forward(self, constants: torch.Tensor = None, prescribed: torch.Tensor = None,
                prognostic: torch.Tensor = None) -> torch.Tensor:
        ctx = self.context_size
        for name, t, C in zip(("constants", "prescribed", "prognostic"), (constants, prescribed, prognostic), self.channels):
            if t is None:
                if C or name == "prognostic":
                    raise ValueError(f"{name} is missing (the model was built with {C} {name} channels)")
                continue
            if t.dim() != 6 or t.shape[3] != 12 or t.shape[4] != t.shape[5] or t.shape[2] != C:
                raise ValueError(f"{name}: expected [B, T, {C}, 12, n, n] with square faces, got {tuple(t.shape)}")
        n, T = prognostic.shape[-1], prognostic.shape[1]
        for name, t in (("constants", constants), ("prescribed", prescribed)):
            if t is not None and (t.shape[-1] != n or t.shape[0] != prognostic.shape[0]):
                raise ValueError(f"{name} {tuple(t.shape)} does not match prognostic {tuple(prognostic.shape)}")
        if T <= ctx:
            raise ValueError(f"prognostic has T = {T} frames: the rollout needs more than context_size = {ctx}")
        if prescribed is not None and prescribed.shape[1] < T - 1:
            raise ValueError(f"prescribed has {prescribed.shape[1]} frames, the rollout reads {T - 1}")
        self.check_sizes(n)
        outs, win, flat = [], prognostic[:, 0:ctx], None
        const = None if constants is None or not self.channels[0] else constants[:, 0]
        for t in range(ctx, T):
            presc = None if prescribed is None or not self.channels[1] else prescribed[:, t - ctx:t].flatten(1, 2)
            delta = self.one_step([const, presc, flat if flat is not None else win.flatten(1, 2)], n)
            win, flat, out = advance(win, delta, want_next=t + 1 < T)
            outs.append(out)
        return torch.stack(outs, dim=1)
