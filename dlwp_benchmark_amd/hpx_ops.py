"""HEALPix faces <-> the patch tokens of the 3n x 4n canvas, one libdlwpmi launch per direction (csrc/hpx_canvas.hip).

Reference: SwinTransformerHPX (src/dlwpbench/models/swintransformer/swin_transformer.py:745-896) lays the 12 faces of a frame out
on a rectangle -- face f, pixel (y, x) -> canvas row (f // 4) n + y, column (f % 4) n + x (_faces2rect :826-834) -- once per
input tensor and lead time, concatenates the canvases (_prepare_inputs :849-865), lets the patch embedding unfold the result, and
splits the head's canvas into faces again (_reshape_output :867-879).

`faces_to_tokens` builds the patch-embedding rows straight from the face tensors (sliding windows are read in place through
their batch strides); `tokens_to_faces` turns the head's channels-last canvas into the frame layout rollout_ops.advance takes.
Each is the other's adjoint, so the backward of one is a launch of the other.  No torch fallback: CPU tensors raise DlwpError.
"""
import numpy as np
import torch

from . import lib as L
from .rollout_ops import _batch_view, _p


def canvas_index(n):
    """(row, column) on the 3n x 4n canvas of every (face, y, x): two int64 arrays [12, n, n]."""
    f, y, x = np.meshgrid(np.arange(12), np.arange(n), np.arange(n), indexing="ij")
    return (f // 4) * n + y, (f % 4) * n + x


def _check_faces(t, n, what):
    if t.dim() != 5 or t.shape[2] != 12 or t.shape[3] != n or t.shape[4] != n:
        raise ValueError(f"{what}: expected [B, C, 12, {n}, {n}], got {tuple(t.shape)}")


class _FacesToTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, patch, *sources):
        ph, pw = patch
        B, dev = sources[0].shape[0], sources[0].device
        args, keep, Ctot = [], [], 0
        for s in sources:
            _check_faces(s, n, "faces_to_tokens")
            if s.shape[0] != B:
                raise ValueError(f"faces_to_tokens: batch sizes differ ({s.shape[0]} and {B})")
            v, bs = _batch_view(s.detach())
            keep.append(v)
            args += [_p(v), bs, s.shape[1]]
            Ctot += s.shape[1]
        args += [None, 0, 0] * (3 - len(sources))
        if (3 * n) % ph or (4 * n) % pw:
            raise ValueError(f"faces_to_tokens: canvas {3 * n} x {4 * n} is not divisible by the patch {ph} x {pw}")
        tok = torch.empty(B, 3 * n // ph, 4 * n // pw, Ctot * ph * pw, device=dev)
        L.check(L.load().dlwp_hpx_canvas_gather(*args, L.ptr(tok), B, n, ph, pw, L.stream()))
        ctx.cfg = (B, n, ph, pw, Ctot, sources[-1].shape[1])
        return tok

    @staticmethod
    def backward(ctx, g_tok):
        B, n, ph, pw, Ctot, C = ctx.cfg
        g_last = None
        if ctx.needs_input_grad[-1]:       # only the prognostic window can need a gradient: one channel range
            g = g_tok.contiguous().float()
            g_last = torch.empty(B, C, 12, n, n, device=g.device)
            L.check(L.load().dlwp_hpx_canvas_scatter(L.ptr(g), L.ptr(g_last), B, n, ph, pw, Ctot, Ctot - C, C, L.stream()))
        return (None,) * (len(ctx.needs_input_grad) - 1) + (g_last,)


class _TokensToFacesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tok, n):
        if tok.dim() != 4 or tok.shape[1] != 3 * n or tok.shape[2] != 4 * n:
            raise ValueError(f"tokens_to_faces: expected [B, {3 * n}, {4 * n}, C], got {tuple(tok.shape)}")
        B, C = tok.shape[0], tok.shape[3]
        t = tok.contiguous().float()
        faces = torch.empty(B, C, 12, n, n, device=tok.device)
        L.check(L.load().dlwp_hpx_canvas_scatter(L.ptr(t), L.ptr(faces), B, n, 1, 1, C, 0, C, L.stream()))
        ctx.cfg = (B, n, C)
        return faces

    @staticmethod
    def backward(ctx, g_faces):
        B, n, C = ctx.cfg
        g, bs = _batch_view(g_faces)
        g_tok = torch.empty(B, 3 * n, 4 * n, C, device=g.device)
        L.check(L.load().dlwp_hpx_canvas_gather(_p(g), bs, C, None, 0, 0, None, 0, 0, L.ptr(g_tok), B, n, 1, 1, L.stream()))
        return g_tok, None


def faces_to_tokens(sources, n, patch=(1, 1)):
    """sources: one to three [B, C_k, 12, n, n] tensors (or views whose samples are dense blocks: `prescribed[:, t-ctx:t]`
    flattened over (time, channel), the flattened window rollout_ops.advance returns) -> [B, 3n/ph, 4n/pw, Ctot*ph*pw], the
    canvases concatenated along the channel in list order and unfolded into patch rows (K order of a [O, C, ph, pw] weight).
    Only the last source is differentiable; an earlier one that requires a gradient is refused."""
    sources = [s for s in sources if s is not None]
    if not 1 <= len(sources) <= 3:
        raise ValueError(f"faces_to_tokens takes one to three sources, got {len(sources)}")
    if torch.is_grad_enabled() and any(s.requires_grad for s in sources[:-1]):
        raise ValueError("faces_to_tokens: only the last source is differentiable (the backward pass scatters one channel range); "
                         "detach the others or pass the tensor that needs a gradient last")
    patch = tuple(patch) if isinstance(patch, (tuple, list)) else (patch, patch)
    return _FacesToTokensFn.apply(int(n), (int(patch[0]), int(patch[1])), *sources)


def tokens_to_faces(tok, n):
    """channels-last canvas [B, 3n, 4n, C] -> faces [B, C, 12, n, n] (_reshape_output :867-879)"""
    return _TokensToFacesFn.apply(tok, int(n))
