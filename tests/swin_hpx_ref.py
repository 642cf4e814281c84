"""TEST INFRASTRUCTURE ONLY -- plain-torch restatement of the reference's SwinTransformerHPX
(src/dlwpbench/models/swintransformer/swin_transformer.py:745-896) on the blocks of oracle/swin_ref.py.

PINNED: tests/test_swin_hpx_ref.py checks it in float64 against tests/golden/swin_hpx_golden.npz, captured from the reference's
own class by tests/golden/make_swin_hpx_golden.py.

    faces2rect / rect2faces  <- _faces2rect :826-834 / _reshape_output :867-879
    swin_hpx                 <- _prepare_inputs :849-865 + one_step :645-677 + _reshape_output, in the working loop of
                                UNet.forward (unet.py:64-111; the class's own forward() raises at the second lead time)
one_step is oracle.swin_ref.dlwp_swin_one_step as it is: its windows come from cfg (img_height, img_width, patch_size), its token
map from the tensor it is given -- on this mesh the 3n x 4n canvas, so the two differ -- and it never pads.
"""
import torch

from oracle import swin_ref


def faces2rect(x):
    """[..., 12, n, n] -> [..., 3n, 4n]: face f at canvas rows (f // 4) n ..., columns (f % 4) n ..."""
    lead, n = x.shape[:-3], x.shape[-1]
    k = len(lead)
    return x.reshape(*lead, 3, 4, n, n).permute(*range(k), k, k + 2, k + 1, k + 3).reshape(*lead, 3 * n, 4 * n)


def rect2faces(x):
    """[..., 3n, 4n] -> [..., 12, n, n]"""
    lead, n = x.shape[:-2], x.shape[-2] // 3
    k = len(lead)
    return x.reshape(*lead, 3, n, 4, n).permute(*range(k), k, k + 2, k + 1, k + 3).reshape(*lead, 12, n, n)


def prepare_inputs(constants, prescribed, prognostic):
    """cat(constants[:, 0], prescribed "(t c)", prognostic "(t c)") on the canvas: [B, Cin, 3n, 4n]"""
    parts = [] if constants is None else [faces2rect(constants[:, 0])]
    if prescribed is not None:
        parts.append(faces2rect(prescribed.flatten(1, 2)))
    parts.append(faces2rect(prognostic.flatten(1, 2)))
    return torch.cat(parts, dim=1)


def swin_hpx(constants, prescribed, prognostic, p, cfg):
    """[B, T, C, 12, n, n] tensors -> [B, T - ctx, C, 12, n, n]"""
    ctx, outs = cfg["context_size"], []
    for t in range(ctx, prognostic.shape[1]):
        if t == ctx:
            prog_t = prognostic[:, t - ctx:t]
        else:
            prog_t = torch.cat([prognostic[:, max(0, t - ctx):ctx], torch.stack(outs, dim=1)[:, -ctx:]], dim=1)
        x_t = prepare_inputs(constants, None if prescribed is None else prescribed[:, t - ctx:t], prog_t)
        outs.append(prog_t[:, -1] + rect2faces(swin_ref.dlwp_swin_one_step(x_t, p, cfg)))
    return torch.stack(outs, dim=1)
