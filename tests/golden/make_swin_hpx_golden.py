#!/usr/bin/env python3
"""Golden vectors for the dlwpbench SwinTransformerHPX, produced by IMPORTING the reference's class
(src/dlwpbench/models/swintransformer/swin_transformer.py:745-896) in this container, with the timm stub of
make_dlwp_swin_golden.py (the class needs no graph library).

(faces)  n 8, patch 1, img 8 x 8 -- one window per face -- a single lead time through the reference's own forward();
(patch2) n 8, patch 2, img 8 x 8: maps 12 x 16 then 6 x 8, windows (4, 4) then (2, 2), three lead times with context 2;
(cross)  n 4, patch 1, img 6 x 8: windows (6, 8) then (3, 4) straddle the faces, ape=True, two lead times with context 2.
The reference's forward() raises at the second lead time: there the loop of UNet.forward (unet.py:64-111) is
driven by hand around the class's own _prepare_inputs, one_step and _reshape_output.
(map) the canvas of an arange face tensor and its _reshape_output, for the face <-> canvas index test.

    python tests/golden/make_swin_hpx_golden.py
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_dlwp_swin_golden import load_reference  # noqa: E402

COMMON = dict(constant_channels=2, prescribed_channels=1, prognostic_channels=3, embed_dim=8, depths=[2, 2], num_heads=[2, 2],
              drop_path_rate=0.0)
CASES = {"faces": dict(n=8, T=2, patch_size=1, img_height=8, img_width=8, context_size=1),
         "patch2": dict(n=8, T=5, patch_size=2, img_height=8, img_width=8, context_size=2),
         "cross": dict(n=4, T=4, patch_size=1, img_height=6, img_width=8, context_size=2, ape=True)}


def main():
    ref = load_reference()
    torch.manual_seed(4242)
    out = {}
    for tag, case in CASES.items():
        cfg = dict(COMMON, **case)
        n, T = cfg.pop("n"), cfg.pop("T")
        net = ref.SwinTransformerHPX(**cfg)
        with torch.no_grad():
            for name, p in net.named_parameters():
                if "relative_position_bias_table" in name:
                    p.mul_(25.0)
        torch.nn.Module.train(net, False)   # the class overrides train() (:739-742)
        B, ctx = 2, cfg["context_size"]
        constants = torch.randn(B, 1, cfg["constant_channels"], 12, n, n)
        prescribed = torch.randn(B, T, cfg["prescribed_channels"], 12, n, n)
        prognostic = torch.randn(B, T, cfg["prognostic_channels"], 12, n, n)
        target = torch.randn(B, T - ctx, cfg["prognostic_channels"], 12, n, n)
        if tag == "faces":
            y = net(constants=constants, prescribed=prescribed, prognostic=prognostic)
        else:
            outs = []
            for t in range(ctx, T):
                prog_t = prognostic[:, t - ctx:t] if t == ctx else torch.cat(
                    [prognostic[:, max(0, t - ctx):ctx], torch.stack(outs, dim=1)[:, -ctx:]], dim=1)
                x_t = net._prepare_inputs(constants=constants, prescribed=prescribed[:, t - ctx:t], prognostic=prog_t)
                outs.append(prog_t[:, -1] + net._reshape_output(net.one_step(x_t)))
            y = torch.stack(outs, dim=1)
        loss = torch.nn.functional.mse_loss(y, target)
        loss.backward()
        names = [name for name, _ in net.named_parameters()]
        out.update({f"{tag}_constants": constants.numpy(), f"{tag}_prescribed": prescribed.numpy(),
                    f"{tag}_prognostic": prognostic.numpy(), f"{tag}_target": target.numpy(), f"{tag}_y": y.detach().numpy(),
                    f"{tag}_loss": np.float32(loss.item()), f"{tag}_order": np.array(names)})
        out.update({f"{tag}_p_{name}": p.detach().numpy() for name, p in net.named_parameters()})
        out.update({f"{tag}_g_{name}": p.grad.numpy() for name, p in net.named_parameters() if p.grad is not None})
        if tag == "faces":
            faces = torch.arange(12 * 3 * 3, dtype=torch.float32).reshape(1, 1, 12, 3, 3)
            canvas = net._faces2rect(faces)
            out["map_canvas"] = canvas[0, 0].numpy().astype(np.int64)
            out["map_faces"] = net._reshape_output(canvas)[0, 0].numpy().astype(np.int64)
    path = os.path.join(OUT, "swin_hpx_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
