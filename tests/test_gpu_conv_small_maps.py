"""The 3 x 3 convolution kernels (csrc/conv3x3.hip, unchanged) on the maps only the U-Net reaches: grids far smaller than the
8 x 16 pixel tile, down to 1 x 2, where most of a tile is masked and -- with circular padding -- the halo wraps onto the very
pixels of the tile.  Through `conv_ops.conv3x3` with autograd (forward, input gradients, weight and bias gradient), one- and
two-input forms, against float64 torch on the CPU with the reference, the per-element bounds and the helpers of
tests/test_gpu_conv_ops.py (|err| <= 1e-6 * S + ulp(result) + carried activation error; every element compared).
"""
import pytest
import torch

from test_gpu_conv_ops import C_, Z, bits, check, cl, reference

pytestmark = pytest.mark.gpu

GRIDS = [(1, 2), (2, 2), (2, 4), (4, 4), (4, 8)]
PADS = [(Z, Z), (Z, C_), (C_, Z), (C_, C_)]
FORMS = {"c5_n13": (5, 0, 13), "c48+48_n24": (48, 48, 24)}      # (C1, C2, Cout)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("pads", PADS, ids=lambda p: f"{p[0]}_{p[1]}")
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_conv3x3_on_small_maps(cuda, grid, pads, form):
    from dlwp_benchmark_amd import conv_ops
    H, W_ = grid
    C1, C2, Cout = FORMS[form]
    for B in (1, 3):
        gen = torch.Generator().manual_seed(7000 + 100 * H + 10 * W_ + B + C1)
        x = torch.randn(B, C1 + C2, H, W_, generator=gen)
        w = torch.randn(Cout, C1 + C2, 3, 3, generator=gen) / (3.0 * (C1 + C2) ** 0.5)
        b = torch.randn(Cout, generator=gen)
        gy = torch.randn(B, Cout, H, W_, generator=gen)
        y_ref, gx_ref, gw_ref, gb_ref, S, E = reference(x, w, b, gy, pads, "relu")
        xcl = cl(x)
        results = []
        for rep in range(2):
            x1 = xcl[..., :C1].contiguous().to(cuda).requires_grad_(True)
            x2 = xcl[..., C1:].contiguous().to(cuda).requires_grad_(True) if C2 else None
            wg, bg = w.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
            y = conv_ops.conv3x3(x1, wg, bg, pads, "relu", x2=x2)
            y.backward(cl(gy).to(cuda))
            torch.cuda.synchronize()
            results.append(dict(y=y.detach(), g1=x1.grad, g2=x2.grad if C2 else None, gw=wg.grad, gb=bg.grad))
        o = results[0]
        for k, v in o.items():
            assert v is None or torch.equal(bits(v), bits(results[1][k])), f"{k}: two runs on the same operands differ"
        print(f"B {B}, {H} x {W_}, {pads}, {form}")
        check("y", o["y"].permute(0, 3, 1, 2), y_ref, S["y"])
        gx = gx_ref.permute(0, 2, 3, 1)
        Sx, Ex = S["gx"].permute(0, 2, 3, 1), E["gx"].permute(0, 2, 3, 1)
        check("gx1", o["g1"], gx[..., :C1], Sx[..., :C1], Ex[..., :C1])
        if C2:
            check("gx2", o["g2"], gx[..., C1:], Sx[..., C1:], Ex[..., C1:])
        check("gw", o["gw"], gw_ref, S["gw"], E["gw"])
        check("gb", o["gb"], gb_ref, S["gb"], E["gb"])
