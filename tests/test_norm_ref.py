"""The float64 closed forms of tests/norm_ref.py against torch autograd of the float64 DEFINITION of each operation (the definition
written out and differentiated, never torch's fused normalisation ops: the fused CPU InstanceNorm backward disagrees with the definition
at B = 1, see test_gpu_shipped_configs.py).  Both sides are float64, so agreement is held to 1e-12 of the max norm: a few hundred
float64 roundings (2^-53 = 1.1e-16 each) over rows of at most 260 elements, nothing measured."""
import pytest
import torch

import norm_ref

TOL = 1e-12


def close(got, want):
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert (got - want).abs().max().item() <= TOL * want.abs().max().item()


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("T,C", [(5, 7), (3, 96), (2, 260)])
@pytest.mark.parametrize("residual", [False, True])
def test_layernorm_closed_forms(T, C, eps, residual):
    g = torch.Generator().manual_seed(100 * T + C)
    x = (2 * torch.randn(T, C, generator=g, dtype=torch.float64) + 0.5).requires_grad_()
    gamma = (1 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_()
    beta = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_()
    gy = torch.randn(T, C, generator=g, dtype=torch.float64)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma + beta
    out = y + x if residual else y                 # a pre-norm block: the identity path hands x the upstream gradient as well,
    gx, gg, gb = torch.autograd.grad(out, (x, gamma, beta), gy)
    gadd = gy if residual else None                # which the closed form takes as gadd
    y_c, mean_c, rstd_c = norm_ref.layernorm_fwd(x.detach(), gamma.detach(), beta.detach(), eps)
    close(y_c, y.detach())
    close(mean_c, mean.detach()[:, 0])
    close(rstd_c, (var.detach()[:, 0] + eps) ** -0.5)
    gx_c, gg_c, gb_c = norm_ref.layernorm_bwd(x.detach(), gamma.detach(), mean_c, rstd_c, gy, gadd)
    close(gx_c, gx)
    close(gg_c, gg)
    close(gb_c, gb)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("B,C,H,W", [(1, 3, 5, 5), (2, 4, 7, 3)])
@pytest.mark.parametrize("residual", [False, True])
def test_instancenorm_closed_forms(B, C, H, W, eps, residual):
    g = torch.Generator().manual_seed(B + 10 * C + 100 * H)
    P = H * W
    x = (2 * torch.randn(B, P, C, generator=g, dtype=torch.float64) + 0.5).requires_grad_()      # channels last: [B][H W][C]
    gamma = (1 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_()
    beta = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_()
    res = torch.randn(B, P, C, generator=g, dtype=torch.float64) if residual else None
    gy = torch.randn(B, P, C, generator=g, dtype=torch.float64)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma + beta
    if res is not None:
        y = y + res
    gx, gg, gb = torch.autograd.grad(y, (x, gamma, beta), gy)
    y_c, mean_c, rstd_c = norm_ref.instnorm_fwd(x.detach(), gamma.detach(), beta.detach(), eps, res)
    close(y_c, y.detach())
    close(mean_c, mean.detach()[:, 0])
    close(rstd_c, (var.detach()[:, 0] + eps) ** -0.5)
    gx_c, gg_c, gb_c = norm_ref.instnorm_bwd(x.detach(), gamma.detach(), mean_c, rstd_c, gy)
    close(gx_c, gx)
    close(gg_c, gg)
    close(gb_c, gb)
