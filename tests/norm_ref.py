"""Plain float64 closed forms of the normalisation family (csrc/norm_ops.hip, csrc/instnorm.hip), written out so that the GPU tests
compare the kernels with arithmetic that shares nothing with them.  tests/test_norm_ref.py holds each form to torch autograd of the
float64 definition.  Every function takes and returns float64 tensors (inputs of another type are widened)."""
import torch


def layernorm_fwd(x, gamma, beta, eps):
    """x [T][C] -> (y, mean [T], rstd [T]); biased variance over the row, as nn.LayerNorm"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.sum(1) / x.shape[1]
    d = x - mean[:, None]
    rstd = ((d * d).sum(1) / x.shape[1] + eps) ** -0.5
    return d * rstd[:, None] * gamma + beta, mean, rstd


def layernorm_bwd(x, gamma, mean, rstd, gy, gadd=None):
    """(gx, ggamma, gbeta) from the saved statistics; gadd: a gradient that reached x along a residual branch, added to gx"""
    x, gamma, mean, rstd, gy = x.double(), gamma.double(), mean.double(), rstd.double(), gy.double()
    C = x.shape[1]
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = gy * gamma
    s1 = gg.sum(1, keepdim=True) / C
    s2 = (gg * xh).sum(1, keepdim=True) / C
    gx = rstd[:, None] * (gg - s1 - xh * s2)
    if gadd is not None:
        gx = gx + gadd.double()
    return gx, (gy * xh).sum(0), gy.sum(0)


def instnorm_fwd(x, gamma, beta, eps, residual=None):
    """x [B][P][C] -> (y, mean [B][C], rstd [B][C]): statistics per sample and channel over the P tokens, biased variance, as
    nn.InstanceNorm2d(affine=True, track_running_stats=False) on channels-last data"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    P = x.shape[1]
    mean = x.sum(1) / P
    d = x - mean[:, None, :]
    rstd = ((d * d).sum(1) / P + eps) ** -0.5
    y = d * rstd[:, None, :] * gamma + beta
    if residual is not None:
        y = y + residual.double()
    return y, mean, rstd


def instnorm_bwd(x, gamma, mean, rstd, gy):
    """(gx, ggamma, gbeta) from the saved statistics"""
    x, gamma, mean, rstd, gy = x.double(), gamma.double(), mean.double(), rstd.double(), gy.double()
    P = x.shape[1]
    xh = (x - mean[:, None, :]) * rstd[:, None, :]
    s1 = gy.sum(1, keepdim=True) / P
    s2 = (gy * xh).sum(1, keepdim=True) / P
    gx = (rstd * gamma)[:, None, :] * (gy - s1 - xh * s2)
    return gx, (gy * xh).sum((0, 1)), gy.sum((0, 1))
