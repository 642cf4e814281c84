"""numpy restatement of the ensemble kernels (csrc/ensemble.hip) and of dlwp_benchmark_amd/ensemble.py's host finish: the member
perturbation, the four pixel sums and the rank counts of dlwp_ens_diag, and the scores made of them.  float64 by default; `dtype=
np.float32` evaluates the same formulas in fp32 with the pixels added one after the other, which is what the GPU tests measure
their tolerance with."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_ref  # noqa: E402

TAG_ENS = 0x656E          # counter word 3 of dlwp_ens_perturb
MAX_MEMBERS = 64


def perturb(x, items, M, sigma, seed, P, control=True):
    """x [B, F] (any trailing shape, flattened per sample), sigma [V], planes of P elements -> [B, M, F] float64."""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    flat = x.reshape(B, -1)
    F = flat.shape[1]
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    sig = sigma[(np.arange(F) // P) % sigma.size]             # element e belongs to variable (e / P) % V
    out = np.empty((B, M, F))
    for b in range(B):
        for m in range(M):
            if m == 0 and control:
                out[b, m] = flat[b]                           # the control member: a copy, nothing drawn
            else:
                # the stream of the batch kernels with the MEMBER where they carry the epoch (counter word 2)
                out[b, m] = flat[b] + sig * batch_ref.normals(seed, m, int(items[b]), F, TAG_ENS)
    return out.reshape((B, M) + x.shape[1:])


def pair_loop(x):
    """sum_{i<j} |x_i - x_j| over axis 0, as the kernel adds it: i ascending, inside it j < i ascending."""
    s = np.zeros(x.shape[1:], dtype=x.dtype)
    for i in range(1, x.shape[0]):
        r = np.zeros(x.shape[1:], dtype=x.dtype)
        for j in range(i):
            r = r + np.abs(x[i] - x[j])
        s = s + r
    return s


def pair_sorted(x):
    """the same sum from the order statistics: sum_i sum_j |x_i - x_j| = 2 sum_k (2 k - M + 1) x_(k), halved."""
    M = x.shape[0]
    xs = np.sort(x, axis=0)
    k = (2 * np.arange(M) - M + 1).astype(x.dtype).reshape((M,) + (1,) * (x.ndim - 1))
    return (k * xs).sum(axis=0)


def pixel_terms(x, y, dtype=np.float64):
    """x [M, ...] members, y [...] target -> (the four per-pixel terms of `sums`, rank = #{i : x_i < y}), members in ascending order."""
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    M = x.shape[0]
    one = dtype(1)
    e = x - x[0]                                              # relative to member 0: exact for members close to each other
    se = np.zeros_like(y)
    sa = np.zeros_like(y)
    below = np.zeros(y.shape, dtype=np.int64)
    for i in range(M):
        se = se + e[i]
        sa = sa + np.abs(x[i] - y)
        below += x[i] < y                                     # a tie (x_i == y) is not below
    mu = se * (one / dtype(M))                                # the ensemble mean is x_0 + mu
    var = np.zeros_like(y)
    for i in range(M):                                        # second pass: no E[x^2] - mean^2
        d = e[i] - mu
        var = var + d * d
    inv_m, inv_m1 = one / dtype(M), one / dtype(M - 1)
    dm = (x[0] - y) + mu
    return (dm * dm, var * inv_m1, sa * inv_m, pair_loop(x) * (inv_m * inv_m1)), below


def diag(members, target, row_weights=None, dtype=np.float64):
    """members [B, M, T, V, H, W], target [B, T, V, H, W] -> sums [B, T, V, 4] (dtype), ranks [B, T, V, M + 1] (int64)."""
    members, target = np.asarray(members), np.asarray(target)
    B, M, T, V, H, W = members.shape
    w = np.ones(H, dtype=dtype) if row_weights is None else np.asarray(row_weights, dtype=dtype)
    terms, below = pixel_terms(np.moveaxis(members, 1, 0), target, dtype)
    sums = np.empty((B, T, V, 4), dtype=dtype)
    for c, t in enumerate(terms):
        weighted = (w[:, None] * t).reshape(B, T, V, H * W)
        sums[..., c] = np.cumsum(weighted, axis=-1, dtype=dtype)[..., -1]      # the pixels one after the other
    ranks = np.zeros((B, T, V, M + 1), dtype=np.int64)
    for k in range(M + 1):                                    # unweighted counts
        ranks[..., k] = (below == k).reshape(B, T, V, H * W).sum(axis=-1)
    return sums, ranks


def metrics(sums, ranks, M, H, W, scale=None):
    """The host finish of ensemble.ensemble_metrics: samples folded in index order, n = B H W, float64."""
    sums = np.asarray(sums, dtype=np.float64)
    B, T, V, _ = sums.shape
    tot, cnt = np.zeros((T, V, 4)), np.zeros((T, V, M + 1))
    for b in range(B):
        tot += sums[b]
        cnt += ranks[b]
    sc = np.ones(V) if scale is None else np.abs(np.asarray(scale, dtype=np.float64).reshape(V))
    n = float(B * H * W)
    rmse, spread = sc * np.sqrt(tot[..., 0] / n), sc * np.sqrt(tot[..., 1] / n)
    with np.errstate(divide="ignore", invalid="ignore"):
        ss = np.sqrt((M + 1) / M) * spread / rmse
    return {"rmse_mean": rmse, "spread": spread, "spread_skill": ss,
            "crps": sc * (tot[..., 2] - tot[..., 3]) / n,                          # the fair estimator
            "crps_ens": sc * (tot[..., 2] - (M - 1) / M * tot[..., 3]) / n,        # the M members taken as the whole distribution
            "mae_members": sc * tot[..., 2] / n, "rank_hist": cnt / n}


def fp32_floor(members, target, row_weights=None):
    """The largest relative difference between the fp32 and the float64 evaluation of `sums` on these inputs (entries that are
    exactly zero in float64 must be exactly zero in fp32), and the float64 tables."""
    s64, r64 = diag(members, target, row_weights, np.float64)
    s32, r32 = diag(members, target, row_weights, np.float32)
    assert (r32 == r64).all()                                 # fp32 inputs: every comparison is exact in both
    zero = s64 == 0
    assert (s32[zero] == 0).all()
    rel = np.abs(s32[~zero].astype(np.float64) - s64[~zero]) / np.abs(s64[~zero])
    return (float(rel.max()) if rel.size else 0.0), s64, r64
