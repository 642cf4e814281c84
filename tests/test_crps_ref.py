"""Anchors of tests/crps_ref.py, the restatement that defines dlwp_crps_loss_fwd_bwd: hand-computed values, the two estimators against
tests/ens_ref.py's metrics, the cancellation of the pair term's gradients, central differences and the tie rule."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crps_ref  # noqa: E402
import ens_ref  # noqa: E402


def one_pixel(x, y):
    """members x [M], target y -> [1, M, 1, 1, 1, 1] / [1, 1, 1, 1, 1]"""
    return np.asarray(x, dtype=np.float64).reshape(1, -1, 1, 1, 1, 1), np.asarray(y, dtype=np.float64).reshape(1, 1, 1, 1, 1)


def test_two_members_by_hand():
    m, t = one_pixel([1.0, 4.0], 2.0)
    # (|1 - 2| + |4 - 2|) / 2 - lambda |1 - 4| / 2
    assert crps_ref.loss(m, t, 1.0)[0] == 1.5 - 1.5 and crps_ref.loss(m, t, 0.5)[0] == 1.5 - 0.75
    assert crps_ref.loss(m, t, 1.0)[1] == 1.5
    # member 0 lies below y and below member 1: -1/2 - lambda (-1) / 2; member 1 above both: 1/2 - lambda / 2
    assert crps_ref.grad(m, t, 1.0).reshape(-1).tolist() == [0.0, 0.0]
    assert crps_ref.grad(m, t, 0.5).reshape(-1).tolist() == [-0.25, 0.25]
    assert crps_ref.grad(m, t, 0.0).reshape(-1).tolist() == [-0.5, 0.5]
    assert crps_ref.pair_coeff(1.0, 4) == 1.0 and crps_ref.pair_coeff(0.0, 4) == 0.75 and crps_ref.pair_coeff(0.5, 4) == 0.875


def test_equal_members_give_the_weighted_mae():
    rng = np.random.default_rng(1)
    B, M, T, V, H, W = 2, 5, 2, 3, 4, 6
    one = rng.standard_normal((B, 1, T, V, H, W))
    mem, tgt = np.repeat(one, M, axis=1), rng.standard_normal((B, T, V, H, W))
    r, c = rng.uniform(0.5, 1.5, H), rng.uniform(0.5, 1.5, V)
    w = r[None, None, None, :, None] * c[None, None, :, None, None]
    for lam in (1.0, 0.8):
        l, mae = crps_ref.loss(mem, tgt, lam, r, c)
        want = (w * np.abs(one[:, 0] - tgt)).mean()
        assert abs(l - want) <= 1e-14 and abs(mae - want) <= 1e-14
        g = crps_ref.grad(mem, tgt, lam, r, c)
        assert np.abs(g - np.repeat((w * np.sign(one[:, 0] - tgt) / (M * tgt.size))[:, None], M, axis=1)).max() <= 1e-17


def test_the_two_estimators_are_ens_ref_s():
    rng = np.random.default_rng(2)
    B, M, T, V, H, W = 3, 6, 2, 2, 5, 7
    mem, tgt = rng.standard_normal((B, M, T, V, H, W)), rng.standard_normal((B, T, V, H, W))
    r = rng.uniform(0.5, 1.5, H)
    sums, ranks = ens_ref.diag(mem, tgt, r)
    met = ens_ref.metrics(sums, ranks, M, H, W)
    for key, lam in (("crps", 1.0), ("crps_ens", (M - 1) / M)):
        assert abs(crps_ref.loss(mem, tgt, lam, r)[0] - met[key].mean()) <= 1e-14, key
    assert abs(crps_ref.loss(mem, tgt, 1.0, r)[1] - met["mae_members"].mean()) <= 1e-14
    # the count form of the pair term against the loop and the order statistics
    x = np.moveaxis(mem, 1, 0)
    pair = ((x - x[0]) * crps_ref.counts(x)).sum(axis=0)
    assert np.abs(pair - ens_ref.pair_loop(x)).max() <= 1e-12 and np.abs(pair - ens_ref.pair_sorted(x)).max() <= 1e-12


def test_the_pair_gradients_cancel():
    rng = np.random.default_rng(3)
    B, M, T, V, H, W = 2, 7, 1, 2, 3, 5
    mem, tgt = rng.standard_normal((B, M, T, V, H, W)), rng.standard_normal((B, T, V, H, W))
    for lam in (1.0, 6 / 7, 0.3):
        g = crps_ref.grad(mem, tgt, lam)
        want = np.sign(mem - tgt[:, None]).sum(axis=1) / (M * tgt.size)
        assert np.abs(g.sum(axis=1) - want).max() <= 1e-15


def lattice_case(rng, B, M, T, V, H, W):
    """distinct multiples of 1/8 per pixel, the target on the half steps between them: no kink within 1/16 of any value"""
    n = B * T * V * H * W
    mem = np.stack([rng.permutation(40)[:M] for _ in range(n)]).astype(np.float64) / 8 - 2.5
    tgt = (rng.integers(0, 40, n) + 0.5) / 8 - 2.5
    return np.moveaxis(mem.reshape(B, T, V, H, W, M), -1, 1).copy(), tgt.reshape(B, T, V, H, W)


def test_gradient_against_central_differences():
    rng = np.random.default_rng(4)
    shape = (2, 5, 1, 2, 3, 4)
    mem, tgt = lattice_case(rng, *shape)
    r, c = rng.uniform(0.5, 1.5, 3), rng.uniform(0.5, 1.5, 2)
    h = 1.0 / 32
    for lam in (1.0, 0.8, 0.0):
        g = crps_ref.grad(mem, tgt, lam, r, c)
        worst = 0.0
        for idx in np.ndindex(*shape):
            up, dn = mem.copy(), mem.copy()
            up[idx] += h
            dn[idx] -= h
            fd = (crps_ref.loss(up, tgt, lam, r, c)[0] - crps_ref.loss(dn, tgt, lam, r, c)[0]) / (2 * h)
            worst = max(worst, abs(fd - g[idx]))
        assert worst <= 1e-10, (lam, worst)


def test_tie_rule():
    # x_0 == x_1 and x_2 == y: the tied pair gives nothing to each other, the member on the target gets sgn(0) = 0
    m, t = one_pixel([1.0, 1.0, 3.0], 3.0)
    assert crps_ref.counts(m[0, :, 0, 0, 0, 0]).tolist() == [-1, -1, 2]
    l, mae = crps_ref.loss(m, t, 1.0)
    assert mae == 4.0 / 3 and abs(l - (4.0 / 3 - 4.0 / 6)) <= 1e-15
    g = crps_ref.grad(m, t, 1.0).reshape(-1)
    assert np.abs(g - np.array([-1 / 3 + 1 / 6, -1 / 3 + 1 / 6, 0.0 - 2 / 6])).max() <= 1e-16
    # all equal, on the target: the loss and every gradient are exactly 0
    m, t = one_pixel([2.0, 2.0, 2.0, 2.0], 2.0)
    assert crps_ref.loss(m, t, 1.0)[0] == 0.0 and not crps_ref.grad(m, t, 1.0).any()


def test_fp32_floor_and_bound_shapes():
    rng = np.random.default_rng(5)
    mem = rng.standard_normal((2, 4, 2, 3, 5, 7)).astype(np.float32)
    tgt = rng.standard_normal((2, 2, 3, 5, 7)).astype(np.float32)
    floor, l64, mae64 = crps_ref.fp32_floor(mem, tgt, 1.0)
    assert 0 < floor < 1e-5 and 0 < l64 < mae64
    r, c = np.linspace(0.5, 1.5, 5), np.array([1.0, 2.0, 0.5])
    b = crps_ref.grad_bound(mem.shape, r, c)
    assert b.shape == (1, 1, 1, 3, 5, 1) and b[0, 0, 0, 1, 2, 0] == 8 * 2.0 ** -24 * 2.0 / (mem.size)
    assert (np.abs(crps_ref.grad(mem, tgt, 1.0, r, c)) <= 2 * r[None, None, None, None, :, None] * c[None, None, None, :, None, None]
            / (tgt.size * 4) * (1 + 1e-12)).all()
