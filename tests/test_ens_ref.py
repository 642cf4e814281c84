"""Anchors of the float64 restatement tests/ens_ref.py (no GPU): hand-computed cases, the tie rule, the two forms of the pair term and
the known scores of a standard-normal ensemble against a standard-normal target."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_ref  # noqa: E402
import ens_ref  # noqa: E402


def one_pixel(x, y, w=None):
    """members x [M], target y -> (sums [4], ranks [M + 1]) of a 1 x 1 grid"""
    m = np.asarray(x, dtype=np.float64).reshape(1, len(x), 1, 1, 1, 1)
    s, r = ens_ref.diag(m, np.full((1, 1, 1, 1, 1), float(y)), None if w is None else [w])
    return s[0, 0, 0], r[0, 0, 0]


def test_two_members_by_hand():
    # x = (1, 4), y = 2: mean 2.5, (mean - y)^2 = 0.25; variance ((1.5)^2 + (1.5)^2) / 1 = 4.5; mean |x_i - y| = (1 + 2) / 2 = 1.5;
    # pair term |1 - 4| / (2 * 1) = 1.5; one member below y
    s, r = one_pixel([1.0, 4.0], 2.0)
    assert np.allclose(s, [0.25, 4.5, 1.5, 1.5], rtol=0, atol=1e-15)
    assert r.tolist() == [0, 1, 0]
    s, _ = one_pixel([1.0, 4.0], 2.0, w=0.5)                  # the row weight multiplies every sum, never the ranks
    assert np.allclose(s, [0.125, 2.25, 0.75, 0.75], rtol=0, atol=1e-15)
    m = ens_ref.metrics(s.reshape(1, 1, 1, 4) * 2, np.array([[[[0, 1, 0]]]]), 2, 1, 1, scale=[-3.0])
    assert np.isclose(m["rmse_mean"][0, 0], 3 * 0.5) and np.isclose(m["spread"][0, 0], 3 * np.sqrt(4.5))
    assert np.isclose(m["spread_skill"][0, 0], np.sqrt(1.5) * np.sqrt(4.5) / 0.5)
    assert np.isclose(m["crps"][0, 0], 0.0) and np.isclose(m["crps_ens"][0, 0], 3 * 0.75) and np.isclose(m["mae_members"][0, 0], 4.5)
    assert m["rank_hist"][0, 0].tolist() == [0, 1, 0]


def test_all_members_equal():
    rng = np.random.default_rng(5)
    x0, y = rng.standard_normal((2, 3, 2, 4, 6)), rng.standard_normal((2, 3, 2, 4, 6))
    M = 5
    mem = np.repeat(x0[:, None], M, axis=1)
    s, r = ens_ref.diag(mem, y)
    assert (s[..., 1] == 0).all() and (s[..., 3] == 0).all()
    assert (r[..., 1:M] == 0).all() and (r[..., 0] + r[..., M] == 24).all()
    m = ens_ref.metrics(s, r, M, 4, 6)
    assert (m["spread"] == 0).all() and np.array_equal(m["crps"], m["mae_members"])
    assert np.allclose(m["rmse_mean"], np.sqrt(((x0 - y) ** 2).mean(axis=(0, 3, 4))))


def test_a_tie_is_not_below():
    _, r = one_pixel([0.0, 1.0, 2.0], 1.0)                    # x_1 == y: only x_0 is below
    assert r.tolist() == [0, 1, 0, 0]
    _, r = one_pixel([1.0, 1.0, 1.0], 1.0)                    # all tied: bin 0
    assert r.tolist() == [1, 0, 0, 0]
    _, r = one_pixel([0.0, 0.5, 0.75], 1.0)                   # all below: bin M
    assert r.tolist() == [0, 0, 0, 1]


def test_pair_loop_equals_the_sorted_form():
    rng = np.random.default_rng(6)
    for M in (2, 3, 5, 16, 64):
        x = rng.standard_normal((M, 50))
        a, b = ens_ref.pair_loop(x), ens_ref.pair_sorted(x)
        brute = np.abs(x[:, None] - x[None]).sum(axis=(0, 1)) / 2
        assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max(), M
        assert np.abs(a - brute).max() <= 1e-13 * np.abs(a).max(), M


def test_two_pass_variance_survives_cancellation():
    """members 3 + 1e-3 z in fp32: the restatement's fp32 evaluation stays at rounding level, E[x^2] - mean^2 does not."""
    rng = np.random.default_rng(7)
    mem = (3 + 1e-3 * rng.standard_normal((1, 8, 1, 1, 5, 7))).astype(np.float32)
    y = (3 + 1e-3 * rng.standard_normal((1, 1, 1, 5, 7))).astype(np.float32)
    floor, s64, _ = ens_ref.fp32_floor(mem, y)
    print(f"fp32 floor on 3 + 1e-3 z: {floor:.2e}")
    assert floor < 1e-5
    x = mem[0, :, 0, 0].astype(np.float32)
    naive = ((x * x).mean(axis=0, dtype=np.float32) - x.mean(axis=0, dtype=np.float32) ** 2) * np.float32(8 / 7)
    exact = x.astype(np.float64).var(axis=0, ddof=1)
    assert np.isclose(exact.sum(), s64[0, 0, 0, 1], rtol=1e-12)
    assert (np.abs(naive - exact) / exact).max() > 1e-2       # one ulp of x^2 = 9 is the size of the variance itself


def test_standard_normal_ensemble():
    rng = np.random.default_rng(1234)
    M, N = 8, 65536
    x, y = rng.standard_normal((M, N)), rng.standard_normal(N)
    (t0, t1, t2, t3), below = ens_ref.pixel_terms(x, y)
    fair = t2 - t3
    se = fair.std(ddof=1) / np.sqrt(N)
    exact = 1 / np.sqrt(np.pi)                                # the CRPS of N(0, 1) forecasts of N(0, 1) truth, averaged
    s, r = ens_ref.diag(x.reshape(1, M, 1, 1, 256, 256), y.reshape(1, 1, 1, 256, 256))
    m = ens_ref.metrics(s, r, M, 256, 256)
    crps, crps_ens, ss = m["crps"][0, 0], m["crps_ens"][0, 0], m["spread_skill"][0, 0]
    hist = r[0, 0, 0]
    chi2 = float(((hist - N / (M + 1)) ** 2 / (N / (M + 1))).sum())
    print(f"fair CRPS {crps:.4f} (se {se:.4f}, exact {exact:.4f}), crps_ens {crps_ens:.4f}, spread_skill {ss:.4f}, chi2 {chi2:.2f}")
    assert np.isclose(crps, fair.mean(), rtol=1e-12)
    assert abs(crps - exact) <= 5 * se
    assert abs(crps_ens - exact) > 5 * se                     # the biased estimator must not pass for the fair one
    assert abs(ss - 1) <= 0.02
    assert hist.sum() == N and chi2 < 26.1                    # 99.9th percentile of chi^2 with 8 degrees of freedom


def test_perturbation_stream():
    """the member sits in counter word 2; the control member is the input; sigma follows (e / P) % V"""
    x = np.arange(2 * 2 * 3 * 5, dtype=np.float64).reshape(2, 2, 3, 5)          # [B, L, V, P]
    sig = [0.5, 0.0, 2.0]
    out = ens_ref.perturb(x, [3, 7], 3, sig, 99, P=5)
    assert out.shape == (2, 3, 2, 3, 5) and np.array_equal(out[:, 0], x)
    z = batch_ref.normals(99, 2, 7, 30, ens_ref.TAG_ENS).reshape(2, 3, 5)
    assert np.allclose(out[1, 2] - x[1], np.array(sig)[None, :, None] * z)
    assert np.array_equal(out[:, :, :, 1], np.repeat(x[:, None, :, 1], 3, axis=1))   # sigma 0: untouched
    free = ens_ref.perturb(x, [3, 7], 3, sig, 99, P=5, control=False)
    assert np.array_equal(free[:, 1:], out[:, 1:]) and not np.array_equal(free[:, 0], x)
