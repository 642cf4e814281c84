"""dlwp_crps_loss_fwd_bwd through dlwp_benchmark_amd/ensemble.py (crps_loss, crps_loss_and_grad) against the float64 restatement
tests/crps_ref.py.

Value.  Members and target are standard normal, so the loss is about half of its weighted-MAE term and never near zero; the error
is measured relative to that term.  The tolerance is measured per case, on the CPU, before the kernel's number is looked at: the
floor is the restatement evaluated in np.float32 (pixels added one after the other) against itself in float64 on the case's inputs
(crps_ref.fp32_floor), the tolerance 4 x the floor (another summation order, FMA contraction), capped at 1e-4 -- the rule of
tests/test_gpu_ensemble.py.
Gradient.  Inputs are fp32, so every comparison is exact in both precisions and the bracket sgn(x_i - y) / M - lambda c_i / (M (M - 1))
is made of the same two integers on both sides: |g - g64| <= 8 x 2^-24 r_h c_v / (N M) for EVERY element (four roundings on terms of
magnitude at most 1 / M, doubled).  lambda is the float the C ABI carries; the weights are the fp32 values the kernel reads.
Shapes: 5 x 7, 1 x 9, 8 x 16 (one pixel block, a partly filled wave), 20 x 23 (two blocks) and 130 x 127 (two pixels per thread, 33
blocks); member counts on both sides of every bucket edge (8 | 9, 16 | 17, 32 | 33) and 2, 3, 64."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crps_ref  # noqa: E402
import ens_ref  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 1e-4
ALPHAS = (1.0, 0.95, 0.0)
VAR_W = np.array([1.0, 0.5, 2.0], dtype=np.float32)


def make_case(B, M, T, V, H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, M, T, V, H, W)).astype(np.float32), rng.standard_normal((B, T, V, H, W)).astype(np.float32)


def tie_case(B, M, T, V, H, W, seed):
    """multiples of 0.25 in [-1, 1]: nine values, so x_i == x_j and x_i == y occur in nearly every pixel"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-4, 5, (B, M, T, V, H, W)) * 0.25).astype(np.float32), (rng.integers(-4, 5, (B, T, V, H, W)) * 0.25).astype(np.float32)


def weights(H):
    from dlwp_benchmark_amd import evaluate
    lats = evaluate.regular_latitudes(H)
    return lats, evaluate.lat_weights(lats).numpy()           # the fp32 weights the kernel reads


def lam_of(alpha, M):
    return float(np.float32(crps_ref.pair_coeff(alpha, M)))   # the C ABI carries lambda as a float


def check(cuda, mem, tgt, alpha, lats=None, roww=None, varw=None, what=""):
    from dlwp_benchmark_amd import ensemble as E
    lam = lam_of(alpha, mem.shape[1])
    floor, l64, mae64 = crps_ref.fp32_floor(mem, tgt, lam, roww, varw)      # before the kernel's number is looked at
    tol = min(4 * floor, CAP)
    g64 = crps_ref.grad(mem, tgt, lam, roww, varw)
    bound = crps_ref.grad_bound(mem.shape, roww, varw)
    assert l64 > 0.25 * mae64, (what, l64, mae64)                          # never near zero
    loss, g = E.crps_loss_and_grad(torch.from_numpy(mem).to(cuda), torch.from_numpy(tgt).to(cuda), alpha=alpha, lats_deg=lats,
                                   var_weights=varw)
    assert loss.dim() == 0 and tuple(g.shape) == mem.shape and g.dtype == torch.float32
    err = abs(float(loss.double().item()) - l64) / mae64
    ratio = float((np.abs(g.double().cpu().numpy() - g64) / bound).max())
    print(f"{what} alpha {alpha}: fp32 floor {floor:.2e}, tolerance {tol:.2e}, kernel {err:.2e}; gradient error / bound {ratio:.3f}")
    assert err <= tol, (what, alpha, err, tol)
    assert ratio <= 1.0, (what, alpha, ratio)                              # every element
    return loss, g


@pytest.mark.parametrize("M", [2, 3, 8, 9, 16, 17, 33, 64])
@pytest.mark.parametrize("H,W", [(5, 7), (1, 9), (8, 16)])
def test_loss_and_gradient_match_the_restatement(cuda, M, H, W):
    mem, tgt = make_case(2, M, 2, 3, H, W, seed=300 + M)
    lats, roww = weights(H)
    for k, alpha in enumerate(ALPHAS):
        if k % 2 == 0:
            check(cuda, mem, tgt, alpha, what=f"M {M} {H}x{W}")
            check(cuda, mem, tgt, alpha, lats, roww, VAR_W, what=f"M {M} {H}x{W} weighted")
        else:
            check(cuda, mem, tgt, alpha, lats, roww, None, what=f"M {M} {H}x{W} rows")
            check(cuda, mem, tgt, alpha, None, None, VAR_W, what=f"M {M} {H}x{W} variables")


@pytest.mark.parametrize("M,H,W", [(3, 20, 23), (16, 20, 23), (3, 130, 127), (16, 130, 127)])
def test_several_pixel_blocks(cuda, M, H, W):
    mem, tgt = make_case(2, M, 2, 3, H, W, seed=400 + M)
    lats, roww = weights(H)
    check(cuda, mem, tgt, 1.0, what=f"M {M} {H}x{W}")
    check(cuda, mem, tgt, 0.95, lats, roww, VAR_W, what=f"M {M} {H}x{W} weighted")
    check(cuda, mem, tgt, 0.0, lats, roww, VAR_W, what=f"M {M} {H}x{W} weighted")


@pytest.mark.parametrize("M", [2, 5, 9, 33])
def test_ties(cuda, M):
    mem, tgt = tie_case(2, M, 2, 3, 8, 16, seed=500 + M)
    x = np.moveaxis(mem, 1, 0)
    assert (x[0] == x[1]).any() and (x[0] == tgt).any()
    lats, roww = weights(8)
    for alpha in ALPHAS:
        check(cuda, mem, tgt, alpha, lats, roww, VAR_W, what=f"ties M {M}")
    same = np.repeat(mem[:, :1], M, axis=1)                              # all members equal: the weighted MAE, the pair term exactly 0
    loss, g = check(cuda, same, tgt, 1.0, what=f"equal members M {M}")
    assert torch.equal(g, g[:, :1].expand_as(g))


def test_two_calls_give_the_same_bits(cuda):
    from dlwp_benchmark_amd import ensemble as E
    mem, tgt = make_case(2, 9, 2, 3, 130, 127, seed=21)
    lats, _ = weights(130)
    m, t = torch.from_numpy(mem).to(cuda), torch.from_numpy(tgt).to(cuda)
    a = E.crps_loss_and_grad(m, t, alpha=0.95, lats_deg=lats, var_weights=VAR_W)
    b = E.crps_loss_and_grad(m, t, alpha=0.95, lats_deg=lats, var_weights=VAR_W)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    out = torch.full((1,), 7.0, device=cuda)
    c = E.crps_loss_and_grad(m, t, out, alpha=0.95, lats_deg=lats, var_weights=VAR_W)      # loss_out is written, not accumulated
    assert torch.equal(out[0], a[0]) and c[0].data_ptr() == out.data_ptr()
    with torch.no_grad():
        assert torch.equal(E.crps_loss(m, t, alpha=0.95, lats_deg=lats, var_weights=VAR_W), a[0])      # the forward-only kernel


def test_forced_bucket(cuda):
    from dlwp_benchmark_amd import ensemble as E, lib as L
    mem, tgt = make_case(2, 5, 2, 3, 8, 16, seed=7)
    m, t = torch.from_numpy(mem).to(cuda), torch.from_numpy(tgt).to(cuda)
    auto = E.crps_loss_and_grad(m, t, alpha=0.95)
    for bucket in (16, 32, 64):
        L.set_tuning("ENS_BUCKET", bucket)
        try:
            forced = E.crps_loss_and_grad(m, t, alpha=0.95)
        finally:
            L.set_tuning("ENS_BUCKET", None)
        assert torch.equal(forced[0], auto[0]) and torch.equal(forced[1], auto[1]), bucket


def test_strided_members_are_read_in_place(cuda):
    from dlwp_benchmark_amd import ensemble as E
    rng = np.random.default_rng(23)
    store = torch.from_numpy(rng.standard_normal((5, 2, 6, 3, 5, 7)).astype(np.float32)).to(cuda)      # [M, B, T', V, H, W]
    view = store.permute(1, 0, 2, 3, 4, 5)[:, :, 1:5]                    # [B, M, T, V, H, W]: member before batch, a time slice
    assert not view.is_contiguous() and view.stride(0) < view.stride(1)
    tgt = torch.from_numpy(rng.standard_normal((2, 4, 3, 5, 7)).astype(np.float32)).to(cuda)
    lats, _ = weights(5)
    a = E.crps_loss_and_grad(view, tgt, lats_deg=lats)
    b = E.crps_loss_and_grad(view.contiguous(), tgt, lats_deg=lats)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].is_contiguous()
    lats, roww = weights(5)
    check(cuda, view.contiguous().cpu().numpy(), tgt.cpu().numpy(), 1.0, lats, roww, None, what="strided")


def test_fair_crps_equals_the_diagnostics_kernel(cuda):
    from dlwp_benchmark_amd import ensemble as E
    mem, tgt = make_case(2, 9, 2, 3, 20, 23, seed=29)
    lats, roww = weights(20)
    floor, l64, mae64 = crps_ref.fp32_floor(mem, tgt, 1.0, roww)
    efloor, _, _ = ens_ref.fp32_floor(mem, tgt, roww)                    # the other kernel's own floor, on its sums
    m, t = torch.from_numpy(mem).to(cuda), torch.from_numpy(tgt).to(cuda)
    loss = E.crps_loss(m, t, alpha=1.0, lats_deg=lats)
    met = E.ensemble_metrics(E.ensemble_diagnostics(m, t, lats_deg=lats))
    want = float(met["crps"].mean())
    tol = min(4 * floor, CAP) + min(4 * efloor, CAP)                     # each side within its own tolerance of float64
    err = abs(float(loss.double().item()) - want) / mae64
    print(f"crps_loss {float(loss):.7f}, diagnostics {want:.7f}: {err:.2e} of the MAE term, tolerance {tol:.2e}")
    assert err <= tol


def test_hpx_planes(cuda):
    from dlwp_benchmark_amd import ensemble as E
    rng = np.random.default_rng(31)
    mem = rng.standard_normal((2, 3, 2, 2, 12, 2, 2)).astype(np.float32)
    tgt = rng.standard_normal((2, 2, 2, 12, 2, 2)).astype(np.float32)
    flat_m, flat_t = mem.reshape(2, 3, 2, 2, 24, 2), tgt.reshape(2, 2, 2, 24, 2)
    vw = np.array([1.0, 0.5], dtype=np.float32)
    floor, l64, mae64 = crps_ref.fp32_floor(flat_m, flat_t, 1.0, None, vw)
    loss, g = E.crps_loss_and_grad(torch.from_numpy(mem).to(cuda), torch.from_numpy(tgt).to(cuda), var_weights=vw)
    assert tuple(g.shape) == mem.shape
    assert abs(float(loss.double().item()) - l64) / mae64 <= min(4 * floor, CAP)
    g64 = crps_ref.grad(flat_m, flat_t, 1.0, None, vw).reshape(mem.shape)
    bound = np.broadcast_to(crps_ref.grad_bound(flat_m.shape, None, vw), flat_m.shape).reshape(mem.shape)
    assert (np.abs(g.double().cpu().numpy() - g64) <= bound).all()
    with pytest.raises(ValueError, match="equal area"):
        E.crps_loss(torch.from_numpy(mem).to(cuda), torch.from_numpy(tgt).to(cuda), lats_deg=np.zeros(24))


def test_autograd_route(cuda):
    from dlwp_benchmark_amd import ensemble as E
    mem, tgt = make_case(2, 5, 2, 3, 8, 16, seed=37)
    lats, _ = weights(8)
    m, t = torch.from_numpy(mem).to(cuda).requires_grad_(True), torch.from_numpy(tgt).to(cuda)
    want_loss, want = E.crps_loss_and_grad(m, t, alpha=0.95, lats_deg=lats, var_weights=VAR_W)
    loss = E.crps_loss(m, t, alpha=0.95, lats_deg=lats, var_weights=VAR_W)
    assert loss.dim() == 0 and torch.equal(loss.detach(), want_loss)
    loss.backward()
    assert torch.equal(m.grad, want)
    m.grad = None
    (3.0 * E.crps_loss(m, t, alpha=0.95, lats_deg=lats, var_weights=VAR_W)).backward()       # grad x upstream
    assert torch.equal(m.grad, want * 3.0)


def test_device_items_are_read_in_place(cuda):
    from dlwp_benchmark_amd import ensemble as E
    x = torch.randn(3, 2, 3, 5, 7, generator=torch.Generator().manual_seed(5)).to(cuda)
    items = torch.tensor([4, 0, 9], dtype=torch.int32, device=cuda)
    a = E.perturb_members(x, [4, 0, 9], 4, [0.5, 0.0, 2.0], 1234, control=False)
    b = E.perturb_members(x, items, 4, [0.5, 0.0, 2.0], 1234, control=False, validate_items=False)
    assert torch.equal(a, b)
