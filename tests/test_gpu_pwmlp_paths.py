"""Every kernel path of the pointwise two-layer MLP (FNO lifting / projection) against a float64 reference, with the
instantiation each case must reach pinned through lib.kernel_accounting.

The scalar-output backward (Cout == 1: pwmlp_bwd_kernel<NIB, 0, 8>) forms g_a = gy[p] * w2[h] on the VALU instead of
multiplying 15 rows of zeros on the matrix pipe, and every backward transposes gz through LDS instead of an identity
product; both are exact, so every deterministic output is bit for bit the previous build's.  The forward kernels and dW2
stay on the MFMA (VALU forms reorder fp32 sums and moved the training step's outputs).  The controls (Cout in {2, 16, 32})
must still launch the generic instantiations.

Error bars.  Every figure is a max-norm relative error against the float64 reference below.  The bar of an output is TWICE
the error the previous (all-MFMA) build made on the same seeded inputs, measured on MI355X and recorded in PARENT_ERR next
to the case (a dropped term or a wrong row shows as 1e-2 or worse), and never more than the 1e-4 forward / 5e-4 gradient
bars of tests/test_gpu_fno.py.  y, gx and everything in slab mode are deterministic: one measurement is the previous
build's error.  The weight gradients of the float-atomic epilogue (gw1, gb1, gw2, gb2 of dlwp_pwmlp_bwd) depend on the
order in which the workgroups' atomics arrive and vary run to run on one and the same build (the previous build's own runs
of one output span a factor of 2 to 300, unchanged per-workgroup partials included), so its error for those is the largest
of 52 runs.  Each test prints its figures before it asserts; PWMLP_PATHS_REPORT=<file> appends them as JSON lines.
"""
import itertools
import json
import os

import pytest
import torch

from oracle import fno_ref

FWD_TOL = 1e-4
GRAD_TOL = 5e-4
SENTINEL = 12345.0

SCALAR_CASES = [(B, Cin, Ch, 1, P) for Cin, Ch, P, B in itertools.product((32, 10, 3), (256, 40), (4096, 100), (1, 4))]
CONTROL_CASES = [(4, 32, 256, 2, 4096), (1, 10, 40, 2, 100), (4, 32, 256, 16, 4096), (1, 3, 40, 16, 100),
                 (4, 10, 256, 32, 4096), (1, 32, 40, 32, 100)]


def case_id(c):
    return "B%d-Cin%d-Ch%d-Cout%d-P%d" % c


# max-norm relative error of the previous build (every product on the MFMA) against the float64 reference, MI355X, the seeded
# inputs of make_case(), rounded up to three digits; keys: y (dlwp_pwmlp_fwd), gx .. gb2 (dlwp_pwmlp_bwd, float atomics), s_gx .. s_gb2 (two accumulating
# dlwp_pwmlp_bwd_slab calls + dlwp_pwmlp_slab_fold)
PARENT_ERR = {
    "B1-Cin32-Ch256-Cout1-P4096": {"y": 2.76e-07, "gx": 1.72e-07, "gw1": 4.00e-07, "gb1": 6.01e-07, "gw2": 4.42e-07, "gb2": 1.67e-06, "s_gx": 2.23e-07, "s_gw1": 2.62e-07, "s_gb1": 7.78e-08, "s_gw2": 1.76e-07, "s_gb2": 9.49e-08},
    "B4-Cin32-Ch256-Cout1-P4096": {"y": 2.93e-07, "gx": 1.91e-07, "gw1": 9.03e-07, "gb1": 8.05e-07, "gw2": 5.71e-07, "gb2": 1.32e-06, "s_gx": 2.31e-07, "s_gw1": 2.43e-07, "s_gb1": 1.90e-07, "s_gw2": 2.36e-07, "s_gb2": 7.96e-07},
    "B1-Cin32-Ch256-Cout1-P100": {"y": 2.18e-07, "gx": 1.69e-07, "gw1": 2.34e-07, "gb1": 2.31e-07, "gw2": 2.08e-07, "gb2": 8.58e-08, "s_gx": 1.31e-07, "s_gw1": 2.63e-07, "s_gb1": 2.98e-07, "s_gw2": 1.72e-07, "s_gb2": 1.49e-07},
    "B4-Cin32-Ch256-Cout1-P100": {"y": 1.91e-07, "gx": 1.80e-07, "gw1": 1.70e-07, "gb1": 2.11e-07, "gw2": 1.98e-07, "gb2": 1.01e-07, "s_gx": 1.84e-07, "s_gw1": 1.66e-07, "s_gb1": 1.17e-07, "s_gw2": 2.64e-07, "s_gb2": 1.74e-07},
    "B1-Cin32-Ch40-Cout1-P4096": {"y": 2.52e-07, "gx": 1.97e-07, "gw1": 2.75e-07, "gb1": 3.40e-07, "gw2": 3.69e-07, "gb2": 4.72e-07, "s_gx": 1.93e-07, "s_gw1": 1.56e-07, "s_gb1": 2.32e-07, "s_gw2": 2.09e-07, "s_gb2": 2.43e-07},
    "B4-Cin32-Ch40-Cout1-P4096": {"y": 2.26e-07, "gx": 1.55e-07, "gw1": 7.48e-07, "gb1": 1.05e-06, "gw2": 9.96e-07, "gb2": 3.26e-05, "s_gx": 1.57e-07, "s_gw1": 2.44e-07, "s_gb1": 2.65e-07, "s_gw2": 2.62e-07, "s_gb2": 3.36e-07},
    "B1-Cin32-Ch40-Cout1-P100": {"y": 1.58e-07, "gx": 1.57e-07, "gw1": 1.91e-07, "gb1": 1.93e-07, "gw2": 1.51e-07, "gb2": 4.33e-08, "s_gx": 2.00e-07, "s_gw1": 1.52e-07, "s_gb1": 2.22e-07, "s_gw2": 1.87e-07, "s_gb2": 1.55e-07},
    "B4-Cin32-Ch40-Cout1-P100": {"y": 1.95e-07, "gx": 1.13e-07, "gw1": 1.99e-07, "gb1": 2.14e-07, "gw2": 4.00e-07, "gb2": 1.30e-07, "s_gx": 1.26e-07, "s_gw1": 2.19e-07, "s_gb1": 2.40e-07, "s_gw2": 1.66e-07, "s_gb2": 1.36e-06},
    "B1-Cin10-Ch256-Cout1-P4096": {"y": 1.88e-07, "gx": 1.45e-07, "gw1": 3.23e-07, "gb1": 5.07e-07, "gw2": 5.13e-07, "gb2": 1.29e-06, "s_gx": 1.62e-07, "s_gw1": 2.02e-07, "s_gb1": 3.89e-07, "s_gw2": 2.22e-07, "s_gb2": 7.46e-07},
    "B4-Cin10-Ch256-Cout1-P4096": {"y": 2.61e-07, "gx": 2.00e-07, "gw1": 8.40e-07, "gb1": 8.74e-07, "gw2": 1.12e-06, "gb2": 1.09e-06, "s_gx": 2.78e-07, "s_gw1": 2.28e-07, "s_gb1": 2.11e-07, "s_gw2": 2.18e-07, "s_gb2": 9.49e-08},
    "B1-Cin10-Ch256-Cout1-P100": {"y": 2.20e-07, "gx": 2.40e-07, "gw1": 3.51e-07, "gb1": 1.85e-07, "gw2": 2.00e-07, "gb2": 1.95e-07, "s_gx": 1.42e-07, "s_gw1": 3.34e-07, "s_gb1": 1.78e-07, "s_gw2": 1.41e-07, "s_gb2": 2.27e-07},
    "B4-Cin10-Ch256-Cout1-P100": {"y": 2.29e-07, "gx": 1.36e-07, "gw1": 2.19e-07, "gb1": 1.90e-07, "gw2": 2.85e-07, "gb2": 2.12e-07, "s_gx": 1.22e-07, "s_gw1": 2.46e-07, "s_gb1": 1.93e-07, "s_gw2": 1.65e-07, "s_gb2": 2.45e-07},
    "B1-Cin10-Ch40-Cout1-P4096": {"y": 2.14e-07, "gx": 1.10e-07, "gw1": 3.64e-07, "gb1": 4.30e-07, "gw2": 5.02e-07, "gb2": 1.50e-06, "s_gx": 1.33e-07, "s_gw1": 1.34e-07, "s_gb1": 1.87e-07, "s_gw2": 2.94e-07, "s_gb2": 3.67e-07},
    "B4-Cin10-Ch40-Cout1-P4096": {"y": 2.81e-07, "gx": 2.36e-07, "gw1": 1.07e-06, "gb1": 8.48e-07, "gw2": 7.46e-07, "gb2": 1.85e-06, "s_gx": 2.16e-07, "s_gw1": 2.98e-07, "s_gb1": 2.77e-07, "s_gw2": 3.21e-07, "s_gb2": 1.35e-06},
    "B1-Cin10-Ch40-Cout1-P100": {"y": 1.71e-07, "gx": 2.05e-07, "gw1": 1.34e-07, "gb1": 1.21e-07, "gw2": 2.02e-07, "gb2": 1.99e-07, "s_gx": 1.59e-07, "s_gw1": 2.64e-07, "s_gb1": 9.88e-08, "s_gw2": 2.73e-07, "s_gb2": 3.67e-08},
    "B4-Cin10-Ch40-Cout1-P100": {"y": 1.37e-07, "gx": 1.75e-07, "gw1": 2.22e-07, "gb1": 1.39e-07, "gw2": 2.01e-07, "gb2": 1.28e-07, "s_gx": 1.34e-07, "s_gw1": 1.94e-07, "s_gb1": 1.37e-07, "s_gw2": 1.17e-07, "s_gb2": 1.08e-07},
    "B1-Cin3-Ch256-Cout1-P4096": {"y": 2.02e-07, "gx": 1.85e-07, "gw1": 4.21e-07, "gb1": 3.38e-07, "gw2": 4.36e-07, "gb2": 3.95e-07, "s_gx": 1.68e-07, "s_gw1": 1.20e-07, "s_gb1": 1.12e-07, "s_gw2": 2.04e-07, "s_gb2": 3.41e-08},
    "B4-Cin3-Ch256-Cout1-P4096": {"y": 4.70e-07, "gx": 2.72e-07, "gw1": 7.75e-07, "gb1": 6.36e-07, "gw2": 8.54e-07, "gb2": 1.02e-06, "s_gx": 2.65e-07, "s_gw1": 3.67e-07, "s_gb1": 2.26e-07, "s_gw2": 3.43e-07, "s_gb2": 1.37e-08},
    "B1-Cin3-Ch256-Cout1-P100": {"y": 2.61e-07, "gx": 1.82e-07, "gw1": 1.34e-07, "gb1": 2.33e-07, "gw2": 2.62e-07, "gb2": 1.06e-06, "s_gx": 2.75e-07, "s_gw1": 1.90e-07, "s_gb1": 9.62e-08, "s_gw2": 1.48e-07, "s_gb2": 9.58e-08},
    "B4-Cin3-Ch256-Cout1-P100": {"y": 2.11e-07, "gx": 1.83e-07, "gw1": 1.87e-07, "gb1": 2.28e-07, "gw2": 2.04e-07, "gb2": 1.42e-07, "s_gx": 1.30e-07, "s_gw1": 3.32e-07, "s_gb1": 3.25e-07, "s_gw2": 4.03e-07, "s_gb2": 4.68e-07},
    "B1-Cin3-Ch40-Cout1-P4096": {"y": 3.62e-07, "gx": 2.25e-07, "gw1": 4.26e-07, "gb1": 4.24e-07, "gw2": 3.22e-07, "gb2": 5.19e-07, "s_gx": 2.37e-07, "s_gw1": 2.34e-07, "s_gb1": 2.37e-07, "s_gw2": 1.97e-07, "s_gb2": 1.85e-07},
    "B4-Cin3-Ch40-Cout1-P4096": {"y": 1.26e-07, "gx": 1.53e-07, "gw1": 6.57e-07, "gb1": 7.99e-07, "gw2": 7.45e-07, "gb2": 4.36e-07, "s_gx": 1.52e-07, "s_gw1": 3.61e-07, "s_gb1": 1.46e-07, "s_gw2": 1.78e-07, "s_gb2": 7.21e-08},
    "B1-Cin3-Ch40-Cout1-P100": {"y": 5.90e-08, "gx": 8.87e-08, "gw1": 2.64e-07, "gb1": 8.54e-08, "gw2": 1.09e-07, "gb2": 9.01e-08, "s_gx": 1.58e-07, "s_gw1": 2.29e-07, "s_gb1": 4.09e-07, "s_gw2": 2.83e-07, "s_gb2": 3.81e-07},
    "B4-Cin3-Ch40-Cout1-P100": {"y": 1.26e-07, "gx": 2.38e-07, "gw1": 4.37e-07, "gb1": 4.63e-07, "gw2": 3.88e-07, "gb2": 7.76e-07, "s_gx": 2.15e-07, "s_gw1": 2.40e-07, "s_gb1": 1.82e-07, "s_gw2": 2.25e-07, "s_gb2": 2.47e-07},
    "B4-Cin32-Ch256-Cout2-P4096": {"y": 3.12e-07, "gx": 1.73e-07, "gw1": 6.42e-07, "gb1": 4.42e-07, "gw2": 9.88e-07, "gb2": 9.05e-07, "s_gx": 2.35e-07, "s_gw1": 2.31e-07, "s_gb1": 2.86e-07, "s_gw2": 4.13e-07, "s_gb2": 5.08e-08},
    "B1-Cin10-Ch40-Cout2-P100": {"y": 1.46e-07, "gx": 1.62e-07, "gw1": 1.86e-07, "gb1": 8.05e-08, "gw2": 2.26e-07, "gb2": 9.22e-08, "s_gx": 1.50e-07, "s_gw1": 1.29e-07, "s_gb1": 1.08e-07, "s_gw2": 1.57e-07, "s_gb2": 1.09e-07},
    "B4-Cin32-Ch256-Cout16-P4096": {"y": 2.40e-07, "gx": 1.96e-07, "gw1": 8.21e-07, "gb1": 7.84e-07, "gw2": 6.22e-07, "gb2": 6.06e-07, "s_gx": 2.19e-07, "s_gw1": 2.97e-07, "s_gb1": 2.51e-07, "s_gw2": 2.81e-07, "s_gb2": 2.72e-07},
    "B1-Cin3-Ch40-Cout16-P100": {"y": 1.69e-07, "gx": 1.46e-07, "gw1": 2.15e-07, "gb1": 1.79e-07, "gw2": 2.26e-07, "gb2": 2.40e-07, "s_gx": 1.81e-07, "s_gw1": 1.96e-07, "s_gb1": 1.97e-07, "s_gw2": 2.09e-07, "s_gb2": 2.70e-07},
    "B4-Cin10-Ch256-Cout32-P4096": {"y": 2.50e-07, "gx": 2.28e-07, "gw1": 6.93e-07, "gb1": 8.77e-07, "gw2": 7.20e-07, "gb2": 8.00e-07, "s_gx": 2.56e-07, "s_gw1": 2.56e-07, "s_gb1": 2.46e-07, "s_gw2": 2.50e-07, "s_gb2": 2.15e-07},
    "B1-Cin32-Ch40-Cout32-P100": {"y": 1.58e-07, "gx": 2.18e-07, "gw1": 1.43e-07, "gb1": 8.49e-08, "gw2": 2.51e-07, "gb2": 2.36e-07, "s_gx": 1.82e-07, "s_gw1": 1.36e-07, "s_gb1": 1.90e-07, "s_gw2": 2.12e-07, "s_gb2": 1.71e-07},
}
# the chained forward (projection of net call k + lifting of call k + 1) through the rollout trainer: error of the prediction
PARENT_ERR_ROLLOUT = {
    "D1": {"yhat": 1.57e-08, "last": 7.41e-07},
    "D2": {"yhat": 1.18e-08, "last": 5.10e-07},
}


def bar(table, key, name, tol):
    """twice the previous build's error, inside the suite's tolerance"""
    return min(2.0 * table[key][name], tol)


def report(kind, key, figures, kernels):
    line = {"kind": kind, "case": key, "err": figures, "kernels": kernels}
    print(json.dumps(line))
    path = os.environ.get("PWMLP_PATHS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def make_case(B, Cin, Ch, Cout, P):
    g = torch.Generator().manual_seed(4321 + 7 * Cin + Ch + 13 * Cout + P + B)
    x = torch.randn(B, Cin, P, generator=g)
    w1 = torch.randn(Ch, Cin, generator=g) / Cin ** 0.5
    b1 = torch.randn(Ch, generator=g) * 0.1
    w2 = torch.randn(Cout, Ch, generator=g) / Ch ** 0.5
    b2 = torch.randn(Cout, generator=g) * 0.1
    gy = torch.randn(B, Cout, P, generator=g)
    gy_b = torch.randn(B, Cout, P, generator=g)      # upstream gradient of the second accumulating slab call
    return x, w1, b1, w2, b2, gy, gy_b


def mlp_ref64(x, w1, b1, w2, b2, gy=None):
    """float64 two-layer MLP (1x1 conv -> exact GELU -> 1x1 conv on [B, C, P]) and its explicit backward"""
    x, w1, b1, w2, b2 = [t.double() for t in (x, w1, b1, w2, b2)]
    z = torch.einsum("hi,bip->bhp", w1, x) + b1[None, :, None]
    cdf = 0.5 * (1.0 + torch.erf(z / 2.0 ** 0.5))
    act = z * cdf
    y = torch.einsum("oh,bhp->bop", w2, act) + b2[None, :, None]
    if gy is None:
        return y
    gy = gy.double()
    dact = cdf + z * torch.exp(-0.5 * z * z) / (2.0 * torch.pi) ** 0.5
    gz = torch.einsum("oh,bop->bhp", w2, gy) * dact
    return y, dict(gx=torch.einsum("hi,bhp->bip", w1, gz), gw1=torch.einsum("bhp,bip->hi", gz, x), gb1=gz.sum((0, 2)),
                   gw2=torch.einsum("bop,bhp->oh", gy, act), gb2=gy.sum((0, 2)))


@pytest.mark.parametrize("B,Cin,Ch,Cout,P", [(2, 3, 40, 1, 100), (1, 10, 24, 5, 64)])
def test_float64_reference_matches_oracle_autograd(B, Cin, Ch, Cout, P):
    x, w1, b1, w2, b2, gy, _ = [t.double() for t in make_case(B, Cin, Ch, Cout, P)]
    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y_o = fno_ref.pw_mlp(leaves[0][..., None], *leaves[1:])[..., 0]
    y_o.backward(gy)
    y, grads = mlp_ref64(x, w1, b1, w2, b2, gy)
    assert rel_err(y, y_o) <= 1e-12
    for leaf, name in zip(leaves, ("gx", "gw1", "gb1", "gw2", "gb2")):
        assert rel_err(grads[name], leaf.grad) <= 1e-12, name


@pytest.fixture(scope="module")
def L(cuda):
    from dlwp_benchmark_amd import lib
    lib.load()
    return lib


def padded(dev, *shape):
    """a buffer of `shape` in front of a sentinel tail that no kernel may touch (returns the view and the tail)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 256,), SENTINEL, device=dev)
    return flat[:n].view(*shape), flat[n:]


def pwmlp_names(acc):
    return sorted({r["name"] for r in acc.rows if r["name"].startswith("pwmlp")})


@pytest.mark.gpu
@pytest.mark.parametrize("case", SCALAR_CASES + CONTROL_CASES, ids=case_id)
def test_pwmlp_paths(L, cuda, case):
    B, Cin, Ch, Cout, P = case
    lib = L.load()
    key = case_id(case)
    x, w1, b1, w2, b2, gy, gy_b = make_case(*case)
    y_ref, ref = mlp_ref64(x, w1, b1, w2, b2, gy)
    _, ref_b = mlp_ref64(x, w1, b1, w2, b2, gy_b)
    dx, dw1, db1, dw2, db2, dgy, dgy_b = [t.to(cuda) for t in (x, w1, b1, w2, b2, gy, gy_b)]
    nib, nob = (Cin + 15) // 16, (Cout + 15) // 16
    if Cout == 1:
        want = {"fwd": ["pwmlp_fwd_kernel<1, 16>"], "bwd": ["pwmlp_bwd_kernel<%d, 0, 8>" % nib]}
    else:
        want = {"fwd": ["pwmlp_fwd_kernel<%d, 16>" % nob], "bwd": ["pwmlp_bwd_kernel<%d, %d, 8>" % (nib, nob)]}
    err, ran = {}, {}

    # forward
    y, y_tail = padded(cuda, B, Cout, P)
    with L.kernel_accounting() as acc:
        L.check(lib.dlwp_pwmlp_fwd(L.ptr(dx), L.ptr(dw1), L.ptr(db1), L.ptr(dw2), L.ptr(db2), y.data_ptr(),
                                   B, Cin, Ch, Cout, P, L.stream()))
        torch.cuda.synchronize()
    ran["fwd"] = pwmlp_names(acc)
    err["y"] = rel_err(y, y_ref)

    # backward, float-atomic epilogue
    gx, gx_tail = padded(cuda, B, Cin, P)
    gw1, gb1, gw2, gb2 = [torch.zeros_like(t) for t in (dw1, db1, dw2, db2)]
    with L.kernel_accounting() as acc:
        L.check(lib.dlwp_pwmlp_bwd(L.ptr(dx), L.ptr(dw1), L.ptr(db1), L.ptr(dw2), L.ptr(dgy), gx.data_ptr(),
                                   L.ptr(gw1), L.ptr(gb1), L.ptr(gw2), L.ptr(gb2), B, Cin, Ch, Cout, P, L.stream()))
        torch.cuda.synchronize()
    ran["bwd"] = pwmlp_names(acc)
    for name, got in (("gx", gx), ("gw1", gw1), ("gb1", gb1), ("gw2", gw2), ("gb2", gb2)):
        err[name] = rel_err(got, ref[name])

    # backward, slab epilogue: a plain-store call, an accumulating call, one fold; twice, for the run-to-run bits
    def slab_pass():
        sgx, tail = padded(cuda, B, Cin, P)
        slab = torch.full((lib.dlwp_pwmlp_slab_floats(B, Cin, Ch, Cout, P),), 1e30, device=cuda)   # last step's values must not leak
        g = [torch.zeros_like(t) for t in (dw1, db1, dw2, db2)]
        L.check(lib.dlwp_pwmlp_bwd_slab(L.ptr(dx), L.ptr(dw1), L.ptr(db1), L.ptr(dw2), L.ptr(dgy), sgx.data_ptr(), L.ptr(slab), 0,
                                        B, Cin, Ch, Cout, P, L.stream()))
        L.check(lib.dlwp_pwmlp_bwd_slab(L.ptr(dx), L.ptr(dw1), L.ptr(db1), L.ptr(dw2), L.ptr(dgy_b), sgx.data_ptr(), L.ptr(slab), 1,
                                        B, Cin, Ch, Cout, P, L.stream()))
        L.check(lib.dlwp_pwmlp_slab_fold(L.ptr(slab), *[L.ptr(t) for t in g], B, Cin, Ch, Cout, P, L.stream()))
        torch.cuda.synchronize()
        return [sgx] + g, tail

    with L.kernel_accounting() as acc:
        first, s_tail = slab_pass()
    ran["slab"] = pwmlp_names(acc)
    second, _ = slab_pass()
    err["s_gx"] = rel_err(first[0], ref_b["gx"])
    for name, got in zip(("gw1", "gb1", "gw2", "gb2"), first[1:]):
        err["s_" + name] = rel_err(got, ref[name] + ref_b[name])

    report("entries", key, err, ran)
    assert ran["fwd"] == want["fwd"] and ran["bwd"] == want["bwd"] and ran["slab"] == want["bwd"], ran
    for tail in (y_tail, gx_tail, s_tail):
        assert bool((tail == SENTINEL).all()), "a kernel wrote past the end of its output"
    for a, b_, name in zip(first, second, ("gx", "gw1", "gb1", "gw2", "gb2")):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), "slab mode repeats bit for bit: " + name
    for name, e in err.items():
        tol = FWD_TOL if name == "y" else GRAD_TOL
        assert e <= tol, (name, e)
        assert e <= bar(PARENT_ERR, key, name, tol), (name, e, PARENT_ERR[key][name])


def rollout_pair(cuda, D, hidden, ctx, dtype=torch.float64):
    """a TFNO2D rollout module on the GPU and the float64 oracle with the same parameters"""
    from dlwp_benchmark_amd import nsbench
    n_modes, n_layers = (12, 12), 2
    oracle = fno_ref.FNO(n_modes, D * ctx, hidden, 256, 256, D, n_layers, seed=99, dtype=dtype)
    module = nsbench.TFNO2DModule(n_modes=list(n_modes), in_channels=D, hidden_channels=hidden, lifting_channels=256,
                                  projection_channels=256, out_channels=D, n_layers=n_layers, type="TFNO2DModule", name="t",
                                  context_size=ctx)
    def f32(v):
        return v.to(torch.complex64) if v.is_complex() else v.float()

    sd = {}
    for k, v in oracle.params.items():
        v = f32(v)
        if ".convs.weight." in k:
            sd["fno." + k + ".tensor"] = v
        elif ".convs.bias." in k:
            continue
        elif k.endswith("weight"):
            sd["fno." + k] = v[:, :, None, None]
        else:
            sd["fno." + k] = v
    sd["fno.fno_blocks.convs.bias"] = torch.stack(
        [f32(oracle.params[f"fno_blocks.convs.bias.{l}"]) for l in range(n_layers)])[:, :, None, None]
    module.load_state_dict(sd)
    for k in oracle.params:                      # the oracle computes in float64 from the fp32-rounded parameters
        v = f32(oracle.params[k])
        oracle.params[k] = v.to(torch.complex128) if v.is_complex() else v.double()
    return oracle, module.to(cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 2], ids=["scalar-field", "two-field-control"])
def test_chained_forward_as_the_trainer_reaches_it(L, cuda, D):
    """closed-loop rollout on a 64 x 64 grid: the projection of net call k and the lifting of call k + 1 run as one launch,
    the new frame handed over in LDS; the prediction is held to the float64 oracle"""
    oracle, module = rollout_pair(cuda, D, 32, 3)
    g = torch.Generator().manual_seed(2468)
    x = torch.randn(2, 8, D, 64, 64, generator=g)
    with torch.no_grad():
        yhat_ref = fno_ref.ns_rollout(oracle, x.double(), 4, 3)
        with L.kernel_accounting() as acc:
            yhat = module(x.to(cuda), teacher_forcing_steps=4)
            torch.cuda.synchronize()
    names = pwmlp_names(acc)
    key = "D%d" % D
    err = {"yhat": rel_err(yhat, yhat_ref), "last": rel_err(yhat[:, -1], yhat_ref[:, -1])}
    report("rollout", key, err, names)
    assert "pwmlp_fwd_chain_kernel<1, 2, 16>" in names, names
    for name, e in err.items():
        assert e <= FWD_TOL, (name, e)
        assert e <= bar(PARENT_ERR_ROLLOUT, key, name, FWD_TOL), (name, e, PARENT_ERR_ROLLOUT[key][name])
