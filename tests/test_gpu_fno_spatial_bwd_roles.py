"""Backward of one FNO block -- g_x, the skip-weight gradient and the bias gradient -- against a float64 computation done
here, on both epilogues of the backward `spatial` kernel: the float atomics of dlwp_fno_block_bwd and the per-workgroup slab
as the rollout trainer runs it (a plain-store call, an accumulating call, one fold: dlwp_fno_block_bwd_slab twice +
dlwp_fno_block_slab_fold).

The backward `spatial` launch gives the skip-weight / bias gradient work to four waves of its own next to the four that
compute g_x (fno_spatial_roles_kernel); where the larger LDS footprint does not fit it launches the four-wave kernel it
always launched.  Shapes: every channel-tile count of the narrow kernel (C 8, 27, 32, 38, 54, 64 -> 1 .. 4 tiles of 16) at
B 1 and 4 with the block input activated and not, on the 64 x 64 grid of the headline (C 54 and 64 take the four-wave
fallback there: 161.5 KiB of LDS), C 64 on a 32 x 32 grid (four tiles in the two-role form), and a shape with two table tiles
(n_modes[1] 18).

Error bars.  Every figure is a max-norm relative error against the float64 reference.  The change is one of scheduling:
every sum keeps its order, so the slab outputs and g_x are bit for bit the previous build's.  The bar of an output is TWICE
the error the previous (four-wave only) build made on the same seeded inputs, measured on MI355X and recorded in PARENT_ERR
beside the case, and never more than the 5e-4 of tests/test_gpu_fno.py.  g_x and everything in slab mode are
deterministic: one measurement is the previous build's error.  gk and gb of the float-atomic epilogue depend on the order
in which 256 workgroups' atomics arrive and vary run to run on one build, so the previous build's figure for those is its
largest over 20 runs.  Each test prints its figures before it asserts; FNO_ROLES_REPORT=<file> appends them as JSON lines.
"""
import ctypes as C
import json
import os

import pytest
import torch

from oracle import fno_ref

GRAD_TOL = 5e-4
SENTINEL = 12345.0

CASES = ([(B, Cc, 64, 64, (12, 12), act) for Cc in (8, 27, 32, 38, 54, 64) for B in (1, 4) for act in (0, 1)]
         + [(B, 64, 32, 32, (12, 12), act) for B in (1, 4) for act in (0, 1)]
         + [(2, 20, 32, 64, (8, 18), 1)])


def case_id(c):
    return "B%d-C%d-%dx%d-m%dx%d-act%d" % (c[0], c[1], c[2], c[3], c[4][0], c[4][1], c[5])


# max-norm relative error of the previous build (four-wave kernel on every shape) against the float64 reference, MI355X, the
# seeded inputs of make_case(), rounded up to three digits; keys: gx, gk, gb (dlwp_fno_block_bwd; gk, gb: largest of 20 runs),
# s_gx, s_gk, s_gb (two dlwp_fno_block_bwd_slab calls + dlwp_fno_block_slab_fold)
PARENT_ERR = {
    "B1-C8-64x64-m12x12-act0": {"gx": 1.89e-07, "gk": 3.93e-07, "gb": 4.63e-07, "s_gx": 1.90e-07, "s_gk": 1.03e-07, "s_gb": 2.40e-07},
    "B1-C8-64x64-m12x12-act1": {"gx": 2.46e-07, "gk": 6.65e-07, "gb": 2.69e-07, "s_gx": 2.46e-07, "s_gk": 1.73e-07, "s_gb": 1.15e-07},
    "B4-C8-64x64-m12x12-act0": {"gx": 2.89e-07, "gk": 4.42e-07, "gb": 9.76e-07, "s_gx": 2.37e-07, "s_gk": 2.77e-07, "s_gb": 3.26e-07},
    "B4-C8-64x64-m12x12-act1": {"gx": 1.70e-07, "gk": 7.48e-07, "gb": 6.15e-07, "s_gx": 2.18e-07, "s_gk": 2.27e-07, "s_gb": 1.58e-07},
    "B1-C27-64x64-m12x12-act0": {"gx": 2.11e-07, "gk": 2.89e-07, "gb": 2.93e-07, "s_gx": 2.89e-07, "s_gk": 1.21e-07, "s_gb": 1.39e-07},
    "B1-C27-64x64-m12x12-act1": {"gx": 3.09e-07, "gk": 2.83e-07, "gb": 3.41e-07, "s_gx": 2.92e-07, "s_gk": 1.45e-07, "s_gb": 2.13e-07},
    "B4-C27-64x64-m12x12-act0": {"gx": 2.70e-07, "gk": 6.19e-07, "gb": 5.24e-07, "s_gx": 2.87e-07, "s_gk": 1.88e-07, "s_gb": 1.63e-07},
    "B4-C27-64x64-m12x12-act1": {"gx": 2.88e-07, "gk": 7.95e-07, "gb": 6.78e-07, "s_gx": 3.13e-07, "s_gk": 2.02e-07, "s_gb": 2.92e-07},
    "B1-C32-64x64-m12x12-act0": {"gx": 2.85e-07, "gk": 3.25e-07, "gb": 4.40e-07, "s_gx": 3.92e-07, "s_gk": 1.09e-07, "s_gb": 1.52e-07},
    "B1-C32-64x64-m12x12-act1": {"gx": 2.48e-07, "gk": 3.41e-07, "gb": 5.48e-07, "s_gx": 2.68e-07, "s_gk": 1.65e-07, "s_gb": 1.91e-07},
    "B4-C32-64x64-m12x12-act0": {"gx": 2.77e-07, "gk": 7.61e-07, "gb": 4.78e-07, "s_gx": 3.29e-07, "s_gk": 2.11e-07, "s_gb": 2.88e-07},
    "B4-C32-64x64-m12x12-act1": {"gx": 3.31e-07, "gk": 7.15e-07, "gb": 8.31e-07, "s_gx": 2.92e-07, "s_gk": 2.06e-07, "s_gb": 2.17e-07},
    "B1-C38-64x64-m12x12-act0": {"gx": 3.78e-07, "gk": 3.76e-07, "gb": 3.14e-07, "s_gx": 2.62e-07, "s_gk": 1.45e-07, "s_gb": 1.16e-07},
    "B1-C38-64x64-m12x12-act1": {"gx": 3.17e-07, "gk": 3.43e-07, "gb": 2.80e-07, "s_gx": 2.99e-07, "s_gk": 1.28e-07, "s_gb": 1.02e-07},
    "B4-C38-64x64-m12x12-act0": {"gx": 3.21e-07, "gk": 7.52e-07, "gb": 6.49e-07, "s_gx": 3.33e-07, "s_gk": 2.92e-07, "s_gb": 2.60e-07},
    "B4-C38-64x64-m12x12-act1": {"gx": 4.28e-07, "gk": 7.04e-07, "gb": 7.04e-07, "s_gx": 2.94e-07, "s_gk": 2.50e-07, "s_gb": 2.37e-07},
    "B1-C54-64x64-m12x12-act0": {"gx": 3.25e-07, "gk": 3.11e-07, "gb": 3.26e-07, "s_gx": 4.03e-07, "s_gk": 1.56e-07, "s_gb": 1.35e-07},
    "B1-C54-64x64-m12x12-act1": {"gx": 2.84e-07, "gk": 3.51e-07, "gb": 2.65e-07, "s_gx": 3.62e-07, "s_gk": 1.61e-07, "s_gb": 2.00e-07},
    "B4-C54-64x64-m12x12-act0": {"gx": 3.65e-07, "gk": 5.71e-07, "gb": 7.41e-07, "s_gx": 3.34e-07, "s_gk": 2.49e-07, "s_gb": 2.70e-07},
    "B4-C54-64x64-m12x12-act1": {"gx": 4.12e-07, "gk": 6.61e-07, "gb": 4.72e-07, "s_gx": 3.70e-07, "s_gk": 2.58e-07, "s_gb": 1.52e-07},
    "B1-C64-64x64-m12x12-act0": {"gx": 3.20e-07, "gk": 3.78e-07, "gb": 2.58e-07, "s_gx": 2.79e-07, "s_gk": 9.67e-08, "s_gb": 1.66e-07},
    "B1-C64-64x64-m12x12-act1": {"gx": 3.19e-07, "gk": 3.42e-07, "gb": 3.71e-07, "s_gx": 3.69e-07, "s_gk": 1.43e-07, "s_gb": 1.68e-07},
    "B4-C64-64x64-m12x12-act0": {"gx": 4.37e-07, "gk": 7.24e-07, "gb": 6.99e-07, "s_gx": 4.12e-07, "s_gk": 1.98e-07, "s_gb": 2.09e-07},
    "B4-C64-64x64-m12x12-act1": {"gx": 3.11e-07, "gk": 8.31e-07, "gb": 6.23e-07, "s_gx": 3.93e-07, "s_gk": 2.38e-07, "s_gb": 2.95e-07},
    "B1-C64-32x32-m12x12-act0": {"gx": 3.20e-07, "gk": 2.43e-07, "gb": 2.74e-07, "s_gx": 3.44e-07, "s_gk": 1.56e-07, "s_gb": 8.03e-08},
    "B1-C64-32x32-m12x12-act1": {"gx": 3.62e-07, "gk": 3.08e-07, "gb": 2.49e-07, "s_gx": 3.39e-07, "s_gk": 1.43e-07, "s_gb": 1.64e-07},
    "B4-C64-32x32-m12x12-act0": {"gx": 3.56e-07, "gk": 5.57e-07, "gb": 5.04e-07, "s_gx": 3.51e-07, "s_gk": 1.33e-07, "s_gb": 1.32e-07},
    "B4-C64-32x32-m12x12-act1": {"gx": 3.28e-07, "gk": 4.52e-07, "gb": 4.05e-07, "s_gx": 3.74e-07, "s_gk": 2.18e-07, "s_gb": 1.63e-07},
    "B2-C20-32x64-m8x18-act1": {"gx": 2.70e-07, "gk": 3.74e-07, "gb": 4.64e-07, "s_gx": 2.76e-07, "s_gk": 1.66e-07, "s_gb": 1.83e-07},
}


def bar(key, name):
    """twice the previous build's error, inside the suite's tolerance"""
    return min(2.0 * PARENT_ERR[key][name], GRAD_TOL)


def report(key, figures):
    line = {"case": key, "err": figures}
    print(json.dumps(line))
    path = os.environ.get("FNO_ROLES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def make_case(B, Cc, H, W, n_modes, act):
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    g = torch.Generator().manual_seed(977 + 3 * Cc + 11 * B + H + 5 * n_modes[1] + act)
    x = torch.randn(B, Cc, H, W, generator=g)
    wspec = torch.view_as_complex(torch.randn(Cc, Cc, m1, m2c, 2, generator=g) / Cc ** 0.5)
    wskip = torch.randn(Cc, Cc, generator=g) / Cc ** 0.5
    bias = torch.randn(Cc, generator=g) * 0.1
    gpre = torch.randn(B, Cc, H, W, generator=g)
    gpre_b = torch.randn(B, Cc, H, W, generator=g)     # upstream gradient of the second accumulating slab call
    return x, wspec, wskip, bias, gpre, gpre_b


def block_ref64(x, wspec, wskip, n_modes, act, gpre):
    """float64: pre = irfft2(mode-truncated rfft2(a) . wspec) + wskip . a with a = gelu(x) if act else x (exact erf GELU);
    returns d/dx, d/dwskip, d/dbias of <pre, gpre>.  The skip and bias gradients are written out; g_x of the spectral path
    comes from autograd on the float64 forward below."""
    x = x.double().clone().requires_grad_(True)
    wspec, wskip, gpre = wspec.to(torch.complex128), wskip.double(), gpre.double()
    B, Cc, H, W = x.shape
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    a = x * 0.5 * (1.0 + torch.erf(x / 2.0 ** 0.5)) if act else x
    X = torch.fft.fftshift(torch.fft.rfftn(a, dim=(-2, -1), norm="forward"), dim=-2)
    lo = (H - m1) // 2
    out = torch.zeros(B, Cc, H, W // 2 + 1, dtype=torch.complex128)
    out[:, :, lo:lo + m1, :m2c] = torch.einsum("bixy,ioxy->boxy", X[:, :, lo:lo + m1, :m2c], wspec)
    y = torch.fft.irfftn(torch.fft.fftshift(out, dim=-2), s=(H, W), dim=(-2, -1), norm="forward")
    pre = y + torch.einsum("oi,bihw->bohw", wskip, a)
    (gx,) = torch.autograd.grad(pre, x, gpre)
    return dict(gx=gx, gk=torch.einsum("bohw,bihw->oi", gpre, a.detach()), gb=gpre.sum((0, 2, 3)))


@pytest.mark.parametrize("B,Cc,H,W,n_modes,act", [(2, 6, 16, 16, (8, 8), 1), (1, 5, 8, 16, (4, 6), 0)])
def test_float64_reference_matches_oracle_autograd(B, Cc, H, W, n_modes, act):
    x, wspec, wskip, bias, gpre, _ = make_case(B, Cc, H, W, n_modes, act)
    xr, kr, br = [t.double().clone().requires_grad_(True) for t in (x, wskip, bias)]
    xin = torch.nn.functional.gelu(xr) if act else xr
    fno_ref.fno_block(xin, wspec.to(torch.complex128), kr, br, list(n_modes)).backward(gpre.double())
    ref = block_ref64(x, wspec, wskip, n_modes, act, gpre)
    for name, leaf in (("gx", xr), ("gk", kr), ("gb", br)):
        assert rel_err(ref[name], leaf.grad) <= 1e-12, name


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


def run_case(L, cuda, case, atomic_runs=1):
    """errors of both epilogues for one case (gk, gb of the atomics path: largest of atomic_runs runs), the sentinel tails and
    the two slab passes"""
    B, Cc, H, W, n_modes, act = case
    lib = L.load()
    m1, m2c = n_modes[0], n_modes[1] // 2 + 1
    x, wspec, wskip, bias, gpre, gpre_b = make_case(*case)
    ref = block_ref64(x, wspec, wskip, n_modes, act, gpre)
    ref_b = block_ref64(x, wspec, wskip, n_modes, act, gpre_b)
    plan = C.c_void_p()
    L.check(lib.dlwp_fno_plan_create(Cc, H, W, m1, m2c, C.byref(plan)))
    err, tails = {}, []
    try:
        ws = torch.empty(lib.dlwp_fno_block_workspace_bytes(plan, B), dtype=torch.uint8, device=cuda)
        dx, dk, db, dg, dg_b = [t.to(cuda) for t in (x, wskip, bias, gpre, gpre_b)]
        dw = fno_ref.spec_to_mode_major(wspec).to(cuda)
        pre = torch.empty(B, Cc, H, W, device=cuda)
        xhat = torch.empty(B, m1, m2c, Cc, 2, device=cuda)
        L.check(lib.dlwp_fno_block_fwd(plan, L.ptr(dx), act, L.ptr(dw), L.ptr(dk), L.ptr(db), L.ptr(pre), L.ptr(xhat), B,
                                       L.ptr(ws), L.stream()))
        # float-atomic epilogue
        for _ in range(atomic_runs):
            gx, tail = padded(cuda, B, Cc, H, W)
            gw, gk, gb = torch.zeros_like(dw), torch.zeros_like(dk), torch.zeros_like(db)
            L.check(lib.dlwp_fno_block_bwd(plan, L.ptr(dx), act, L.ptr(dw), L.ptr(dk), L.ptr(dg), L.ptr(xhat), gx.data_ptr(),
                                           L.ptr(gw), L.ptr(gk), L.ptr(gb), B, L.ptr(ws), L.stream()))
            torch.cuda.synchronize()
            tails.append(tail)
            for name, got in (("gx", gx), ("gk", gk), ("gb", gb)):
                err[name] = max(err.get(name, 0.0), rel_err(got, ref[name]))

        # slab epilogue: a plain-store call, an accumulating call, one fold
        def slab_pass():
            sgx, tail = padded(cuda, B, Cc, H, W)
            slab = torch.full((lib.dlwp_fno_block_slab_floats(plan, B),), 1e30, device=cuda)   # stale values must not leak
            gw, gk, gb = torch.zeros_like(dw), torch.zeros_like(dk), torch.zeros_like(db)
            for acc, up in ((0, dg), (1, dg_b)):
                L.check(lib.dlwp_fno_block_bwd_slab(plan, L.ptr(dx), act, L.ptr(dw), L.ptr(dk), L.ptr(up), L.ptr(xhat),
                                                    sgx.data_ptr(), L.ptr(gw), L.ptr(slab), acc, B, L.ptr(ws), L.stream()))
            L.check(lib.dlwp_fno_block_slab_fold(plan, L.ptr(slab), L.ptr(gk), L.ptr(gb), B, L.stream()))
            torch.cuda.synchronize()
            return [sgx, gk, gb], tail

        first, tail = slab_pass()
        tails.append(tail)
        second, _ = slab_pass()
        err["s_gx"] = rel_err(first[0], ref_b["gx"])
        err["s_gk"] = rel_err(first[1], ref["gk"] + ref_b["gk"])
        err["s_gb"] = rel_err(first[2], ref["gb"] + ref_b["gb"])
    finally:
        lib.dlwp_fno_plan_destroy(plan)
    return err, tails, first, second


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fno_block_bwd_both_epilogues(L, cuda, case):
    key = case_id(case)
    err, tails, first, second = run_case(L, cuda, case)
    report(key, err)
    for tail in tails:
        assert bool((tail == SENTINEL).all()), "a kernel wrote past the end of g_x"
    for a, b_, name in zip(first, second, ("gx", "gk", "gb")):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), "slab mode repeats bit for bit: " + name
    for name, e in err.items():
        assert e <= GRAD_TOL, (name, e)
        assert e <= bar(key, name), (name, e, PARENT_ERR[key][name])
