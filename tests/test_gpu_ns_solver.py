"""The seeded GPU Navier-Stokes generator (csrc/ns_solver.hip, nsdata.py, docs/kernels/data.md "Navier-Stokes generator").

Single launches against float64: dlwp_ns2d_grf against the symmetrised spectrum built from tests/batch_ref.py, and the three
solver kernels against the float64 expressions of nsdata.navier_stokes_2d on the half spectrum.  Shapes n = 8 and 12 (the smallest
with a Nyquist row and column of their own and an odd half width; at n = 12 the 2/3 cutoff |k| <= 4 falls exactly on a mode),
B = 3, and n = 32.  Then the whole solver against the float64 CPU solver, the same seed on either device, batch and slice
invariance (bit for bit), and the device-resident results.

Bounds of the single launches: relative max-norm, 4 x the largest value measured on an MI355X over the shapes below (the margin
covers fp32 logf / sincospif / powf / division differences between inputs), and none above 1e-5: an index, sign or Nyquist
mistake gives an error of order 1.  Measured values and bounds are listed in docs/kernels/data.md.  The solver bounds (2e-4
relative max, sol_t to 1e-6) are those of tests/test_gpu_nsdata.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TAG = 0x6772
ALPHA, TAU = 2.5, 7.0
SHAPES = [8, 12, 32]
B = 3
# relative max-norm bounds of the single launches: 4 x measured (see the module docstring).  Measured on an MI355X over the
# cases of this file: grf 1.76e-7, field (irFFT2 of it, against the CPU's float64 field) 2.47e-7, terms 1.11e-7,
# advect 9.60e-8, cn 9.82e-8
BOUND = {"grf": 7.1e-7, "field": 9.9e-7, "terms": 4.5e-7, "advect": 3.9e-7, "cn": 4.0e-7}
assert max(BOUND.values()) <= 1e-5


@pytest.fixture(scope="module")
def lib():
    from dlwp_benchmark_amd import lib as L
    return L


def rel(got, ref):
    """relative max-norm error of a device tensor against a float64 CPU tensor"""
    got = got.detach().cpu()
    got = got.to(torch.complex128) if ref.is_complex() else got.double()
    return float((got - ref).abs().max() / ref.abs().max())


def check(name, what, err):
    print(f"{what}: relative max error {err:.3e} (bound {BOUND[name]:.1e})")
    assert err <= BOUND[name], (what, err)


# ---- float64 references
def sqrt_eig64(n, alpha=ALPHA, tau=TAU):
    k = np.concatenate((np.arange(0, n // 2), np.arange(-(n // 2), 0))).astype(np.float64)
    sigma = tau ** (0.5 * (2 * alpha - 2))
    se = n ** 2 * math.sqrt(2.0) * sigma * (4 * math.pi ** 2 * (k[:, None] ** 2 + k[None, :] ** 2) + tau ** 2) ** (-alpha / 2.0)
    se[0, 0] = 0.0
    return se, sigma


def half_spectrum64(n, seed, sample):
    """H[a, b] = (c[a, b] + conj(c[-a mod n, -b mod n])) / 2 for b <= n/2, c from the float64 stream"""
    se, _ = sqrt_eig64(n)
    z = batch_ref.normals(seed, 0, sample, 2 * n * n, TAG).reshape(n, n, 2)
    c = se * (z[..., 0] + 1j * z[..., 1])
    mirror = np.conj(np.roll(c[::-1, ::-1], (1, 1), axis=(0, 1)))          # [a, b] -> conj(c[(n - a) % n, (n - b) % n])
    return torch.from_numpy(0.5 * (c + mirror)[:, : n // 2 + 1])


def solver_parts64(n):
    """k_x, k_y, lap, dealias of nsdata.navier_stokes_2d, cut to the half spectrum"""
    from dlwp_benchmark_amd import nsdata
    k_x, k_y, k_max = nsdata._wavenumbers(n, "cpu")
    lap = 4 * math.pi ** 2 * (k_x ** 2 + k_y ** 2)
    lap[0, 0] = 1.0
    dealias = ((k_y.abs() <= (2.0 / 3.0) * k_max) & (k_x.abs() <= (2.0 / 3.0) * k_max)).double()
    wc = n // 2 + 1
    return k_x[:, :wc], k_y[:, :wc], lap[:, :wc], dealias[:, :wc]


def hermitian_state(n, batch, seed):
    """complex64 half spectrum [batch, n, n/2+1] of a random real field (Nyquist row and column populated), on the CPU"""
    g = torch.Generator().manual_seed(seed)
    return torch.fft.rfft2(torch.randn(batch, n, n, generator=g, dtype=torch.float64)).to(torch.complex64)


# ---- single launches
def run_grf(lib, cuda, seed, first, batch, n, out=None):
    H = torch.empty(batch, n, n // 2 + 1, 2, device=cuda) if out is None else out
    lib.check(lib.load().dlwp_ns2d_grf(seed, first, batch, n, ALPHA, TAU, sqrt_eig64(n)[1], lib.ptr(H), lib.stream()))
    return H


def run_terms(lib, w):
    batch, n = w.shape[0], w.shape[1]
    out = torch.empty(batch, 4, n, n // 2 + 1, 2, device=w.device)
    lib.check(lib.load().dlwp_ns2d_spectral_terms(lib.ptr(w), lib.ptr(out), batch, n, lib.stream()))
    return out


def run_advect(lib, fields):
    batch, n = fields.shape[0], fields.shape[-1]
    out = torch.empty(batch, n, n, device=fields.device)
    lib.check(lib.load().dlwp_ns2d_advect(lib.ptr(fields), lib.ptr(out), batch, n, lib.stream()))
    return out


def run_cn(lib, w, F, f, dt, visc):
    batch, n = w.shape[0], w.shape[1]
    w = w.clone()
    lib.check(lib.load().dlwp_ns2d_cn_update(lib.ptr(w), lib.ptr(F), lib.ptr(f), int(f.dim() == 4), batch, n, dt, visc, lib.stream()))
    return w


def as_real(z, cuda):
    return torch.view_as_real(z).contiguous().to(cuda)


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("seed,first", [(5, 0), (2 ** 40 + 9, 2), (5, 2 ** 32 - 3)])
def test_grf_spectrum_against_float64(lib, cuda, n, seed, first):
    H = torch.view_as_complex(run_grf(lib, cuda, seed, first, B, n))
    for i in range(B):
        ref = half_spectrum64(n, seed, first + i)
        check("grf", f"grf n {n} seed {seed} sample {first + i}", rel(H[i], ref))
    assert H[:, 0, 0].abs().max() == 0 and H[:, n // 2, n // 2].imag.abs().max() == 0          # the mean; a self-mirrored mode is real


@pytest.mark.parametrize("n", SHAPES)
def test_grf_field_is_the_cpu_field(cuda, n):
    from dlwp_benchmark_amd import nsdata
    cpu = nsdata.GaussianRF(n, alpha=ALPHA, tau=TAU, rng="philox", seed=5, device="cpu").sample(B, first_sample=1)
    gpu = nsdata.GaussianRF(n, alpha=ALPHA, tau=TAU, rng="philox", seed=5, device=cuda).sample(B, first_sample=1)
    assert gpu.is_cuda and gpu.dtype == torch.float32 and gpu.shape == cpu.shape
    for i in range(B):
        check("field", f"field n {n} sample {1 + i}", rel(gpu[i], cpu[i].double()))


@pytest.mark.parametrize("n", SHAPES)
def test_spectral_terms_against_float64(lib, cuda, n):
    w = hermitian_state(n, B, 1)
    k_x, k_y, lap, _ = solver_parts64(n)
    w64 = w.to(torch.complex128)
    psi = w64 / lap
    ikx, iky = 2j * math.pi * k_x, 2j * math.pi * k_y
    ref = torch.stack((iky * psi, -ikx * psi, ikx * w64, iky * w64), dim=1)
    got = torch.view_as_complex(run_terms(lib, as_real(w, cuda)))
    assert w[:, n // 2].abs().min() > 0 and w[:, :, n // 2].abs().min() > 0          # the Nyquist row and column take part
    for c, name in enumerate(("i k_y psi", "-i k_x psi", "i k_x w", "i k_y w")):
        check("terms", f"terms n {n} {name}", rel(got[:, c], ref[:, c]))


@pytest.mark.parametrize("n", SHAPES)
def test_advect_against_float64(lib, cuda, n):
    fields = torch.randn(B, 4, n, n, generator=torch.Generator().manual_seed(2))
    f64 = fields.double()
    check("advect", f"advect n {n}", rel(run_advect(lib, fields.to(cuda)), f64[:, 0] * f64[:, 2] + f64[:, 1] * f64[:, 3]))


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("batched", [False, True])
def test_cn_update_against_float64(lib, cuda, n, batched):
    dt, visc = 1e-2, 1e-3
    w, F = hermitian_state(n, B, 3), hermitian_state(n, B, 4)
    f = hermitian_state(n, B if batched else 1, 5)
    f = f if batched else f[0]
    _, _, lap, dealias = solver_parts64(n)
    num, den = 1.0 - 0.5 * dt * visc * lap, 1.0 + 0.5 * dt * visc * lap
    ref = (-dt * dealias * F.to(torch.complex128) + dt * f.to(torch.complex128) + num * w.to(torch.complex128)) / den
    got = torch.view_as_complex(run_cn(lib, as_real(w, cuda), as_real(F, cuda), as_real(f, cuda), dt, visc))
    check("cn", f"cn_update n {n} {'batched' if batched else 'shared'} forcing", rel(got, ref))
    if n == 12:      # the cutoff lies on a mode: |k| = 4 is kept, |k| = 5 is not
        assert dealias[4, 4] == 1 and dealias[8, 4] == 1 and dealias[5, 0] == 0 and dealias[0, 5] == 0 and dealias[6, 6] == 0
        only_F = torch.view_as_complex(run_cn(lib, as_real(torch.zeros_like(w), cuda), as_real(F, cuda),
                                              as_real(torch.zeros_like(f), cuda), dt, visc)).cpu()
        assert ((only_F != 0) == (dealias != 0)).all()


def test_scalar_form_gives_the_vector_forms_bits(lib, cuda):
    """arrays that are 8-byte but not 16-byte aligned take two 8-byte accesses per pair: the same bits"""
    n, wc = 12, 7

    def shifted(t):      # the same values, 8 bytes off a 16-byte boundary
        buf = torch.empty(t.numel() + 2, device=cuda)
        view = buf[2:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 8
        return view

    w, F, f = (as_real(hermitian_state(n, B, s), cuda) for s in (6, 7, 8))
    assert w.data_ptr() % 16 == 0
    assert torch.equal(run_terms(lib, shifted(w)), run_terms(lib, w))
    assert torch.equal(run_cn(lib, shifted(w), shifted(F), shifted(f), 1e-2, 1e-3), run_cn(lib, w, F, f, 1e-2, 1e-3))
    H = run_grf(lib, cuda, 5, 0, B, n)
    assert torch.equal(run_grf(lib, cuda, 5, 0, B, n, out=shifted(torch.zeros(B, n, wc, 2, device=cuda))), H)
    fields = torch.randn(B, 4, n, n, device=cuda)
    buf = torch.empty(fields.numel() + 1, device=cuda)
    off = buf[1:].view(fields.shape)          # 4 bytes off: the scalar loop
    off.copy_(fields)
    assert torch.equal(run_advect(lib, off), run_advect(lib, fields))


def test_kernels_do_not_depend_on_the_batch(lib, cuda):
    """a sample's outputs are the same bits alone, in a batch of 2 and in a batch of 6"""
    n = 8
    H = run_grf(lib, cuda, 7, 0, 6, n)
    assert torch.equal(torch.cat([run_grf(lib, cuda, 7, s, 2, n) for s in (0, 2, 4)]), H)
    assert torch.equal(torch.cat([run_grf(lib, cuda, 7, s, 1, n) for s in range(6)]), H)
    w, F, f = (as_real(hermitian_state(n, 6, s), cuda) for s in (9, 10, 11))
    fields = torch.randn(6, 4, n, n, device=cuda)
    for lo, hi in ((0, 2), (2, 5), (5, 6)):
        assert torch.equal(run_terms(lib, w[lo:hi]), run_terms(lib, w)[lo:hi])
        assert torch.equal(run_advect(lib, fields[lo:hi]), run_advect(lib, fields)[lo:hi])
        assert torch.equal(run_cn(lib, w[lo:hi], F[lo:hi], f[lo:hi], 1e-2, 1e-3), run_cn(lib, w, F, f, 1e-2, 1e-3)[lo:hi])
        assert torch.equal(run_cn(lib, w[lo:hi], F[lo:hi], f[0], 1e-2, 1e-3), run_cn(lib, w, F, f[0], 1e-2, 1e-3)[lo:hi])


# ---- the solver
@pytest.mark.parametrize("n,T,dt,records,alpha", [(64, 2.0, 5e-3, 4, 2.5), (12, 0.2, 1e-2, 2, 2.5)])
def test_device_solver_tracks_the_cpu_solver(cuda, n, T, dt, records, alpha):
    from dlwp_benchmark_amd import nsdata
    g = torch.Generator().manual_seed(4)
    w0 = nsdata.GaussianRF(n, alpha=alpha, tau=7.0, generator=g).sample(3)
    f = nsdata.forcing(n)
    ref, t_ref = nsdata.navier_stokes_2d(w0, f, 1e-3, T=T, delta_t=dt, record_steps=records)
    got, t_got = nsdata.navier_stokes_2d_device(w0.to(cuda), f.to(cuda), 1e-3, T=T, delta_t=dt, record_steps=records)
    assert got.is_cuda and got.shape == ref.shape and got.dtype == torch.float32
    assert torch.allclose(t_got.cpu(), t_ref, atol=1e-6)
    err = rel(got, ref.double())
    print(f"solver n {n}: relative max error {err:.3e} (bound 2.0e-04)")
    assert err <= 2e-4, err
    if n == 12:      # a batched forcing and a caller's buffer give the same frames
        out = torch.zeros(3, records, 1, n, n, device=cuda)
        sol, _ = nsdata.navier_stokes_2d_device(w0.to(cuda), f.to(cuda)[None].repeat(3, 1, 1), 1e-3, T, dt, records, out=out)
        assert sol.data_ptr() == out.data_ptr() and torch.equal(sol, got) and torch.equal(out[:, :, 0].permute(0, 2, 3, 1), got)
    # a forcing [1, n, n] is ONE plane shared by the B = 3 samples, as navier_stokes_2d broadcasts it: the frames of f [n, n]
    one, t_one = nsdata.navier_stokes_2d_device(w0.to(cuda), f.to(cuda)[None], 1e-3, T=T, delta_t=dt, record_steps=records)
    assert torch.equal(one, got) and torch.equal(t_one, t_got)


def test_device_solver_refuses_bad_shapes(cuda):
    from dlwp_benchmark_amd import nsdata
    f = torch.zeros(8, 8, device=cuda)
    for shape in ((8, 8), (2, 8, 6), (2, 7, 7), (2, 2, 2), (0, 8, 8)):
        with pytest.raises(ValueError, match="w0"):
            nsdata.navier_stokes_2d_device(torch.zeros(shape, device=cuda), f, 1e-3, 1, 1e-2)
    for shape in ((2, 8, 8), (8, 6), (3, 3, 8, 8)):
        with pytest.raises(ValueError, match="f must"):
            nsdata.navier_stokes_2d_device(torch.zeros(3, 8, 8, device=cuda), torch.zeros(shape, device=cuda), 1e-3, 1, 1e-2)


KW32 = dict(resolution=32, n_samples=4, batch_size=4, max_simulation_time=3, delta_t=1e-2, rng="philox", seed=5)


def test_same_seed_on_either_device(cuda):
    from dlwp_benchmark_amd import nsdata
    cpu = nsdata.generate_data(device="cpu", **KW32)
    gpu = nsdata.generate_data(device=cuda, solver="kernels", **KW32)
    assert gpu["a"].shape == cpu["a"].shape and gpu["u"].shape == cpu["u"].shape and gpu["attrs"] == cpu["attrs"]
    assert np.allclose(gpu["t"], cpu["t"], atol=1e-6)
    for i in range(4):
        check("field", f"generate_data a[{i}]", rel(torch.from_numpy(gpu["a"][i]), torch.from_numpy(cpu["a"][i]).double()))
    err = rel(torch.from_numpy(gpu["u"]), torch.from_numpy(cpu["u"]).double())
    print(f"generate_data u: relative max error {err:.3e} (bound 2.0e-04)")
    assert err <= 2e-4, err
    # the torch solver on the same device-drawn fields: the two GPU solvers agree as well
    hip = nsdata.generate_data(device=cuda, solver="torch", **KW32)
    assert np.array_equal(hip["a"], gpu["a"]) and rel(torch.from_numpy(hip["u"]), torch.from_numpy(cpu["u"]).double()) <= 2e-4


KW8 = dict(resolution=8, max_simulation_time=1, delta_t=1e-2, rng="philox", seed=7, solver="kernels")


@pytest.fixture(scope="module")
def whole8(cuda):
    from dlwp_benchmark_amd import nsdata
    return nsdata.generate_data(n_samples=6, batch_size=6, device=cuda, **KW8)


@pytest.mark.parametrize("batch_size", [2, 3])
def test_generate_data_is_batch_invariant_on_the_device(cuda, whole8, batch_size):
    from dlwp_benchmark_amd import nsdata
    got = nsdata.generate_data(n_samples=6, batch_size=batch_size, device=cuda, **KW8)
    assert np.array_equal(got["a"], whole8["a"]) and np.array_equal(got["u"], whole8["u"])
    assert (np.abs(whole8["u"]).max(axis=(1, 2, 3, 4)) > 0).all()


def test_generate_data_slices_concatenate_on_the_device(cuda, whole8):
    from dlwp_benchmark_amd import nsdata
    lo = nsdata.generate_data(n_samples=3, batch_size=3, device=cuda, first_sample=0, **KW8)
    hi = nsdata.generate_data(n_samples=3, batch_size=3, device=cuda, first_sample=3, **KW8)
    assert np.array_equal(np.concatenate((lo["a"], hi["a"])), whole8["a"])
    assert np.array_equal(np.concatenate((lo["u"], hi["u"])), whole8["u"])
    assert hi["attrs"]["first_sample"] == 3 and hi["attrs"]["seed"] == 7 and hi["attrs"]["rng"] == "philox"


def test_results_stay_on_the_device(cuda, monkeypatch):
    from dlwp_benchmark_amd import ddp, nsdata
    from dlwp_benchmark_amd.device_data import DeviceTrajectories
    kw = dict(KW8, max_simulation_time=2, record_steps=8)
    host = nsdata.generate_data(n_samples=6, batch_size=3, device=cuda, **kw)
    dev = nsdata.generate_data(n_samples=6, batch_size=3, device=cuda, to_device=True, **kw)
    assert dev["a"].is_cuda and dev["u"].is_cuda and dev["u"].dtype == torch.float32
    assert np.array_equal(dev["a"].cpu().numpy(), host["a"]) and np.array_equal(dev["u"].cpu().numpy(), host["u"])
    assert np.array_equal(dev["t"], host["t"]) and dev["attrs"] == host["attrs"]

    gen_kw = {k: v for k, v in kw.items() if k not in ("rng", "seed", "solver")}
    returned, plain = [], nsdata.generate_data
    monkeypatch.setattr(nsdata, "generate_data", lambda *a, **k: returned.append(plain(*a, **k)) or returned[-1])
    d = DeviceTrajectories.generate(4, seed=7, device=cuda, n_samples=6, batch_size=3, **gen_kw)
    monkeypatch.undo()
    assert len(returned) == 1 and d.u is returned[0]["u"]                     # wrapped where it lies: no copy
    assert d.u.is_cuda and d.shape == (6, 8, 1, 8, 8) and torch.equal(d.u, dev["u"])
    table = d.epoch_table(0, batch_size=3)
    x, y = d.batch(table[0], 0)
    u_host = d.u.cpu()
    xs, ys = zip(*(ddp.ns_sample(u_host, int(i), 0, 4, 0.0, 7) for i in table[0, :, 0].cpu()))
    assert torch.equal(x.cpu(), torch.stack(xs)) and torch.equal(y.cpu(), torch.stack(ys))
    with pytest.raises(ValueError, match="sets"):
        DeviceTrajectories.generate(4, solver="torch")
