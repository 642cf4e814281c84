"""The seeded Navier-Stokes generator without a GPU: nsdata.philox_normals against the reference of the stream
(tests/batch_ref.py), GaussianRF(rng="philox") against a spelled-out float64 field, and generate_data(rng="philox") across batch
sizes and first_sample slices; the default call (rng="torch") against GaussianRF + navier_stokes_2d run by hand."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_ref  # noqa: E402

from dlwp_benchmark_amd import nsdata  # noqa: E402

TAG = 0x6772
KW = dict(resolution=8, n_samples=6, max_simulation_time=1, delta_t=1e-2)


def test_tag_is_the_documented_one():
    assert nsdata.TAG_GRF == TAG and TAG not in (batch_ref.TAG_NS, batch_ref.TAG_WB)


@pytest.mark.parametrize("seed", [7, 2 ** 32 + 12345])
@pytest.mark.parametrize("n", [1, 5, 8, 2 * 12 * 12])
def test_philox_normals_restate_the_stream(seed, n):
    """The package's restatement and tests/batch_ref.py are the same text by design (the issue asks for a copy the package can use
    without its tests): this pins the two copies to each other -- counter layout, key halves, tag, truncation to n -- and is NOT
    independent evidence for the stream.  That comes from tests/test_batch_ref.py (published Philox known answers) and from
    tests/test_gpu_ns_solver.py, where the kernel's own fp32 evaluation meets the float64 spectrum."""
    for item in (0, 3, 2 ** 32 - 1):
        got = nsdata.philox_normals(seed, item, n, TAG)
        assert got.dtype == np.float64 and got.shape == (n,)
        assert np.array_equal(got, batch_ref.normals(seed, 0, item, n, TAG))
    assert np.array_equal(nsdata.philox_normals(seed, 1, n, batch_ref.TAG_NS), batch_ref.normals(seed, 0, 1, n, batch_ref.TAG_NS))


def spelled_out_field(n, seed, sample, alpha, tau):
    """Re(ifft2(c)) in float64 numpy with c[a, b] = sqrt_eig[a, b] (z[2 (a n + b)] + i z[2 (a n + b) + 1]) from batch_ref.normals."""
    k = np.concatenate((np.arange(0, n // 2), np.arange(-(n // 2), 0))).astype(np.float64)
    kx, ky = k[:, None], k[None, :]
    sigma = tau ** (0.5 * (2 * alpha - 2))
    sqrt_eig = n ** 2 * math.sqrt(2.0) * sigma * (4 * math.pi ** 2 * (kx ** 2 + ky ** 2) + tau ** 2) ** (-alpha / 2.0)
    sqrt_eig[0, 0] = 0.0
    z = batch_ref.normals(seed, 0, sample, 2 * n * n, TAG)
    c = np.empty((n, n), dtype=np.complex128)
    for a in range(n):
        for b in range(n):
            c[a, b] = sqrt_eig[a, b] * complex(z[2 * (a * n + b)], z[2 * (a * n + b) + 1])
    return np.fft.ifft2(c).real


@pytest.mark.parametrize("seed", [11, 2 ** 40 + 1])
def test_cpu_initial_conditions(seed):
    n, alpha, tau = 8, 2.5, 7.0
    got = nsdata.GaussianRF(n, alpha=alpha, tau=tau, rng="philox", seed=seed, device="cpu").sample(3)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, n, n)
    for i in range(3):
        ref = spelled_out_field(n, seed, i, alpha, tau)
        # the result is the float32 rounding of a float64 field (two FFT libraries: 1e-13 relative apart)
        assert np.abs(got[i].double().numpy() - ref).max() <= 2.0 ** -23 * np.abs(ref).max()


def test_first_sample_slices_of_the_initial_conditions():
    grf = nsdata.GaussianRF(8, rng="philox", seed=3, device="cpu")
    assert torch.equal(grf.sample(3, first_sample=2), grf.sample(5)[2:5])
    other = nsdata.GaussianRF(8, rng="philox", seed=4, device="cpu").sample(5)
    assert not torch.equal(other, grf.sample(5))


@pytest.fixture(scope="module")
def whole():
    return nsdata.generate_data(batch_size=6, rng="philox", seed=7, device="cpu", **KW)


@pytest.mark.parametrize("batch_size", [2, 3])
def test_generate_data_does_not_depend_on_the_batch_size(whole, batch_size):
    got = nsdata.generate_data(batch_size=batch_size, rng="philox", seed=7, device="cpu", **KW)
    assert np.array_equal(got["a"], whole["a"]) and np.array_equal(got["u"], whole["u"]) and np.array_equal(got["t"], whole["t"])
    assert (np.abs(whole["u"]).max(axis=(1, 2, 3, 4)) > 0).all()          # every sample was generated


def test_generate_data_slices_concatenate(whole):
    kw = dict(KW, n_samples=3)
    lo = nsdata.generate_data(batch_size=3, rng="philox", seed=7, device="cpu", first_sample=0, **kw)
    hi = nsdata.generate_data(batch_size=3, rng="philox", seed=7, device="cpu", first_sample=3, **kw)
    assert np.array_equal(np.concatenate((lo["a"], hi["a"])), whole["a"])
    assert np.array_equal(np.concatenate((lo["u"], hi["u"])), whole["u"])
    assert hi["attrs"]["rng"] == "philox" and hi["attrs"]["seed"] == 7 and hi["attrs"]["first_sample"] == 3
    assert whole["attrs"]["first_sample"] == 0


def test_default_call_is_the_torch_generator_run_by_hand():
    got = nsdata.generate_data(batch_size=3, seed=5, **KW)
    gen = torch.Generator().manual_seed(5)
    grf = nsdata.GaussianRF(8, alpha=2.5, tau=7.0, device=torch.device("cpu"), generator=gen)
    f = nsdata.forcing(8, 2.0, torch.device("cpu"))
    for c in (0, 3):
        w0 = grf.sample(3)
        sol, sol_t = nsdata.navier_stokes_2d(w0, f, 1e-3, 1, 1e-2, 1)
        assert np.array_equal(got["a"][c:c + 3], w0.numpy())
        assert np.array_equal(got["u"][c:c + 3], sol.permute(0, 3, 1, 2).unsqueeze(2).numpy())
    assert np.array_equal(got["t"], sol_t.numpy())
    assert set(got) == {"a", "u", "t", "attrs"}
    assert got["attrs"] == {"info": "Incompressible Navier-Stokes data", "viscosity": 1e-3, "delta_t": "1e-02", "simulation T": 1,
                            "recorded steps": 1}


def test_netcdf_attributes_name_the_dataset(tmp_path):
    """the classic format has no 64-bit integers: a seed or first_sample that does not fit int32 is written as decimal text"""
    from scipy.io import netcdf_file
    kw = dict(KW, n_samples=2)
    for seed, first in ((7, 3), (2 ** 40 + 9, 2 ** 32 - 2)):
        data = nsdata.generate_data(batch_size=2, rng="philox", seed=seed, first_sample=first, device="cpu", **kw)
        path = str(tmp_path / f"s{seed}.nc")
        nsdata.save_netcdf(data, path)
        with netcdf_file(path, "r", mmap=False) as f:
            got = {k: getattr(f, k) for k in ("rng", "seed", "first_sample")}
        as_int = {k: int(v.decode() if isinstance(v, bytes) else v) for k, v in got.items() if k != "rng"}
        assert as_int == {"seed": seed, "first_sample": first} and got["rng"] in (b"philox", "philox")
        assert np.array_equal(nsdata.load_u(path), data["u"])


def test_refusals():
    with pytest.raises(ValueError, match="seed"):
        nsdata.GaussianRF(8, rng="philox")
    with pytest.raises(ValueError, match="seed"):
        nsdata.generate_data(rng="philox", device="cpu", **KW)
    with pytest.raises(ValueError, match="kernels"):
        nsdata.generate_data(solver="kernels", device="cpu", rng="philox", seed=1, **KW)
    with pytest.raises(ValueError, match="to_device"):
        nsdata.generate_data(to_device=True, device="cpu", **KW)
    with pytest.raises(ValueError, match="first_sample"):
        nsdata.generate_data(first_sample=2, seed=1, device="cpu", **KW)
    with pytest.raises(ValueError, match="rng"):
        nsdata.generate_data(rng="numpy", device="cpu", **KW)
    with pytest.raises(ValueError, match="cuda"):
        nsdata.navier_stokes_2d_device(torch.zeros(1, 8, 8), torch.zeros(8, 8), 1e-3, 1, 1e-2)
