"""2-D incompressible Navier-Stokes data generator, restated on torch.fft and a NetCDF-free format.

Reference: src/nsbench/data/ns_generation/generate_ns_2d.py:27-130 (pseudo-spectral vorticity solver, Crank-Nicolson
for the viscous term, explicit non-linear term with 2/3 dealiasing), random_fields.py:8-64 (Gaussian random field initial
vorticity) and the driver :170-255 (forcing 0.1 (sin(f pi (x+y)) + cos(f pi (x+y))), record every T / record_steps).
The reference is written against the torch-1.6 API (`th.rfft(w0, 2, onesided=False)`, `th.ifft`), which no longer exists;
this restatement uses the full complex FFT for the forward transforms and the half-spectrum C2R transform for the
inverses, which is what the legacy `irfft(..., onesided=False, signal_sizes=...)` computed.  It is a data tool, not part
of the training hot path: it runs on whatever torch device it is given.

Opt-in (docs/kernels/data.md "Navier-Stokes generator"): rng="philox" takes the initial fields from the library's counter-based
normal stream, so a seed names one dataset on every device, in every batch split and slice; solver="kernels" runs the point-wise
work of a GPU time step on the kernels of csrc/ns_solver.hip (navier_stokes_2d_device); to_device=True keeps the result on the GPU.

On-disk format: one `.npz` with `a` [N, s, s] (initial vorticity), `u` [N, T, 1, s, s] (recorded solution), `t` [T] and the
scalar attributes of the reference's NetCDF file (:224-233).  `NavierStokesNpz` mirrors NavierStokesDataset
(data/datasets/datasets.py:11-44): random crop of `sequence_length` frames, x = frames[:-1] (+ noise), y = frames[1:].
"""
import math
import os

import numpy as np
import torch


def _wavenumbers(n, device):
    k_max = n // 2
    k = torch.cat((torch.arange(0, k_max, device=device), torch.arange(-k_max, 0, device=device)), 0)
    k_y = k.repeat(n, 1).to(torch.float64)        # varies along the last axis
    return k_y.transpose(0, 1).contiguous(), k_y, k_max


TAG_GRF = 0x6772                      # Philox counter word 3 of dlwp_ns2d_grf (include/dlwpmi.h: DLWP_NS2D_TAG_GRF)
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # key increments
_MASK32 = np.uint64(0xFFFFFFFF)


def _philox4x32_10(counter, key):
    """Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw, SC'11) in uint64 arithmetic: counter = four words (scalars or arrays of
    one shape), key = two words -> uint64 array [..., 4] of 32-bit words.  csrc/batch_rng.hip.h is the kernels' copy."""
    c = [np.asarray(w, dtype=np.uint64) & _MASK32 for w in np.broadcast_arrays(*counter)]
    k = [np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)]
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c[0], np.uint64(_PHILOX_M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK32]
        k = [(k[0] + np.uint64(_PHILOX_W0)) & _MASK32, (k[1] + np.uint64(_PHILOX_W1)) & _MASK32]
    return np.stack(c, axis=-1)


def philox_normals(seed, item, n, tag=TAG_GRF):
    """The standard normals of the elements 0 .. n-1 of item `item` under the 64-bit `seed` in the library's counter-based stream
    (docs/kernels/data.md), float64: counter (e >> 2, item, 0, tag), key (seed & 0xffffffff, seed >> 32), words w[0..3]; with
    j = e & 3, q = j >> 1: u1 = ((w[2q] >> 8) + 1) 2^-24, u2 = (w[2q+1] >> 8) 2^-24, z = sqrt(-2 ln u1) (cos if j is even else sin)
    (2 pi u2).  The kernels evaluate the same map in fp32; this restatement needs no GPU."""
    seed = int(seed)
    groups = np.arange((n + 3) // 4, dtype=np.uint64)
    w = _philox4x32_10((groups, item, 0, tag), (seed & 0xFFFFFFFF, seed >> 32))
    z = np.empty((len(groups), 4))
    for q in (0, 1):
        u1 = ((w[:, 2 * q] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (w[:, 2 * q + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * q] = r * np.cos(2.0 * np.pi * u2)
        z[:, 2 * q + 1] = r * np.sin(2.0 * np.pi * u2)
    return z.reshape(-1)[:n]


class GaussianRF:
    """random_fields.py:8-64 (dim = 2): samples of N(0, sigma^2 (-Laplace + tau^2)^-alpha) on the periodic unit square.

    rng="torch" (default) draws the coefficients from torch.randn with `generator`: the host and the device generators are
    different streams.  rng="philox" draws them from the library's counter-based stream keyed by `seed`: the coefficient
    z[2 (a n + b)] + i z[2 (a n + b) + 1] of mode (a, b) of global sample s is philox_normals(seed, s, 2 n^2)[...], so a sample
    depends on (seed, s) only -- the same field on the CPU (float64, this file) and on a cuda device (dlwp_ns2d_grf + irfft2,
    fp32), in any batch and from any first_sample."""

    def __init__(self, size, alpha=2.0, tau=3.0, sigma=None, device=None, generator=None, rng="torch", seed=None):
        if rng not in ("torch", "philox"):
            raise ValueError(f"rng must be 'torch' or 'philox', got {rng!r}")
        if rng == "philox":
            if seed is None:
                raise ValueError("rng='philox' needs a seed: the stream is keyed by it")
            if not 0 <= int(seed) < 2 ** 64:
                raise ValueError(f"seed {seed} must fit 64 unsigned bits")
            if size < 4 or size % 2:
                raise ValueError(f"rng='philox' needs an even size of at least 4, got {size}")
            seed = int(seed)
        self.size, self.device, self.generator, self.rng, self.seed = size, device, generator, rng, seed
        if sigma is None:
            sigma = tau ** (0.5 * (2 * alpha - 2))
        self.alpha, self.tau, self.sigma = float(alpha), float(tau), float(sigma)
        self.on_kernel = rng == "philox" and torch.device(device or "cpu").type == "cuda"
        if self.on_kernel:
            return                                     # dlwp_ns2d_grf computes sqrt_eig from the indices: no table
        k_x, k_y, _ = _wavenumbers(size, device)
        self.sqrt_eig = (size ** 2) * math.sqrt(2.0) * sigma * ((4 * math.pi ** 2 * (k_x ** 2 + k_y ** 2) + tau ** 2) ** (-alpha / 2.0))
        self.sqrt_eig[0, 0] = 0.0

    def sample(self, n, first_sample=0):
        """n fields [n, size, size]; first_sample (rng="philox" only): the global index of the first one."""
        if self.rng == "philox":
            return self._sample_philox(int(n), int(first_sample))
        if first_sample != 0:
            raise ValueError("first_sample needs rng='philox': a torch generator has no random access")
        coeff = torch.randn(n, self.size, self.size, 2, device=self.device, generator=self.generator, dtype=torch.float64)
        c = torch.complex(self.sqrt_eig * coeff[..., 0], self.sqrt_eig * coeff[..., 1])
        return torch.fft.ifftn(c, dim=(-2, -1)).real.float()

    def _sample_philox(self, n, first_sample):
        s = self.size
        if n < 1 or first_sample < 0 or first_sample + n > 2 ** 32:
            raise ValueError(f"samples {first_sample} .. {first_sample + n - 1} must be a non-empty range inside [0, 2^32)")
        if self.on_kernel:
            from . import fft
            from . import lib as L
            H = torch.empty(n, 1, s, s // 2 + 1, 2, device=self.device)
            L.check(L.load().dlwp_ns2d_grf(self.seed, first_sample, n, s, self.alpha, self.tau, self.sigma, L.ptr(H), L.stream()))
            return fft.irfft2(H, s, "channels_first", "backward")[:, 0]       # = Re(ifft2(c)): H is c's Hermitian part
        z = np.stack([philox_normals(self.seed, first_sample + i, 2 * s * s, TAG_GRF) for i in range(n)]).reshape(n, s, s, 2)
        coeff = torch.from_numpy(z)
        c = torch.complex(self.sqrt_eig * coeff[..., 0], self.sqrt_eig * coeff[..., 1])
        return torch.fft.ifftn(c, dim=(-2, -1)).real.float()


def _c2r(spec, n):
    """Inverse transform of a full [.., n, n] spectrum the way the legacy C2R did it: from the half spectrum."""
    return torch.fft.irfft2(spec[..., : n // 2 + 1], s=(n, n))


def navier_stokes_2d(w0, f, visc, T, delta_t=1e-4, record_steps=1):
    """w0 [B, n, n] initial vorticity, f [n, n] (or [B, n, n]) forcing -> (sol [B, n, n, record_steps], sol_t)."""
    n = w0.shape[-1]
    dev = w0.device
    steps = math.ceil(T / delta_t)
    w_h = torch.fft.fft2(w0.double())
    f_h = torch.fft.fft2(f.double())
    if f_h.dim() < w_h.dim():
        f_h = f_h.unsqueeze(0)
    record_time = math.floor(steps / record_steps)
    k_x, k_y, k_max = _wavenumbers(n, dev)
    lap = 4 * math.pi ** 2 * (k_x ** 2 + k_y ** 2)
    lap[0, 0] = 1.0
    dealias = ((k_y.abs() <= (2.0 / 3.0) * k_max) & (k_x.abs() <= (2.0 / 3.0) * k_max)).double().unsqueeze(0)
    ikx, iky = 2j * math.pi * k_x, 2j * math.pi * k_y
    sol = torch.zeros(*w0.shape, record_steps, device=dev)
    sol_t = torch.zeros(record_steps, device=dev)
    cn_num, cn_den = 1.0 - 0.5 * delta_t * visc * lap, 1.0 + 0.5 * delta_t * visc * lap
    c, t = 0, 0.0
    for j in range(steps):
        psi_h = w_h / lap                                   # stream function: Poisson equation
        q = _c2r(iky * psi_h, n)                            # u_x =  psi_y
        v = _c2r(-ikx * psi_h, n)                           # u_y = -psi_x
        w_x = _c2r(ikx * w_h, n)
        w_y = _c2r(iky * w_h, n)
        F_h = dealias * torch.fft.fft2(q * w_x + v * w_y)   # non-linear term, 2/3 rule
        w_h = (-delta_t * F_h + delta_t * f_h + cn_num * w_h) / cn_den
        t += delta_t
        if (j + 1) % record_time == 0 and c < record_steps:
            sol[..., c] = _c2r(w_h, n).float()
            sol_t[c] = t
            c += 1
    return sol, sol_t


def navier_stokes_2d_hip(w0, f, visc, T, delta_t=1e-4, record_steps=1):
    """The same solver on the GPU with every transform on libdlwpmi's LDS-staged rFFT2 / irFFT2 kernels (fft.py,
    csrc/fft2d.hip; channels-first, norm "backward") in fp32 -- the precision the reference's torch-1.6 solver ran in.  The
    state is the Hermitian HALF spectrum [B, n, n/2+1]; the four inverse transforms of a step (velocity components and
    vorticity gradients) are one batched call.  The point-wise spectral algebra between the transforms is torch elementwise
    work: this is the data tool of SURVEY.md §8f.2, not the training hot path."""
    from . import fft
    n, dev, B = w0.shape[-1], w0.device, w0.shape[0]
    steps = math.ceil(T / delta_t)

    def r2c(x):                                            # [B, C, n, n] -> complex [B, C, n, n/2+1]
        return torch.view_as_complex(fft.rfft2(x.float().contiguous(), "channels_first", "backward"))

    def c2r(X):
        return fft.irfft2(torch.view_as_real(X).contiguous(), n, "channels_first", "backward")

    w_h = r2c(w0[:, None])[:, 0]
    f_h = r2c((f if f.dim() == 3 else f[None]).float()[:, None].to(dev))[:, 0]
    record_time = math.floor(steps / record_steps)
    k_x, k_y, k_max = _wavenumbers(n, dev)
    k_x, k_y = k_x[:, : n // 2 + 1].float(), k_y[:, : n // 2 + 1].float()
    lap = 4 * math.pi ** 2 * (k_x ** 2 + k_y ** 2)
    lap[0, 0] = 1.0
    dealias = ((k_y.abs() <= (2.0 / 3.0) * k_max) & (k_x.abs() <= (2.0 / 3.0) * k_max)).float().unsqueeze(0)
    ikx, iky = torch.complex(torch.zeros_like(k_x), 2 * math.pi * k_x), torch.complex(torch.zeros_like(k_y), 2 * math.pi * k_y)
    sol = torch.zeros(*w0.shape, record_steps, device=dev)
    sol_t = torch.zeros(record_steps, device=dev)
    cn_num, cn_den = 1.0 - 0.5 * delta_t * visc * lap, 1.0 + 0.5 * delta_t * visc * lap
    c, t = 0, 0.0
    for j in range(steps):
        psi_h = w_h / lap
        fields = c2r(torch.stack((iky * psi_h, -ikx * psi_h, ikx * w_h, iky * w_h), dim=1))     # q, v, w_x, w_y
        F_h = dealias * r2c((fields[:, 0] * fields[:, 2] + fields[:, 1] * fields[:, 3])[:, None])[:, 0]
        w_h = (-delta_t * F_h + delta_t * f_h + cn_num * w_h) / cn_den
        t += delta_t
        if (j + 1) % record_time == 0 and c < record_steps:
            sol[..., c] = c2r(w_h[:, None])[:, 0]
            sol_t[c] = t
            c += 1
    return sol, sol_t


def navier_stokes_2d_device(w0, f, visc, T, delta_t=1e-4, record_steps=1, out=None):
    """The GPU solver with the point-wise work of a step on libdlwpmi's own kernels as well (csrc/ns_solver.hip): a step is
    dlwp_ns2d_spectral_terms -> irFFT2 of the four spectra -> dlwp_ns2d_advect -> rFFT2 -> dlwp_ns2d_cn_update, in fp32, on buffers
    allocated once.  Same arguments and return value as navier_stokes_2d_hip; frames are recorded on the device.  out: an optional
    float32 [B, record_steps, 1, n, n] device tensor (a slice of a dataset's u) to record into; sol is then a view of it."""
    from . import fft
    from . import lib as L
    if not w0.is_cuda:
        raise ValueError("navier_stokes_2d_device needs cuda tensors (navier_stokes_2d is the CPU solver)")
    if w0.dim() != 3 or w0.shape[0] < 1 or w0.shape[1] != w0.shape[2] or w0.shape[2] < 4 or w0.shape[2] % 2:
        raise ValueError(f"w0 must be [B, n, n] with B >= 1 and n even and at least 4, got {tuple(w0.shape)}")
    n, dev, B = w0.shape[-1], w0.device, w0.shape[0]
    steps = math.ceil(T / delta_t)
    record_time = math.floor(steps / record_steps)
    if out is None:
        out = torch.zeros(B, record_steps, 1, n, n, device=dev)
    elif tuple(out.shape) != (B, record_steps, 1, n, n) or out.dtype != torch.float32 or out.device != dev:
        raise ValueError(f"out must be float32 {(B, record_steps, 1, n, n)} on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    fb = (f if f.dim() == 3 else f[None]).float().to(dev).contiguous()
    if tuple(fb.shape) not in ((1, n, n), (B, n, n)):
        raise ValueError(f"f must be [{n}, {n}] or [{B}, {n}, {n}], got {tuple(f.shape)}")
    h, plan, st, wc = L.load(), fft._plan(n, n), L.stream(), n // 2 + 1
    w_h, F_h, f_h = (torch.empty(b, 1, n, wc, 2, device=dev) for b in (B, B, fb.shape[0]))
    terms, work = torch.empty(B, 4, n, wc, 2, device=dev), torch.empty(B, 4, n, wc, 2, device=dev)
    fields, adv, frame = torch.empty(B, 4, n, n, device=dev), torch.empty(B, 1, n, n, device=dev), torch.empty(B, 1, n, n, device=dev)
    x0 = w0.float().contiguous()
    L.check(h.dlwp_rfft2(plan, L.ptr(x0), L.ptr(w_h), B, 1, 1, 0, 0, st))
    L.check(h.dlwp_rfft2(plan, L.ptr(fb), L.ptr(f_h), fb.shape[0], 1, 1, 0, 0, st))
    p_w, p_F, p_f, p_terms, p_work, p_fields, p_adv, p_frame = (L.ptr(t) for t in (w_h, F_h, f_h, terms, work, fields, adv, frame))
    f_batched, dt, nu = int(fb.shape[0] > 1), float(delta_t), float(visc)      # [1, n, n] is one plane: shared, as [n, n]
    ts = [0.0] * record_steps
    c, t = 0, 0.0
    for j in range(steps):
        L.check(h.dlwp_ns2d_spectral_terms(p_w, p_terms, B, n, st))
        L.check(h.dlwp_irfft2(plan, p_terms, p_fields, p_work, B, 4, 1, 0, 0, st))          # q, v, w_x, w_y
        L.check(h.dlwp_ns2d_advect(p_fields, p_adv, B, n, st))
        L.check(h.dlwp_rfft2(plan, p_adv, p_F, B, 1, 1, 0, 0, st))
        L.check(h.dlwp_ns2d_cn_update(p_w, p_F, p_f, f_batched, B, n, dt, nu, st))
        t += delta_t
        if (j + 1) % record_time == 0 and c < record_steps:
            L.check(h.dlwp_irfft2(plan, p_w, p_frame, p_work, B, 1, 1, 0, 0, st))
            out[:, c] = frame
            ts[c] = t
            c += 1
    return out[:, :, 0].permute(0, 2, 3, 1), torch.tensor(ts, dtype=torch.float32, device=dev)


def forcing(resolution, forcing_multiplicator=2.0, device=None):
    t = torch.linspace(0, 1, resolution + 1, device=device, dtype=torch.float64)[:-1]
    X, Y = torch.meshgrid(t, t, indexing="ij")
    return 0.1 * (torch.sin(forcing_multiplicator * math.pi * (X + Y)) + torch.cos(forcing_multiplicator * math.pi * (X + Y)))


def generate_data(resolution=64, n_samples=1000, batch_size=50, max_simulation_time=50, delta_t=1e-3, record_steps=None,
                  viscosity=1e-3, alpha=2.5, tau=7.0, forcing_multiplicator=2.0, device="cpu", seed=None, rng="torch",
                  solver="torch", first_sample=0, to_device=False):
    """generate_ns_2d.generate_data (:170-221) without the NetCDF writer: returns dict(a, u, t, attrs).

    rng="philox" (needs a seed; either device): the initial fields come from the library's counter-based stream, so sample
    first_sample + i is the same field on the CPU and on the GPU, with any batch size, and ranks or sessions can generate disjoint
    slices of one dataset.  solver="kernels" (cuda only): navier_stokes_2d_device instead of navier_stokes_2d_hip.
    to_device=True (cuda only): a and u are returned as device tensors and never pass through host memory.  The defaults keep
    the arithmetic, the random streams and the returned attributes of the plain torch generator."""
    device = torch.device(device)
    if rng not in ("torch", "philox"):
        raise ValueError(f"rng must be 'torch' or 'philox', got {rng!r}")
    if solver not in ("torch", "kernels"):
        raise ValueError(f"solver must be 'torch' or 'kernels', got {solver!r}")
    if rng == "philox" and seed is None:
        raise ValueError("rng='philox' needs a seed: the stream is keyed by it")
    if solver == "kernels" and device.type != "cuda":
        raise ValueError(f"solver='kernels' runs on a cuda device, not on {device}")
    if to_device and device.type != "cuda":
        raise ValueError(f"to_device=True needs a cuda device, not {device}")
    if first_sample != 0 and rng != "philox":
        raise ValueError("first_sample needs rng='philox': a torch generator has no random access")
    record_steps = record_steps or max_simulation_time
    batch_size = min(n_samples, batch_size)
    gen = None
    if seed is not None and rng == "torch":
        gen = torch.Generator(device=device).manual_seed(seed)
    grf = GaussianRF(resolution, alpha=alpha, tau=tau, device=device, generator=gen, rng=rng, seed=seed if rng == "philox" else None)
    f = forcing(resolution, forcing_multiplicator, device)
    a = torch.zeros(n_samples, resolution, resolution, device=device if to_device else None)
    u = torch.zeros(n_samples, record_steps, 1, resolution, resolution, device=device if to_device else None)
    sol_t = None
    for c in range(0, (n_samples // batch_size) * batch_size, batch_size):
        w0 = grf.sample(batch_size, first_sample + c) if rng == "philox" else grf.sample(batch_size)
        if solver == "kernels" and to_device:
            _, sol_t = navier_stokes_2d_device(w0, f, viscosity, max_simulation_time, delta_t, record_steps, out=u[c:c + batch_size])
        else:
            solve = navier_stokes_2d_device if solver == "kernels" else navier_stokes_2d_hip if device.type == "cuda" else navier_stokes_2d
            sol, sol_t = solve(w0, f, viscosity, max_simulation_time, delta_t, record_steps)
            u[c:c + batch_size] = sol.permute(0, 3, 1, 2).unsqueeze(2).to(u.device)
        a[c:c + batch_size] = w0.to(a.device)
    attrs = {"info": "Incompressible Navier-Stokes data", "viscosity": viscosity, "delta_t": "%.e" % delta_t,
             "simulation T": max_simulation_time, "recorded steps": record_steps}
    if rng == "philox":
        attrs.update({"rng": "philox", "seed": int(seed), "first_sample": int(first_sample)})
    if to_device:
        return {"a": a, "u": u, "t": sol_t.cpu().numpy(), "attrs": attrs}
    return {"a": a.numpy(), "u": u.numpy(), "t": sol_t.cpu().numpy(), "attrs": attrs}


def default_name(viscosity, n_samples, T, resolution):
    return f"ns_r{'%.e' % int(1 / viscosity)}_n{n_samples}_t{T}_s{resolution}.npz"   # reference naming (:250), .npz


def save(data, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, a=data["a"], u=data["u"], t=data["t"], **{"attr_" + k.replace(" ", "_"): v for k, v in data["attrs"].items()})


def save_netcdf(data, path):
    """The reference's file layout (generate_ns_2d.py:223-260: coordinates sample / time / dim / height / width, variables a, u, t, the
    attributes) as NetCDF-3 CLASSIC through scipy.io.netcdf_file -- what `xarray.Dataset.to_netcdf` itself writes where the netCDF4
    library is absent, and what `xr.open_dataset` reads back either way.  (NetCDF-4 / HDF5 files need h5py or netCDF4: not in this image.)"""
    from scipy.io import netcdf_file
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    u, a, t = np.asarray(data["u"], dtype=np.float32), np.asarray(data["a"], dtype=np.float32), np.asarray(data["t"], dtype=np.float32)
    dims = dict(zip(("sample", "time", "dim", "height", "width"), u.shape))
    with netcdf_file(path, "w", version=2) as f:          # 64-bit offsets: the 1000-sample files exceed 2 GiB
        for name, n in dims.items():
            f.createDimension(name, n)
            v = f.createVariable(name, "i4", (name,))
            v[:] = np.arange(n, dtype=np.int32)
        f.createVariable("a", "f4", ("sample", "height", "width"))[:] = a
        f.createVariable("u", "f4", tuple(dims))[:] = u
        f.createVariable("t", "f4", ("time",))[:] = t
        for k, val in {"info": "Incompressible Navier-Stokes data", "a": "Initial condition", "u": "Solution", "t": "Time step in simulation",
                       **data.get("attrs", {})}.items():
            if not isinstance(val, (str, bytes)):          # the classic format has no 64-bit integers
                if isinstance(val, (int, np.integer)) and not -2 ** 31 <= int(val) < 2 ** 31:
                    val = str(int(val))                    # a 64-bit seed, a first_sample near 2^32: decimal text, not a truncated int32
                val = np.asarray(val)
                val = val.astype(np.int32) if val.dtype.kind in "iu" else val.astype(np.float64) if val.dtype.kind == "f" else str(val)
            setattr(f, k.replace(" ", "_"), val)


def load_u(data_path):
    """The solution array u [sample, time, dim, height, width] of a data file: .npz (this build's format) or NetCDF-3 classic (.nc)."""
    if str(data_path).endswith(".npz"):
        return np.load(data_path)["u"]
    from scipy.io import netcdf_file
    try:
        with netcdf_file(data_path, "r", mmap=False) as f:
            return np.array(f.variables["u"][:], dtype=np.float32)
    except (TypeError, ValueError) as e:          # scipy: "... is not a valid NetCDF 3 file" for an HDF5-based NetCDF-4 file
        raise OSError(f"{data_path}: only NetCDF-3 classic files can be read in this environment (scipy.io.netcdf_file; NetCDF-4 / HDF5 "
                      f"needs h5py or netCDF4, which the image does not have): {e}") from e


class NavierStokesNpz(torch.utils.data.Dataset):
    """NavierStokesDataset (datasets.py:11-44) on the .npz file or on a NetCDF-3 classic file of the reference's layout (load_u)."""

    def __init__(self, data_path, sequence_length=15, noise=0.0, normalize=False, downscale_factor=None):
        self.u = load_u(data_path)
        self.sequence_length, self.noise, self.normalize = sequence_length, noise, normalize
        self.mean, self.std = self.u.mean(), self.u.std()
        if downscale_factor:
            n, t, d, h, w = self.u.shape
            k = downscale_factor
            self.u = self.u.reshape(n, t, d, h // k, k, w // k, k).mean(axis=(4, 6))

    def __len__(self):
        return self.u.shape[0]

    def __getitem__(self, item):
        r = np.random.randint(0, self.u.shape[1] - self.sequence_length + 1)
        x = np.float32(self.u[item, r:r + self.sequence_length - 1])
        x = x + np.float32(np.random.randn(*x.shape) * self.noise)
        y = np.float32(self.u[item, 1 + r:r + self.sequence_length])
        return x, y


def main():
    import argparse
    ap = argparse.ArgumentParser(description="Incompressible Navier-Stokes data generation (.npz)")
    ap.add_argument("-r", "--resolution", type=int, default=64)
    ap.add_argument("-n", "--n_samples", type=int, default=1000)
    ap.add_argument("-b", "--batch-size", type=int, default=50)
    ap.add_argument("-t", "--max-simulation-time", type=int, default=50)
    ap.add_argument("--delta-t", type=float, default=1e-3)
    ap.add_argument("-s", "--record-steps", type=int, default=None)
    ap.add_argument("-v", "--viscosity", type=float, default=1e-3)
    ap.add_argument("-a", "--alpha", type=float, default=2.0)      # CLI default of the reference (:280)
    ap.add_argument("--tau", type=float, default=7.0)
    ap.add_argument("--forcing-multiplicator", type=float, default=2.0)
    ap.add_argument("-d", "--device", default="cpu")
    ap.add_argument("-p", "--dst-path", default=os.path.join("data", "npz", "navier-stokes"))
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--rng", choices=("torch", "philox"), default="torch",
                    help="philox: the library's counter-based stream (needs --seed); the same dataset on the CPU and on the GPU")
    ap.add_argument("--solver", choices=("torch", "kernels"), default="torch", help="kernels: navier_stokes_2d_device (cuda only)")
    ap.add_argument("--first-sample", type=int, default=0, help="global index of the first generated sample (--rng philox)")
    a = ap.parse_args()
    data = generate_data(a.resolution, a.n_samples, a.batch_size, a.max_simulation_time, a.delta_t, a.record_steps,
                         a.viscosity, a.alpha, a.tau, a.forcing_multiplicator, a.device, a.seed, rng=a.rng, solver=a.solver,
                         first_sample=a.first_sample)
    path = os.path.join(a.dst_path, default_name(a.viscosity, a.n_samples, a.max_simulation_time, a.resolution))
    save(data, path)
    print("wrote", path)


if __name__ == "__main__":
    main()
