"""Float64 numpy restatement of csrc/spectra.hip (helper module for tests/test_spectra_ref.py and tests/test_gpu_spectra.py, not a
conftest): the power per spherical-harmonic degree of fields on the sphere and the shell-binned spectrum of periodic planes, with its
OWN construction of nodes, weights, Legendre functions and shell lists (nothing imported from the package), and with the sums of
absolute terms of its two stages, from which the GPU tests form their bounds.

Conventions (those of dlwp_benchmark_amd/spectra.py): a_lm = sum_k w_k P~_l^m(x_k) (2 pi / W) sum_n f[k, n] exp(-2 pi i m n / W) for
0 <= m < M = min(L, W // 2), P~ orthonormal over the sphere with the Condon-Shortley phase; P_l = (1 / 4 pi) sum_m c_m |a_lm|^2 with
c_0 = 1, c_m = 2.  "midpoint": rows lat_k = -90 + d / 2 + d k (south first) with Fejer's first rule; "legendre-gauss" and
"equiangular" (Clenshaw-Curtis): north first."""
import numpy as np

U24 = 2.0 ** -24


def fejer1(n):
    """theta_j = (j + 1/2) pi / n and the weights of Fejer's first rule on [-1, 1]"""
    theta = (np.arange(n) + 0.5) * np.pi / n
    w = np.empty(n)
    for j in range(n):
        s = sum(np.cos(2 * k * theta[j]) / (4.0 * k * k - 1.0) for k in range(1, n // 2 + 1))
        w[j] = 2.0 / n * (1.0 - 2.0 * s)
    return theta, w


def nodes(H, grid):
    """(x [H] = cos(colatitude) of the rows in the grid's order, w [H])"""
    if grid == "midpoint":
        lat = np.deg2rad(-90.0 + 90.0 / H + np.arange(H) * (180.0 / H))
        theta, w = fejer1(H)                                   # theta ascending = north first; the rows are south first
        return np.sin(lat), w[::-1].copy()
    if grid == "legendre-gauss":
        x, w = np.polynomial.legendre.leggauss(H)
        return x[::-1].copy(), w[::-1].copy()
    if grid == "equiangular":
        theta = np.pi * np.arange(H) / (H - 1)
        w = np.empty(H)
        for j in range(H):
            s = 0.0
            for k in range(1, (H - 1) // 2 + 1):
                s += (1.0 if 2 * k == H - 1 else 2.0) / (4.0 * k * k - 1.0) * np.cos(2 * k * theta[j])
            w[j] = (1.0 if j in (0, H - 1) else 2.0) / (H - 1) * (1.0 - s)
        return np.cos(theta), w
    raise ValueError(grid)


def legendre(M, L, x):
    """P~_l^m(x) [M, L, len(x)], orthonormal over the sphere, Condon-Shortley phase; the standard recurrence in l at fixed m"""
    x = np.asarray(x, dtype=np.float64)
    s = np.sqrt((1.0 - x) * (1.0 + x))
    P = np.zeros((M, L, x.size))
    pmm = np.full(x.size, 1.0 / np.sqrt(4.0 * np.pi))
    for m in range(M):
        if m > 0:
            pmm = -np.sqrt((2.0 * m + 1.0) / (2.0 * m)) * s * pmm
        if m < L:
            P[m, m] = pmm
        if m + 1 < L:
            P[m, m + 1] = np.sqrt(2.0 * m + 3.0) * x * pmm
        for l in range(m + 2, L):
            a = np.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
            b = np.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0))
            P[m, l] = a * (x * P[m, l - 1] - b * P[m, l - 2])
    return P


def tables(H, W, grid, L=None):
    """(F [2 M, W], Wf [M, L, H]) float64"""
    L = H if L is None else L
    M = min(L, W // 2)
    x, w = nodes(H, grid)
    Wf = legendre(M, L, x) * w[None, None, :]
    ang = 2.0 * np.pi * np.outer(np.arange(M), np.arange(W)) / W
    F = np.empty((2 * M, W))
    F[0::2] = 2.0 * np.pi / W * np.cos(ang)
    F[1::2] = -2.0 * np.pi / W * np.sin(ang)
    return F, Wf


def analysis(f, grid, L=None, input_err=0.0):
    """f [..., H, W] -> (a [..., L, M] complex, da [..., L, M, 2]): the coefficients, and for their real and imaginary parts the bound
    on what a fixed-order fp32 evaluation with once-rounded fp32 tables may differ by -- per stage (terms + 2) U24 times the sum of
    absolute terms, plus one rounding per table entry (U24 times the same sum), the first stage's bound carried through the second.
    input_err: a bound on the error of every input value (the HEALPix interpolation)."""
    f = np.asarray(f, dtype=np.float64)
    H, W = f.shape[-2:]
    F, Wf = tables(H, W, grid, L)
    M, L = Wf.shape[:2]
    T = np.einsum("qn,...kn->...kq", F, f)                     # [..., H, 2 M]
    A1 = np.einsum("qn,...kn->...kq", np.abs(F), np.abs(f))
    e1 = (W + 3) * U24 * A1 + input_err * np.abs(F).sum(axis=1)
    T, A1, e1 = (z.reshape(z.shape[:-1] + (M, 2)) for z in (T, A1, e1))
    a = np.einsum("mlk,...kmr->...lmr", Wf, T)
    A2 = np.einsum("mlk,...kmr->...lmr", np.abs(Wf), np.abs(T))
    da = np.einsum("mlk,...kmr->...lmr", np.abs(Wf), e1) + (H + 3) * U24 * A2
    return a[..., 0] + 1j * a[..., 1], da


def synthesis(a, H, W, grid):
    """a [L, M] complex (a[l, m] with m > l ignored, Im a[l, 0] ignored) -> the real field [H, W] with exactly these coefficients"""
    L, M = a.shape
    x, _ = nodes(H, grid)
    P = legendre(M, L, x)
    lon = 2.0 * np.pi * np.arange(W) / W
    f = np.zeros((H, W))
    for m in range(M):
        col = np.einsum("lk,l->k", P[m, m:], a[m:, m]) if m < L else np.zeros(H)
        if m == 0:
            f += col.real[:, None]
        else:
            f += 2.0 * (col.real[:, None] * np.cos(m * lon)[None, :] - col.imag[:, None] * np.sin(m * lon)[None, :])
    return f


def cm(M):
    return np.where(np.arange(M) == 0, 1.0, 2.0)


def power(a, b=None):
    """P_l [..., L] of a, or the cross-spectrum of a and b"""
    b = a if b is None else b
    return (cm(a.shape[-1]) * (a * np.conj(b)).real).sum(axis=-1) / (4.0 * np.pi)


def sphere_spectra(fo, ft, grid, L=None, err_o=0.0, err_t=0.0):
    """fo (or None) / ft [..., H, W] float64 -> power [2, ..., L], cross [..., L], a00 [2, ...] and their bounds (module docstring of
    tests/test_gpu_spectra.py): |dP_l| <= sum_m c_m (2 |a| d + d^2) / 4 pi + (M + 1) U24 P_l per part, the cross term likewise."""
    at, dt = analysis(ft, grid, L, err_t)
    if fo is None:
        ao, do = np.zeros_like(at), np.zeros_like(dt)
    else:
        ao, do = analysis(fo, grid, L, err_o)
    M = at.shape[-1]
    c = cm(M)

    def parts(z):
        return np.stack([np.abs(z.real), np.abs(z.imag)], axis=-1)

    def self_tol(a, d):
        return (c[:, None] * (2.0 * parts(a) * d + d * d)).sum(axis=(-1, -2)) / (4.0 * np.pi) + (M + 1) * U24 * power(a)

    cross_abs = (c[:, None] * parts(ao) * parts(at)).sum(axis=(-1, -2)) / (4.0 * np.pi)
    cross_tol = ((c[:, None] * (parts(ao) * dt + parts(at) * do + do * dt)).sum(axis=(-1, -2)) / (4.0 * np.pi)
                 + (M + 1) * U24 * cross_abs)
    return {"power": np.stack([power(ao), power(at)]), "cross": power(ao, at), "a00": np.stack([ao[..., 0, 0].real, at[..., 0, 0].real]),
            "power_tol": np.stack([self_tol(ao, do), self_tol(at, dt)]), "cross_tol": cross_tol,
            "a00_tol": np.stack([do[..., 0, 0, 0], dt[..., 0, 0, 0]])}


# ---- plane ----------------------------------------------------------------------------------------------------------------------------
def shells(H, W):
    """(shell [H, W // 2 + 1] int, c [H, W // 2 + 1], K): by explicit loops over the half spectrum"""
    Wc = W // 2 + 1
    shell, c = np.zeros((H, Wc), dtype=np.int64), np.zeros((H, Wc))
    for iy in range(H):
        ky = iy if iy < (H + 1) // 2 else iy - H             # (the Nyquist row of an even H: either sign, the same shell)
        for kx in range(Wc):
            shell[iy, kx] = int(np.rint(np.sqrt(float(kx * kx + ky * ky))))
            c[iy, kx] = 1.0 if kx == 0 or 2 * kx == W else 2.0
    return shell, c, int(shell.max()) + 1


def plane_spectra(fo, ft, fft_rtol=1e-5):
    """fo (or None) / ft [..., H, W] float64 -> power [2, ..., K], cross [..., K] and bounds: every component of a half-spectrum entry
    may be off by fft_rtol max|u| of its field (the library's FFT tolerance), carried through
    |dE_k| <= sum c (2 |u| d + d^2) / (H W)^2 + (n_k + 1) U24 E_k with n_k the entries of the shell."""
    ft = np.asarray(ft, dtype=np.float64)
    H, W = ft.shape[-2:]
    shell, c, K = shells(H, W)
    nk = np.bincount(shell.reshape(-1), minlength=K)
    norm = float(H * W) ** 2

    def binned(z):                                             # z [..., H, Wc] real -> [..., K]
        out = np.zeros(z.shape[:-2] + (K,))
        flat = z.reshape(z.shape[:-2] + (-1,))
        for k in range(K):
            out[..., k] = flat[..., shell.reshape(-1) == k].sum(axis=-1)
        return out

    def parts(u):
        return np.abs(u.real), np.abs(u.imag)

    ut = np.fft.rfft2(ft)
    uo = np.zeros_like(ut) if fo is None else np.fft.rfft2(np.asarray(fo, dtype=np.float64))
    dt_ = fft_rtol * np.abs(ut).max(axis=(-1, -2), keepdims=True)
    do_ = fft_rtol * np.abs(uo).max(axis=(-1, -2), keepdims=True)
    res = {"power": np.stack([binned(c * np.abs(uo) ** 2), binned(c * np.abs(ut) ** 2)]) / norm,
           "cross": binned(c * (uo * np.conj(ut)).real) / norm, "K": K}
    tol = []
    for u, d in ((uo, do_), (ut, dt_)):
        r, i = parts(u)
        tol.append(binned(c * (2.0 * (r + i) * d + 2.0 * d * d)) / norm)
    res["power_tol"] = np.stack(tol) + (nk + 1) * U24 * res["power"]
    (ro, io), (rt, it) = parts(uo), parts(ut)
    res["cross_tol"] = (binned(c * ((ro + io) * dt_ + (rt + it) * do_ + 2.0 * do_ * dt_)) / norm
                        + (nk + 1) * U24 * binned(c * (ro * rt + io * it)) / norm)
    return res
