// The point-wise kernels of the 2-D Navier-Stokes data generator (nsdata.py: GaussianRF(rng="philox"), navier_stokes_2d_device;
// docs/kernels/data.md "Navier-Stokes generator").
//
// Reference: the pseudo-spectral vorticity solver of src/nsbench/data/ns_generation/generate_ns_2d.py:27-130 (stream function
// from the Poisson equation, velocity and vorticity gradients by spectral differentiation, explicit non-linear term with the
// 2/3 de-aliasing rule, Crank-Nicolson for the viscous term) and the Gaussian random field of random_fields.py:8-64, as
// nsdata.navier_stokes_2d / nsdata.GaussianRF restate them.  One time step is
//   dlwp_ns2d_spectral_terms -> dlwp_irfft2 (4 channels) -> dlwp_ns2d_advect -> dlwp_rfft2 -> dlwp_ns2d_cn_update
// instead of about twenty torch element-wise launches between the two transforms.
//
// Conventions: complex arrays are interleaved fp32 pairs; the state is the Hermitian half spectrum [B][n][n/2+1] of an n x n
// field, n even.  Index a stands for the wavenumber a (a < n/2) or a - n, so the Nyquist row and column carry -n/2: the
// reference's cat(arange(0, k_max), arange(-k_max, 0)), of which the half spectrum is the slice [:, : n/2+1].  k_x runs along
// the rows, k_y along the columns.  Everything is computed from the indices: no tables, no atomics, no LDS, and every output
// element has exactly one writer whose arithmetic depends on that element's own sample and indices only -- a launch gives the
// same bits whatever the batch size, the position in the batch or the alignment of the pointers.  The build contracts a
// multiply that feeds an add into a fused multiply-add wherever it finds one (-ffp-contract=fast), so every such pair below is
// written as fmaf by hand, and a mode that is its own mirror gets its zero imaginary part by index, not from z - z (fused with
// the product inside dlwp_noise4, that difference would be the product's rounding error).
//
// Shape: bandwidth- and launch-bound.  256 threads, a grid-stride loop, one PAIR of neighbouring complex elements per
// iteration: n (n/2+1) is even, so the linear indices 2p, 2p+1 lie in the same sample, and where the array is 16-byte aligned
// the pair is one 16-byte access (n/2+1 is odd: the pairing goes by linear index, not by row).  Arrays that are only 8-byte
// aligned (a slice that begins at an odd plane) take two 8-byte accesses per pair with the same arithmetic.
#include "common.hip.h"
#include "dlwpmi_internal.h"
#include "batch_rng.hip.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int MAX_WGS = 2048;                         // about eight workgroups per CU, the rest by striding
constexpr float TWO_PI = 6.283185307179586f;
constexpr float FOUR_PI2 = 39.47841760435743f;        // 4 pi^2

struct Shape {
    int n, Wc, plane, total;                          // Wc = n/2+1, plane = n Wc, total = B plane complex elements
};

struct Mode {
    int i, a, b, rem;                                 // sample, row, column, a Wc + b
    float kx, ky, k2, lap;                            // signed wavenumbers, |k|^2, 4 pi^2 |k|^2 with lap(0, 0) = 1
    bool keep;                                        // inside the 2/3 box: 3 |k_x| <= n and 3 |k_y| <= n
};

__device__ __forceinline__ Mode mode_of(int idx, const Shape& s) {
    Mode m;
    m.i = (int)((unsigned)idx / (unsigned)s.plane);
    m.rem = idx - m.i * s.plane;
    m.a = (int)((unsigned)m.rem / (unsigned)s.Wc);
    m.b = m.rem - m.a * s.Wc;
    const int kx = 2 * m.a < s.n ? m.a : m.a - s.n, ky = 2 * m.b < s.n ? m.b : m.b - s.n;
    m.kx = (float)kx, m.ky = (float)ky;
    m.k2 = (float)(kx * kx + ky * ky);                // <= n^2 / 2: exact in fp32 up to n = 4096
    m.lap = (kx | ky) ? FOUR_PI2 * m.k2 : 1.0f;
    m.keep = 3 * abs(kx) <= s.n && 3 * abs(ky) <= s.n;
    return m;
}

// the complex elements 2p, 2p+1 of an array
template <bool VEC>
__device__ __forceinline__ void load_pair(const float* src, int p, float2& v0, float2& v1) {
    if constexpr (VEC) {
        const float4 v = reinterpret_cast<const float4*>(src)[p];
        v0 = make_float2(v.x, v.y), v1 = make_float2(v.z, v.w);
    } else {
        v0 = reinterpret_cast<const float2*>(src)[2 * p], v1 = reinterpret_cast<const float2*>(src)[2 * p + 1];
    }
}
template <bool VEC>
__device__ __forceinline__ void store_pair(float* dst, int p, const float2 v0, const float2 v1) {
    if constexpr (VEC) {
        reinterpret_cast<float4*>(dst)[p] = make_float4(v0.x, v0.y, v1.x, v1.y);
    } else {
        reinterpret_cast<float2*>(dst)[2 * p] = v0, reinterpret_cast<float2*>(dst)[2 * p + 1] = v1;
    }
}

// ---- initial vorticity
struct GrfArgs {
    float* H;
    Shape s;
    uint32_t k0, k1, first;                           // key = the two halves of the seed; first sample (mod 2^32)
    float coef, tau2, mhalf_alpha;                    // n^2 sqrt(2) sigma, tau^2, -alpha / 2
};

// the complex normal of full-spectrum element (a, b) of a sample: elements 2 (a n + b), 2 (a n + b) + 1 of its stream, i.e. one
// half of the Philox group (a n + b) >> 1
__device__ __forceinline__ float2 grf_normal(const GrfArgs& g, uint32_t sample, int a, int b) {
    const int c = a * g.s.n + b;
    float z[4];
    dlwp_noise4((uint32_t)(c >> 1), sample, 0u, DLWP_NS2D_TAG_GRF, g.k0, g.k1, z);
    return (c & 1) ? make_float2(z[2], z[3]) : make_float2(z[0], z[1]);
}

__device__ __forceinline__ float2 grf_elem(const GrfArgs& g, int idx) {
    const Mode m = mode_of(idx, g.s);
    if ((m.a | m.b) == 0) return make_float2(0.f, 0.f);                   // sqrt_eig[0][0] = 0
    // sqrt_eig is even in both indices: one value for c and its mirror
    const float se = g.coef * powf(fmaf(FOUR_PI2, m.k2, g.tau2), g.mhalf_alpha);
    const uint32_t sample = g.first + (uint32_t)m.i;
    const float2 z = grf_normal(g, sample, m.a, m.b);
    const int ma = m.a ? g.s.n - m.a : 0, mb = m.b ? g.s.n - m.b : 0;
    if (ma == m.a && mb == m.b) return make_float2(se * z.x, 0.f);      // its own mirror: (c + conj(c)) / 2 is real
    const float2 zm = grf_normal(g, sample, ma, mb);
    const float h = 0.5f * se;
    return make_float2(h * (z.x + zm.x), h * (z.y - zm.y));
}

template <bool VEC>
__global__ __launch_bounds__(256) void ns2d_grf_kernel(const GrfArgs g) {
    const int pairs = g.s.total >> 1;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < pairs; p += gridDim.x * 256)
        store_pair<VEC>(g.H, p, grf_elem(g, 2 * p), grf_elem(g, 2 * p + 1));
}

// ---- spectra of the velocity components and the vorticity gradients
struct TermsArgs {
    const float* w;
    float* out;
    Shape s;
};

// (0 + i s) (re + i im)
__device__ __forceinline__ float2 times_i(float s, const float2 v) { return make_float2(-(s * v.y), s * v.x); }

__device__ __forceinline__ void terms_elem(const Mode& m, const float2 w, float2 t[4]) {
    const float2 psi = make_float2(w.x / m.lap, w.y / m.lap);
    const float sx = TWO_PI * m.kx, sy = TWO_PI * m.ky;
    t[0] = times_i(sy, psi);                          // q   = psi_y
    t[1] = times_i(-sx, psi);                         // v   = -psi_x
    t[2] = times_i(sx, w);                            // w_x
    t[3] = times_i(sy, w);                            // w_y
}

template <bool VEC>
__global__ __launch_bounds__(256) void ns2d_spectral_terms_kernel(const TermsArgs g) {
    const int pairs = g.s.total >> 1, half_plane = g.s.plane >> 1;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < pairs; p += gridDim.x * 256) {
        float2 w0, w1, t0[4], t1[4];
        load_pair<VEC>(g.w, p, w0, w1);
        const Mode m0 = mode_of(2 * p, g.s), m1 = mode_of(2 * p + 1, g.s);
        terms_elem(m0, w0, t0);
        terms_elem(m1, w1, t1);
        const int po = p + 3 * m0.i * half_plane;     // pair index of (sample i, channel 0) in [B][4][plane]
#pragma unroll
        for (int c = 0; c < 4; ++c) store_pair<VEC>(g.out, po + c * half_plane, t0[c], t1[c]);
    }
}

// ---- non-linear term in physical space
struct AdvectArgs {
    const float* fields;
    float* out;
    int nn, total;                                    // n^2 (a multiple of 4), B n^2
};

template <bool VEC>
__global__ __launch_bounds__(256) void ns2d_advect_kernel(const AdvectArgs g) {
    if constexpr (VEC) {
        const int quads = g.total >> 2, qn = g.nn >> 2;
        const float4* f = reinterpret_cast<const float4*>(g.fields);
        for (int p = blockIdx.x * 256 + threadIdx.x; p < quads; p += gridDim.x * 256) {
            const int i = (int)((unsigned)p / (unsigned)qn), src = p + 3 * i * qn;
            const float4 q = f[src], v = f[src + qn], wx = f[src + 2 * qn], wy = f[src + 3 * qn];
            reinterpret_cast<float4*>(g.out)[p] = make_float4(fmaf(q.x, wx.x, v.x * wy.x), fmaf(q.y, wx.y, v.y * wy.y),
                                                              fmaf(q.z, wx.z, v.z * wy.z), fmaf(q.w, wx.w, v.w * wy.w));
        }
    } else {
        for (int e = blockIdx.x * 256 + threadIdx.x; e < g.total; e += gridDim.x * 256) {
            const int i = (int)((unsigned)e / (unsigned)g.nn), src = e + 3 * i * g.nn;
            g.out[e] = fmaf(g.fields[src], g.fields[src + 2 * g.nn], g.fields[src + g.nn] * g.fields[src + 3 * g.nn]);
        }
    }
}

// ---- de-aliasing and the Crank-Nicolson update
struct CnArgs {
    float* w;
    const float *F, *f;
    Shape s;
    int f_batched;
    float dt, half_dt_visc;
};

__device__ __forceinline__ float2 cn_elem(const CnArgs& g, const Mode& m, const float2 w, const float2 F, const float2 f) {
    const float num = fmaf(-g.half_dt_visc, m.lap, 1.0f), den = fmaf(g.half_dt_visc, m.lap, 1.0f);
    const float2 Fd = m.keep ? F : make_float2(0.f, 0.f);
    return make_float2(fmaf(num, w.x, fmaf(g.dt, f.x, -(g.dt * Fd.x))) / den, fmaf(num, w.y, fmaf(g.dt, f.y, -(g.dt * Fd.y))) / den);
}

template <bool VEC>
__global__ __launch_bounds__(256) void ns2d_cn_update_kernel(const CnArgs g) {
    const int pairs = g.s.total >> 1, half_plane = g.s.plane >> 1;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < pairs; p += gridDim.x * 256) {
        const Mode m0 = mode_of(2 * p, g.s), m1 = mode_of(2 * p + 1, g.s);
        float2 w0, w1, F0, F1, f0, f1;
        load_pair<VEC>(g.w, p, w0, w1);
        load_pair<VEC>(g.F, p, F0, F1);
        load_pair<VEC>(g.f, g.f_batched ? p : p - m0.i * half_plane, f0, f1);
        store_pair<VEC>(g.w, p, cn_elem(g, m0, w0, F0, f0), cn_elem(g, m1, w1, F1, f1));
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

unsigned grid_for(long long items) { return (unsigned)std::max<long long>(1, std::min<long long>((items + 255) / 256, MAX_WGS)); }

// B and n of every entry point; fills the shape
int check_shape(const char* who, int B, int n, Shape* s) {
    DLWP_REQUIRE(B >= 1, DLWP_E_INVALID, "%s: B %d must be at least 1", who, B);
    DLWP_REQUIRE(n >= 4 && n % 2 == 0, DLWP_E_INVALID, "%s: n %d must be even and at least 4", who, n);
    DLWP_REQUIRE(n <= 4096, DLWP_E_UNSUPPORTED, "%s: n %d is above 4096 (the squared wavenumbers are kept exactly in fp32)", who, n);
    const long long plane = (long long)n * (n / 2 + 1);
    DLWP_REQUIRE((long long)B * plane <= INT_MAX / 4 && (long long)B * n * n <= INT_MAX / 4, DLWP_E_UNSUPPORTED,
                 "%s: B %d x n %d is too large for the 32-bit element indices of one launch", who, B, n);
    s->n = n, s->Wc = n / 2 + 1, s->plane = (int)plane, s->total = (int)(B * plane);
    return DLWP_OK;
}

}  // namespace

extern "C" int dlwp_ns2d_grf(unsigned long long seed, long long first_sample, int B, int n, float alpha, float tau, float sigma,
                             float* H, void* stream) {
    DLWP_REQUIRE(H, DLWP_E_INVALID, "ns2d_grf: H is NULL");
    GrfArgs g;
    if (int rc = check_shape("ns2d_grf", B, n, &g.s)) return rc;
    DLWP_REQUIRE(first_sample >= 0 && first_sample + B <= (1LL << 32), DLWP_E_INVALID,
                 "ns2d_grf: first_sample %lld + B %d must lie in [0, 2^32] (the sample is one counter word)", first_sample, B);
    DLWP_REQUIRE(std::isfinite(alpha), DLWP_E_INVALID, "ns2d_grf: alpha %g must be finite", (double)alpha);
    DLWP_REQUIRE(std::isfinite(tau), DLWP_E_INVALID, "ns2d_grf: tau %g must be finite", (double)tau);
    DLWP_REQUIRE(std::isfinite(sigma), DLWP_E_INVALID, "ns2d_grf: sigma %g must be finite", (double)sigma);
    DLWP_REQUIRE(aligned(H, 8), DLWP_E_INVALID, "ns2d_grf: H must be 8-byte aligned");
    g.H = H;
    g.k0 = (uint32_t)(seed & 0xffffffffull), g.k1 = (uint32_t)(seed >> 32), g.first = (uint32_t)first_sample;
    g.coef = (float)((double)n * n * std::sqrt(2.0) * (double)sigma), g.tau2 = tau * tau, g.mhalf_alpha = -0.5f * alpha;
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 8.0 * g.s.total, "ns2d_grf");
    const unsigned grid = grid_for(g.s.total / 2);
    if (aligned(H, 16)) hipLaunchKernelGGL(ns2d_grf_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(ns2d_grf_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, g);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_ns2d_spectral_terms(const float* w_h, float* out, int B, int n, void* stream) {
    DLWP_REQUIRE(w_h, DLWP_E_INVALID, "ns2d_spectral_terms: w_h is NULL");
    DLWP_REQUIRE(out, DLWP_E_INVALID, "ns2d_spectral_terms: out is NULL");
    TermsArgs g;
    if (int rc = check_shape("ns2d_spectral_terms", B, n, &g.s)) return rc;
    DLWP_REQUIRE(aligned(w_h, 8) && aligned(out, 8), DLWP_E_INVALID, "ns2d_spectral_terms: w_h and out must be 8-byte aligned");
    g.w = w_h, g.out = out;
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 40.0 * g.s.total, "ns2d_spectral_terms");
    const unsigned grid = grid_for(g.s.total / 2);
    if (aligned(w_h, 16) && aligned(out, 16))
        hipLaunchKernelGGL(ns2d_spectral_terms_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(ns2d_spectral_terms_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, g);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_ns2d_advect(const float* fields, float* out, int B, int n, void* stream) {
    DLWP_REQUIRE(fields, DLWP_E_INVALID, "ns2d_advect: fields is NULL");
    DLWP_REQUIRE(out, DLWP_E_INVALID, "ns2d_advect: out is NULL");
    Shape s;
    if (int rc = check_shape("ns2d_advect", B, n, &s)) return rc;
    AdvectArgs g;
    g.fields = fields, g.out = out, g.nn = n * n, g.total = B * n * n;
    dlwp_prof_scope prof((hipStream_t)stream, 3.0 * g.total, 20.0 * g.total, "ns2d_advect");
    if (aligned(fields, 16) && aligned(out, 16))
        hipLaunchKernelGGL(ns2d_advect_kernel<true>, dim3(grid_for(g.total / 4)), dim3(256), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(ns2d_advect_kernel<false>, dim3(grid_for(g.total)), dim3(256), 0, (hipStream_t)stream, g);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_ns2d_cn_update(float* w_h, const float* F_h, const float* f_h, int f_batched, int B, int n, float dt,
                                   float visc, void* stream) {
    DLWP_REQUIRE(w_h, DLWP_E_INVALID, "ns2d_cn_update: w_h is NULL");
    DLWP_REQUIRE(F_h, DLWP_E_INVALID, "ns2d_cn_update: F_h is NULL");
    DLWP_REQUIRE(f_h, DLWP_E_INVALID, "ns2d_cn_update: f_h is NULL");
    CnArgs g;
    if (int rc = check_shape("ns2d_cn_update", B, n, &g.s)) return rc;
    DLWP_REQUIRE(dt > 0.f && dt < INFINITY, DLWP_E_INVALID, "ns2d_cn_update: dt %g must be finite and positive", (double)dt);
    DLWP_REQUIRE(visc >= 0.f && visc < INFINITY, DLWP_E_INVALID, "ns2d_cn_update: visc %g must be finite and not negative", (double)visc);
    DLWP_REQUIRE(aligned(w_h, 8) && aligned(F_h, 8) && aligned(f_h, 8), DLWP_E_INVALID,
                 "ns2d_cn_update: w_h, F_h and f_h must be 8-byte aligned");
    g.w = w_h, g.F = F_h, g.f = f_h, g.f_batched = f_batched != 0, g.dt = dt, g.half_dt_visc = (float)(0.5 * (double)dt * (double)visc);
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 8.0 * g.s.total * (g.f_batched ? 4.0 : 3.0), "ns2d_cn_update");
    const unsigned grid = grid_for(g.s.total / 2);
    if (aligned(w_h, 16) && aligned(F_h, 16) && aligned(f_h, 16))
        hipLaunchKernelGGL(ns2d_cn_update_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(ns2d_cn_update_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, g);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}
