// Training batches assembled on the device from resident datasets: one launch per batch instead of per-sample host slicing,
// stacking and host-to-device copies (docs/kernels/data.md).
//
// Reference: NavierStokesDataset.__getitem__ (src/nsbench/data/datasets/datasets.py:39-44: x = u[i, r : r+L-1] + noise,
// y = u[i, r+1 : r+L]) as ddp.ns_sample restates it, and the training branch of WeatherBenchDataset.__getitem__
// (src/dlwpbench/data/datasets/datasets.py:335-395: z-score per variable, target = prognostic[1:][context:], noise on
// prognostic[:-1]) as wbdata.WeatherBenchArrays restates it, followed by the default collate (to_device_batch).
//
// Both kernels are data movement: no atomics, no LDS, every output address has one writer, so two calls give the same bits.
// The unit of work is one SOURCE plane (a frame of a trajectory, one frame of one WeatherBench channel): a workgroup row
// (blockIdx.x) owns it, reads it once and writes it to the one or two outputs it belongs to -- the frames r+1 .. r+L-2 of a
// Navier-Stokes window go to x and y, a prognostic frame to `prognostic` and `target`.  blockIdx.y strides over the plane in
// pieces of 256 lanes x 16 bytes (consecutive lanes, consecutive addresses); planes whose float count is no multiple of 4, or
// whose pointers are not 16-byte aligned, take the scalar form of the same loop.  The grid is capped near 2048 workgroups
// (eight per CU) and strides the rest.
//
// Row guard: the table rows are validated on the host before they are uploaded (device_data.py); a row that is out of range
// all the same (sample index, crop window or item outside the resident data, a NULL series) writes nothing and reads nothing.
//
// Noise: batch_rng.hip.h.  The counter is (element >> 2, item, epoch, tag) with the element index taken inside ONE sample's
// noisy tensor, so the perturbation of a sample does not depend on its position in the batch, on the other samples or on the
// number of ranks.  With noise == 0 the generator is not touched: the outputs are exact copies / normalisations.
#include "common.hip.h"
#include "dlwpmi_internal.h"
#include "batch_rng.hip.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int TARGET_WGS = 2048;      // memory-bound copy: about eight workgroups per CU, the rest by striding

struct Rng {
    float noise;                      // 0: the generator is not touched
    uint32_t k0, k1, epoch, tag;
};

// one source plane of n floats -> d0 (nullable; + noise z when noisy) and d1 (nullable; never perturbed).
// e0: index of the plane's first element inside the sample's noisy tensor (a multiple of 4 in the vector form)
template <bool VEC>
__device__ __forceinline__ void move_plane(const float* __restrict__ src, float* __restrict__ d0, float* __restrict__ d1,
                                           long long n, bool norm, float mean, float sd, bool noisy, long long e0,
                                           uint32_t item, const Rng& g) {
    const long long count = VEC ? n >> 2 : n;
    for (long long p = (long long)blockIdx.y * 256 + threadIdx.x; p < count; p += (long long)gridDim.y * 256) {
        if constexpr (VEC) {
            float4 v = reinterpret_cast<const float4*>(src)[p];
            if (norm) {
                v.x = __fdiv_rn(v.x - mean, sd), v.y = __fdiv_rn(v.y - mean, sd);
                v.z = __fdiv_rn(v.z - mean, sd), v.w = __fdiv_rn(v.w - mean, sd);
            }
            if (d1) reinterpret_cast<float4*>(d1)[p] = v;
            if (d0) {
                if (noisy) {
                    float z[4];
                    dlwp_noise4((uint32_t)((e0 >> 2) + p), item, g.epoch, g.tag, g.k0, g.k1, z);
                    v.x = fmaf(g.noise, z[0], v.x), v.y = fmaf(g.noise, z[1], v.y);
                    v.z = fmaf(g.noise, z[2], v.z), v.w = fmaf(g.noise, z[3], v.w);
                }
                reinterpret_cast<float4*>(d0)[p] = v;
            }
        } else {
            float v = src[p];
            if (norm) v = __fdiv_rn(v - mean, sd);
            if (d1) d1[p] = v;
            if (d0) {
                if (noisy) {
                    const long long e = e0 + p;
                    const int j = (int)(e & 3);
                    float z[4];
                    dlwp_noise4((uint32_t)(e >> 2), item, g.epoch, g.tag, g.k0, g.k1, z);
                    v = fmaf(g.noise, j == 0 ? z[0] : j == 1 ? z[1] : j == 2 ? z[2] : z[3], v);
                }
                d0[p] = v;
            }
        }
    }
}

struct NsArgs {
    const float* u;
    const int* table;
    float *x, *y;
    long long F;
    int N, T, L, vec;
    Rng rng;
};

// blockIdx.x = b L + k: source frame r + k of window b
__global__ __launch_bounds__(256) void ns_batch_kernel(const NsArgs a) {
    const int b = blockIdx.x / a.L, k = blockIdx.x - b * a.L;
    const int i = a.table[2 * b], r = a.table[2 * b + 1];
    if (i < 0 || i >= a.N || r < 0 || r > a.T - a.L) return;      // row guard (workgroup-uniform)
    const float* src = a.u + ((long long)i * a.T + r + k) * a.F;
    const long long row = (long long)b * (a.L - 1);
    float* dx = k < a.L - 1 ? a.x + (row + k) * a.F : nullptr;
    float* dy = k >= 1 ? a.y + (row + k - 1) * a.F : nullptr;
    const bool noisy = a.rng.noise > 0.f;
    if (a.vec) move_plane<true>(src, dx, dy, a.F, false, 0.f, 1.f, noisy, (long long)k * a.F, (uint32_t)i, a.rng);
    else move_plane<false>(src, dx, dy, a.F, false, 0.f, 1.f, noisy, (long long)k * a.F, (uint32_t)i, a.rng);
}

struct WbArgs {
    const dlwp_wb_channel* chan;
    const int* items;
    float *constants, *prescribed, *prognostic, *target;
    long long P;
    int nC, nP, nG, L, context, n_time, planes, out_vec;
    Rng rng;
};

// blockIdx.x = b planes + s: the nC constant planes, then the L nP prescribed planes (frame-major), then the (L + 1) nG
// prognostic planes (frame-major) of sample b
__global__ __launch_bounds__(256) void wb_batch_kernel(const WbArgs a) {
    const int b = blockIdx.x / a.planes;
    int s = blockIdx.x - b * a.planes;
    const int item = a.items[b];
    const long long t0 = (long long)item * a.L;
    if (item < 0 || t0 + a.L + 1 > a.n_time) return;             // row guard (workgroup-uniform)
    float *d0, *d1 = nullptr;
    long long frame = 0, e0 = 0;                                  // source frame of the channel's series (constants: the one plane)
    bool noisy = false;
    int c;
    if (s < a.nC) {
        c = s;
        d0 = a.constants + ((long long)b * a.nC + s) * a.P;
    } else if ((s -= a.nC) < a.L * a.nP) {
        const int l = s / a.nP, p = s - l * a.nP;
        c = a.nC + p;
        frame = t0 + l;
        d0 = a.prescribed + (((long long)b * a.L + l) * a.nP + p) * a.P;
    } else {
        s -= a.L * a.nP;
        const int k = s / a.nG, g = s - k * a.nG, kt = k - 1 - a.context;      // 0 <= k <= L
        c = a.nC + a.nP + g;
        frame = t0 + k;
        d0 = k < a.L ? a.prognostic + (((long long)b * a.L + k) * a.nG + g) * a.P : nullptr;
        d1 = kt >= 0 ? a.target + (((long long)b * (a.L - a.context) + kt) * a.nG + g) * a.P : nullptr;
        e0 = ((long long)k * a.nG + g) * a.P;
        noisy = a.rng.noise > 0.f;
    }
    const dlwp_wb_channel ch = a.chan[c];
    if (!ch.base) return;
    const float* src = ch.base + frame * a.P;
    const bool norm = ch.normalize != 0;
    if (a.out_vec && (reinterpret_cast<uintptr_t>(ch.base) & 15) == 0)
        move_plane<true>(src, d0, d1, a.P, norm, ch.mean, ch.std, noisy, e0, (uint32_t)item, a.rng);
    else move_plane<false>(src, d0, d1, a.P, norm, ch.mean, ch.std, noisy, e0, (uint32_t)item, a.rng);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// grid.y: pieces of a plane, so that rows x pieces stays near TARGET_WGS
unsigned pieces(long long rows, long long n, bool vec) {
    const long long per = ((vec ? n >> 2 : n) + 255) / 256;
    const long long cap = std::max<long long>(1, TARGET_WGS / rows);
    return (unsigned)std::max<long long>(1, std::min<long long>(std::min(per, cap), 65535));
}

Rng make_rng(float noise, unsigned long long seed, int epoch, uint32_t tag) {
    return Rng{noise, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), (uint32_t)epoch, tag};
}

}  // namespace

extern "C" int dlwp_ns_batch(const float* u, int N, int T, long long F, const int* table, int B, int L, float noise,
                             unsigned long long seed, int epoch, float* x, float* y, void* stream) {
    DLWP_REQUIRE(u, DLWP_E_INVALID, "ns_batch: u is NULL");
    DLWP_REQUIRE(table, DLWP_E_INVALID, "ns_batch: table is NULL");
    DLWP_REQUIRE(x, DLWP_E_INVALID, "ns_batch: x is NULL");
    DLWP_REQUIRE(y, DLWP_E_INVALID, "ns_batch: y is NULL");
    DLWP_REQUIRE(N > 0 && T > 0 && F > 0 && B > 0, DLWP_E_INVALID, "ns_batch: N %d, T %d, F %lld, B %d must be positive", N, T, F, B);
    DLWP_REQUIRE(L >= 2, DLWP_E_INVALID, "ns_batch: sequence length L %d must be at least 2 (x and y are L - 1 frames)", L);
    DLWP_REQUIRE(L <= T, DLWP_E_INVALID, "ns_batch: sequence length L %d is longer than the trajectories (T %d)", L, T);
    DLWP_REQUIRE(noise >= 0.f && noise < INFINITY, DLWP_E_INVALID, "ns_batch: noise %g must be finite and not negative", (double)noise);
    DLWP_REQUIRE(epoch >= 0, DLWP_E_INVALID, "ns_batch: epoch %d is negative", epoch);
    DLWP_REQUIRE((long long)B * L <= INT_MAX, DLWP_E_UNSUPPORTED, "ns_batch: B %d x L %d frames are too many for one launch", B, L);
    DLWP_REQUIRE(F <= (1LL << 34) / L, DLWP_E_UNSUPPORTED, "ns_batch: a sample of %d x %lld floats exceeds the 2^34 elements of the noise counter", L, F);
    NsArgs a;
    a.u = u, a.table = table, a.x = x, a.y = y, a.F = F, a.N = N, a.T = T, a.L = L;
    a.vec = F % 4 == 0 && aligned16(u) && aligned16(x) && aligned16(y);
    a.rng = make_rng(noise, seed, epoch, DLWP_BATCH_TAG_NS);
    const long long rows = (long long)B * L;
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 4.0 * (double)F * (rows + 2.0 * B * (L - 1)), "ns_batch");
    hipLaunchKernelGGL(ns_batch_kernel, dim3((unsigned)rows, pieces(rows, F, a.vec)), dim3(256), 0, (hipStream_t)stream, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_wb_batch(const dlwp_wb_channel* chan, int nC, int nP, int nG, const int* items, int B, int L, int context,
                             int n_time, long long P, float noise, unsigned long long seed, int epoch, float* constants,
                             float* prescribed, float* prognostic, float* target, void* stream) {
    DLWP_REQUIRE(chan, DLWP_E_INVALID, "wb_batch: chan is NULL");
    DLWP_REQUIRE(items, DLWP_E_INVALID, "wb_batch: items is NULL");
    DLWP_REQUIRE(nC >= 0 && nP >= 0 && nG >= 0 && nC + nP + nG > 0 && nC <= 65535 && nP <= 65535 && nG <= 65535, DLWP_E_INVALID,
                 "wb_batch: channel counts (constants %d, prescribed %d, prognostic %d) must lie in [0, 65535] and not all be 0", nC, nP, nG);
    DLWP_REQUIRE(B > 0 && n_time > 0 && P > 0, DLWP_E_INVALID, "wb_batch: B %d, n_time %d, P %lld must be positive", B, n_time, P);
    DLWP_REQUIRE(L >= 2, DLWP_E_INVALID, "wb_batch: sequence length L %d must be at least 2", L);
    DLWP_REQUIRE(context >= 0 && context < L, DLWP_E_INVALID, "wb_batch: context %d must lie in [0, L = %d)", context, L);
    DLWP_REQUIRE(!nC || constants, DLWP_E_INVALID, "wb_batch: constants is NULL with %d constant channels", nC);
    DLWP_REQUIRE(!nP || prescribed, DLWP_E_INVALID, "wb_batch: prescribed is NULL with %d prescribed channels", nP);
    DLWP_REQUIRE(!nG || (prognostic && target), DLWP_E_INVALID, "wb_batch: prognostic or target is NULL with %d prognostic channels", nG);
    DLWP_REQUIRE(noise >= 0.f && noise < INFINITY, DLWP_E_INVALID, "wb_batch: noise %g must be finite and not negative", (double)noise);
    DLWP_REQUIRE(epoch >= 0, DLWP_E_INVALID, "wb_batch: epoch %d is negative", epoch);
    const long long planes = nC + (long long)L * nP + (L + 1LL) * nG;
    DLWP_REQUIRE(planes * B <= INT_MAX, DLWP_E_UNSUPPORTED, "wb_batch: %lld planes x B %d are too many for one launch", planes, B);
    DLWP_REQUIRE(!nG || P <= (1LL << 34) / L / nG, DLWP_E_UNSUPPORTED,
                 "wb_batch: a sample of %d x %d x %lld floats exceeds the 2^34 elements of the noise counter", L, nG, P);
    WbArgs a;
    a.chan = chan, a.items = items, a.constants = constants, a.prescribed = prescribed, a.prognostic = prognostic, a.target = target;
    a.P = P, a.nC = nC, a.nP = nP, a.nG = nG, a.L = L, a.context = context, a.n_time = n_time, a.planes = (int)planes;
    a.out_vec = P % 4 == 0 && aligned16(constants) && aligned16(prescribed) && aligned16(prognostic) && aligned16(target);
    a.rng = make_rng(noise, seed, epoch, DLWP_BATCH_TAG_WB);
    const long long rows = planes * B;
    const double moved = (double)nC + 2.0 * L * nP + (L + 1.0) * nG + (double)(2 * L - context) * nG;      // planes read + written per sample
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 4.0 * (double)P * B * moved, "wb_batch");
    hipLaunchKernelGGL(wb_batch_kernel, dim3((unsigned)rows, pieces(rows, P, a.out_vec)), dim3(256), 0, (hipStream_t)stream, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}
