// Seeded ensemble forecasts: the perturbation of an initial state into M members and the probabilistic scores of the members
// against the target -- CRPS terms, spread, error of the ensemble mean and the rank histogram -- per lead time.
//
// The reference has no ensembles; correctness is defined by the float64 restatement tests/ens_ref.py.  The noise is the stream of
// csrc/batch_rng.hip.h with the MEMBER in counter word 2 (where the batch kernels carry the epoch) and a tag of its own; the scores
// follow csrc/rollout_diag.hip: NORMALISED values are read once, sums run in a fixed order without atomics, every output address
// has one writer, and a chunk's results are written at its global frame indices, so a rollout scored in time chunks and batch
// chunks gives the bits of one call.
//
// ---- dlwp_ens_perturb ---------------------------------------------------------------------------------------------------------------
// out[b][m][e] = x[b][e] + sigma[(e / P) % V] z,  z = dlwp_noise4 with counter (e >> 2, items[b], m, DLWP_ENS_TAG), key = seed.
// A thread owns an aligned group of four elements of one sample: it reads them once and writes them for every member (16-byte
// pieces when F % 4 == 0 and both tensors are aligned, element by element otherwise: the same draws either way).  control != 0:
// member 0 is the input itself and draws nothing.  sigma == 0 gives x back exactly (fma(0, z, x), z finite).
//
// ---- dlwp_ens_diag --------------------------------------------------------------------------------------------------------------------
// A thread owns a pixel and holds its M members in registers: the kernel is a template on the member BUCKET (8, 16, 32, 64: the
// smallest that holds M; the knob ENS_BUCKET forces a larger one) and every loop over members is unrolled over the bucket behind a
// wave-uniform guard i < M, so that the members sit in a statically indexed array -- no scratch (docs/kernels/diagnostics.md has the
// compiler's figures) -- and a bucket wider than M costs registers, not work.  Per pixel, in fp32, members in ascending order:
//   a      = x_0,  e_i = x_i - a                     (exact for members that lie within a factor of two of each other)
//   mu     = (sum_i e_i) / M                         the ensemble mean is a + mu
//   col 0  = ((a - y) + mu)^2
//   col 1  = sum_i (e_i - mu)^2 / (M - 1)            two passes over held values; never E[x^2] - mean^2
//   col 2  = sum_i |x_i - y| / M
//   col 3  = sum_{i=1}^{M-1} (sum_{j<i} |x_i - x_j|) / (M (M - 1))      the O(M^2) loop in every bucket: at M = 64 its 2016
//            subtract / add pairs per pixel are about the time of the 65 loads they follow, and a sorting network would need
//            padding that the sums cannot carry
//   rank   = #{i : x_i < y}                          (a tie counts as not below)
// Decomposition.  A workgroup of 256 threads owns (sample, frame, variable) and a block of 256 K consecutive pixels; thread t takes
// the pixels block + 256 k + t for k = 0 .. K - 1, so a wave reads 256 contiguous bytes of every member.  K = ceil(H W / 16384)
// clamped to 1 .. 16: a function of H W ONLY.
// Summation order (fixed): per thread the four columns (times the row weight) over k ascending; the xor butterfly 32, 16, ..., 1
// over the wave; the four waves in ascending order -> one partial per block in the workspace; ens_fold_kernel adds the blocks in
// ascending order.  Ranks: per k and bin a wave ballot and its population count, added to a wave-uniform counter per bin (scalar
// registers); waves and blocks are added as above (integers: exact in any order).
//
// ---- dlwp_crps_loss_fwd_bwd -----------------------------------------------------------------------------------------------------------
// The CRPS of the members as a training loss, with its gradient from the same read (tests/crps_ref.py defines both): the
// decomposition of dlwp_ens_diag, one partial per block, crps_fold_kernel adds them in a fixed order.  See crps_loss_kernel.
#include "common.hip.h"
#include "dlwpmi_internal.h"
#include "batch_rng.hip.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int ENS_MAX_PIXELS = 1 << 21;      // pixels of a plane (721 x 1440 = 1 038 240 fits)
constexpr int ENS_TARGET_WGS = 2048;         // perturb: memory-bound copy, about eight workgroups per CU, the rest by striding

struct PerturbArgs {
    const float *x, *sigma;
    const int* items;
    float* out;
    long long F, P;
    int V, M, control;
    uint32_t k0, k1;
};

template <bool VEC>
__global__ __launch_bounds__(256) void ens_perturb_kernel(const PerturbArgs a) {
    const int b = blockIdx.y;
    const uint32_t item = (uint32_t)a.items[b];
    const float* src = a.x + (long long)b * a.F;
    float* dst = a.out + (long long)b * a.M * a.F;
    const long long groups = (a.F + 3) >> 2;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        const long long e0 = g << 2;
        float v[4], s[4];
        if constexpr (VEC) {
            const float4 q = reinterpret_cast<const float4*>(src)[g];
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        }
        const bool one_plane = (a.P & 3) == 0;               // the group lies inside one plane: one variable
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = VEC || e0 + j < a.F;
            if constexpr (!VEC) v[j] = ok ? src[e0 + j] : 0.f;
            s[j] = j > 0 && one_plane ? s[0] : ok ? a.sigma[((e0 + j) / a.P) % a.V] : 0.f;
        }
        for (int m = 0; m < a.M; ++m) {
            float o[4] = {v[0], v[1], v[2], v[3]};
            if (m > 0 || !a.control) {
                float z[4];
                dlwp_noise4((uint32_t)g, item, (uint32_t)m, DLWP_ENS_TAG, a.k0, a.k1, z);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fmaf(s[j], z[j], v[j]);
            }
            float* d = dst + (long long)m * a.F;
            if constexpr (VEC) {
                reinterpret_cast<float4*>(d)[g] = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e0 + j < a.F) d[e0 + j] = o[j];
            }
        }
    }
}

struct EnsArgs {
    const float *members, *target, *roww;
    long long bs, ms, ts;
    int Bc, M, Tc, V, H, W, hw, K, nblk;
    float* part;      // [Bc][Tc][V][nblk][4] sums, then (as int) [Bc][Tc][V][nblk][M + 1] rank counts
    int* rpart;
};

template <int MB>
__global__ __launch_bounds__(256) void ens_diag_kernel(const EnsArgs a) {
    __shared__ float red_s[4][4];
    __shared__ int red_r[4][MB + 1];
    const int tc = blockIdx.x / a.nblk, blk = blockIdx.x - tc * a.nblk, v = blockIdx.y, b = blockIdx.z;
    const int lane = lane_id(), wave = wave_id(), M = a.M;
    const float* mp = a.members + b * a.bs + tc * a.ts + (long long)v * a.hw;
    const float* tp = a.target + (((long long)b * a.Tc + tc) * a.V + v) * a.hw;
    const float invM = 1.f / (float)M, invM1 = 1.f / (float)(M - 1), invP = invM * invM1;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int hist[MB + 1];            // wave-uniform counts of the rank bins (ballot + population count: scalar registers)
#pragma unroll
    for (int j = 0; j <= MB; ++j) hist[j] = 0;
    for (int k = 0; k < a.K; ++k) {
        const int p = (blk * a.K + k) * 256 + (int)threadIdx.x;
        const bool ok = p < a.hw;
        // the member stride is made opaque per round: the MB member offsets and guards are then formed on the fly with scalar adds
        // and compares instead of being hoisted out of the k loop into more scalar registers than there are
        long long ms = a.ms;
        int M = a.M;
        asm volatile("" : "+s"(ms), "+s"(M));
        float x[MB];
        const float* q = mp + p;
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            x[i] = ok && i < M ? *q : 0.f;
            q += ms;
        }
        const float y = ok ? tp[p] : 0.f;
        const float w = ok ? (a.roww ? a.roww[p / a.W] : 1.f) : 0.f;
        const float x0 = x[0];
        float se = 0.f, sa = 0.f, pair = 0.f, var = 0.f;
        int below = 0;
        // (guards, not exits: a loop with an exit is not unrolled, and x[] would be indexed at run time)
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            if (i < M) {
                se += x[i] - x0;
                sa += fabsf(x[i] - y);
                below += x[i] < y ? 1 : 0;
                float r = 0.f;
#pragma unroll
                for (int j = 0; j < i; ++j) r += fabsf(x[i] - x[j]);
                pair += r;
            }
        }
        const float mu = se * invM;
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            if (i < M) {
                const float d = (x[i] - x0) - mu;
                var += d * d;
            }
        }
        const float dm = (x0 - y) + mu;
        acc[0] += w * (dm * dm);
        acc[1] += w * (var * invM1);
        acc[2] += w * (sa * invM);
        acc[3] += w * (pair * invP);
        const int c = ok ? below : -1;      // a lane without a pixel falls in no bin
#pragma unroll
        for (int j = 0; j <= MB; ++j)
            if (j <= M) hist[j] += __popcll(__ballot(c == j));
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        float o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = __shfl_xor(acc[q], s);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += o[q];
    }
    if (lane < 4) red_s[wave][lane] = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j <= MB; ++j)
            if (j <= M) red_r[wave][j] = hist[j];
    }
    __syncthreads();
    const long long f = (((long long)b * a.Tc + tc) * a.V + v) * a.nblk + blk;
    const int t = threadIdx.x;
    if (t < 4) a.part[f * 4 + t] = ((red_s[0][t] + red_s[1][t]) + red_s[2][t]) + red_s[3][t];
    if (t <= M) a.rpart[f * (M + 1) + t] = red_r[0][t] + red_r[1][t] + red_r[2][t] + red_r[3][t];
}

// sums [Bc][T][V][4] and ranks [Bc][T][V][M + 1] <- the blocks' partials in ascending block order
__global__ __launch_bounds__(256) void ens_fold_kernel(const float* __restrict__ part, const int* __restrict__ rpart, float* sums, int* ranks,
                                                       long long n, int Tc, int V, int M, int nblk, int t_begin, int T) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;      // e = ((b Tc + tc) V + v) (M + 5) + c
    if (e >= n) return;
    const int c = (int)(e % (M + 5));
    const long long q = e / (M + 5);
    const int v = (int)(q % V);
    const long long bt = q / V;
    const int tc = (int)(bt % Tc);
    const long long b = bt / Tc;
    const long long z = (b * T + t_begin + tc) * V + v;
    if (c < 4) {
        float s = 0.f;
        for (int i = 0; i < nblk; ++i) s += part[(q * nblk + i) * 4 + c];
        sums[z * 4 + c] = s;
    } else {
        int s = 0;
        for (int i = 0; i < nblk; ++i) s += rpart[(q * nblk + i) * (M + 1) + c - 4];
        ranks[z * (M + 1) + c - 4] = s;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// pixels per thread: a function of H W only, so that the summation order does not depend on the chunking
int ens_ppt(long long hw) { return (int)std::min<long long>(16, std::max<long long>(1, (hw + 16383) / 16384)); }

int ens_check_shape(const char* who, int Bc, int M, int Tc, int V, int H, int W) {
    DLWP_REQUIRE(Bc > 0 && Tc > 0 && V > 0 && H > 0 && W > 0, DLWP_E_INVALID, "%s: Bc %d, Tc %d, V %d, H %d, W %d must be positive", who, Bc, Tc, V,
                 H, W);
    DLWP_REQUIRE(M >= 2, DLWP_E_INVALID, "%s: M %d members: the spread and the pair term need at least 2", who, M);
    DLWP_REQUIRE(M <= DLWP_ENS_MAX_MEMBERS, DLWP_E_UNSUPPORTED, "%s: M %d members above %d", who, M, DLWP_ENS_MAX_MEMBERS);
    DLWP_REQUIRE((long long)H * W <= ENS_MAX_PIXELS, DLWP_E_UNSUPPORTED, "%s: %d x %d points above %d", who, H, W, ENS_MAX_PIXELS);
    DLWP_REQUIRE(V <= 65535 && Bc <= 65535, DLWP_E_UNSUPPORTED, "%s: grid limits (V %d, Bc %d above 65535)", who, V, Bc);
    return DLWP_OK;
}

int ens_blocks(int H, int W) {
    const long long hw = (long long)H * W;
    return (int)((hw + 256LL * ens_ppt(hw) - 1) / (256LL * ens_ppt(hw)));
}

// the member bucket of dlwp_ens_diag and dlwp_crps_loss_fwd_bwd: the smallest that holds M, or the one the knob forces
int ens_bucket(const char* who, int M, int* bucket) {
    const int forced = dlwp_tune_or("ENS_BUCKET", 0);
    DLWP_REQUIRE(forced == 0 || forced == 8 || forced == 16 || forced == 32 || forced == 64, DLWP_E_INVALID,
                 "%s: ENS_BUCKET %d is not 0 (auto), 8, 16, 32 or 64", who, forced);
    DLWP_REQUIRE(forced == 0 || forced >= M, DLWP_E_UNSUPPORTED, "%s: ENS_BUCKET %d cannot hold M %d members", who, forced, M);
    *bucket = forced ? forced : M <= 8 ? 8 : M <= 16 ? 16 : M <= 32 ? 32 : 64;
    return DLWP_OK;
}

struct CrpsArgs {
    const float *members, *target, *roww, *varw;
    long long bs, ms, ts, gms;      // gms: the member stride of the dense gradient, Tc V H W
    int M, Tc, V, W, hw, K, nblk;
    float invM, cp;                 // the value: 1 / M and lambda / (M (M - 1))
    double a1, a2;                  // the gradient: 1 / (N M) and lambda / (N M (M - 1))
    float *grad, *part;             // part [B][Tc][V][nblk]: one weighted pixel sum per block
};

// One thread per pixel as ens_diag_kernel (same blocks, same K, same member bucket and guards).  For member i the loop over ALL j
// counts c_i = #{j : x_j < x_i} - #{j : x_j > x_i}: it serves the pair term, sum_{i<j} |x_i - x_j| = sum_i (x_i - x_0) c_i (the c_i
// add up to 0, so any shift of x is free and x_0 keeps the products small), and it IS the pair term's gradient.  The j loop runs
// unguarded over chunks of eight held members; the members from M up to the chunk's end are NaN, which compares false both ways.
// Member i's gradient is formed and stored inside the i loop and never held: lane t writes pixel block + 256 k + t, so a wave
// writes 256 contiguous bytes per member.  Its bracket sgn(x_i - y) / M - lambda c_i / (M (M - 1)) is made of two integers; the
// scaling by r_h c_v / N runs in double and is rounded to fp32 once (a handful of operations per member against the 4 M of the
// count loop), so an element is within one fp32 rounding of the exact gradient.
template <int MB, bool GRAD>
__global__ __launch_bounds__(256) void crps_loss_kernel(const CrpsArgs a) {
    __shared__ float red[4];
    const int tc = blockIdx.x / a.nblk, blk = blockIdx.x - tc * a.nblk, v = blockIdx.y, b = blockIdx.z;
    const int lane = lane_id(), wave = wave_id();
    const long long f = ((long long)b * a.Tc + tc) * a.V + v;
    const float* mp = a.members + b * a.bs + tc * a.ts + (long long)v * a.hw;
    const float* tp = a.target + f * a.hw;
    float* gp = GRAD ? a.grad + (((long long)b * a.M * a.Tc + tc) * a.V + v) * a.hw : nullptr;
    const float cv = a.varw ? a.varw[v] : 1.f;
    float acc = 0.f;
    for (int k = 0; k < a.K; ++k) {
        const int p = (blk * a.K + k) * 256 + (int)threadIdx.x;
        const bool ok = p < a.hw;
        // opaque per round, as in ens_diag_kernel: the member offsets are formed with scalar adds, not hoisted out of the k loop
        long long ms = a.ms, gms = a.gms;
        int M = a.M;
        asm volatile("" : "+s"(ms), "+s"(gms), "+s"(M));
        float x[MB];
        const float* q = mp + p;
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            x[i] = i < M ? (ok ? *q : 0.f) : __builtin_nanf("");
            q += ms;
        }
        const float y = ok ? tp[p] : 0.f;
        const float w = ok ? (a.roww ? a.roww[p / a.W] : 1.f) : 0.f;
        const double wd = (double)w * (double)cv;      // exact
        const float x0 = x[0];
        float sa = 0.f, pair = 0.f;
        float* gq = GRAD ? gp + p : nullptr;
        auto member = [&](const float xi) {
            int c = 0;
#pragma unroll
            for (int j0 = 0; j0 < MB; j0 += 8) {
                if (j0 == 0 || j0 < M) {
#pragma unroll
                    for (int j = j0; j < j0 + 8; ++j) c += (x[j] < xi ? 1 : 0) - (x[j] > xi ? 1 : 0);
                }
            }
            sa += fabsf(xi - y);
            pair = fmaf(xi - x0, (float)c, pair);
            if constexpr (GRAD) {
                const int sg = (xi > y ? 1 : 0) - (xi < y ? 1 : 0);      // sgn(0) = 0
                const float g = (float)(wd * fma(-a.a2, (double)c, (double)sg * a.a1));
                if (ok) *gq = g;
                gq += gms;
            }
        };
        if constexpr (MB <= 32) {
#pragma unroll
            for (int i = 0; i < MB; ++i)
                if (i < M) member(x[i]);
        } else {
            // 64 x 64 unrolled comparisons are more code than the instruction cache holds, and a rolled loop cannot index the held
            // array: member i is read a second time (from the cache: the wave has just loaded the line) while x[] serves the j loop
            const float* q2 = mp + p;
#pragma unroll 1
            for (int i = 0; i < M; ++i) {
                member(ok ? *q2 : 0.f);
                q2 += ms;
            }
        }
        acc += (w * cv) * fmaf(-a.cp, pair, sa * a.invM);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) a.part[f * a.nblk + blk] = ((red[0] + red[1]) + red[2]) + red[3];
}

// loss <- invN times the n block partials: thread t adds the partials t, t + 256, ... in ascending order, then the wave butterfly
// and the four waves in ascending order (one workgroup: a fixed order for a given n)
__global__ __launch_bounds__(256) void crps_fold_kernel(const float* __restrict__ part, long long n, float invN, float* loss) {
    __shared__ float red[4];
    float s = 0.f;
    for (long long e = threadIdx.x; e < n; e += 256) s += part[e];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if (lane_id() == 0) red[wave_id()] = s;
    __syncthreads();
    if (threadIdx.x == 0) *loss = (((red[0] + red[1]) + red[2]) + red[3]) * invN;
}

template <bool GRAD>
void crps_launch(int bucket, dim3 grid, hipStream_t stream, const CrpsArgs& a) {
    if (bucket == 8) hipLaunchKernelGGL((crps_loss_kernel<8, GRAD>), grid, dim3(256), 0, stream, a);
    else if (bucket == 16) hipLaunchKernelGGL((crps_loss_kernel<16, GRAD>), grid, dim3(256), 0, stream, a);
    else if (bucket == 32) hipLaunchKernelGGL((crps_loss_kernel<32, GRAD>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((crps_loss_kernel<64, GRAD>), grid, dim3(256), 0, stream, a);
}

}  // namespace

extern "C" int dlwp_ens_perturb(const float* x, const int* items, const float* sigma, int B, long long F, long long P, int V, int M,
                                int control, unsigned long long seed, float* out, void* stream) {
    DLWP_REQUIRE(x, DLWP_E_INVALID, "ens_perturb: x is NULL");
    DLWP_REQUIRE(items, DLWP_E_INVALID, "ens_perturb: items is NULL");
    DLWP_REQUIRE(sigma, DLWP_E_INVALID, "ens_perturb: sigma is NULL");
    DLWP_REQUIRE(out, DLWP_E_INVALID, "ens_perturb: out is NULL");
    DLWP_REQUIRE(B > 0 && F > 0 && P > 0 && V > 0, DLWP_E_INVALID, "ens_perturb: B %d, F %lld, P %lld, V %d must be positive", B, F, P, V);
    DLWP_REQUIRE(M >= 1, DLWP_E_INVALID, "ens_perturb: M %d members must be at least 1", M);
    DLWP_REQUIRE(M <= DLWP_ENS_MAX_MEMBERS, DLWP_E_UNSUPPORTED, "ens_perturb: M %d members above %d", M, DLWP_ENS_MAX_MEMBERS);
    DLWP_REQUIRE(P <= F / V && F % (P * V) == 0, DLWP_E_INVALID, "ens_perturb: F %lld is not a multiple of V %d planes of P %lld floats", F, V, P);
    DLWP_REQUIRE(F <= (1LL << 34), DLWP_E_UNSUPPORTED, "ens_perturb: a sample of %lld floats exceeds the 2^34 elements of the noise counter", F);
    DLWP_REQUIRE(B <= 65535, DLWP_E_UNSUPPORTED, "ens_perturb: grid limits (B %d above 65535)", B);
    PerturbArgs a;
    a.x = x, a.items = items, a.sigma = sigma, a.out = out, a.F = F, a.P = P, a.V = V, a.M = M, a.control = control != 0;
    a.k0 = (uint32_t)(seed & 0xffffffffull), a.k1 = (uint32_t)(seed >> 32);
    const bool vec = F % 4 == 0 && aligned16(x) && aligned16(out);
    const long long per = (((F + 3) >> 2) + 255) / 256;
    const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>(per, std::max(1, ENS_TARGET_WGS / B)));
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 4.0 * (double)B * (double)F * (M + 1), "ens_perturb");
    if (vec) hipLaunchKernelGGL(ens_perturb_kernel<true>, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(ens_perturb_kernel<false>, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" long long dlwp_ens_diag_ws_floats(int Bc, int M, int Tc, int V, int H, int W) {
    const int rc = ens_check_shape("ens_diag_ws_floats", Bc, M, Tc, V, H, W);
    if (rc) return rc;
    return (long long)Bc * Tc * V * ens_blocks(H, W) * (M + 5);      // per block four sums and M + 1 rank counts
}

extern "C" int dlwp_ens_diag(const float* members, long long bstride, long long mstride, long long tstride, const float* target,
                             const float* row_weights, int Bc, int M, int Tc, int V, int H, int W, int t_begin, int T, float* sums,
                             int* ranks, float* ws, void* stream) {
    DLWP_REQUIRE(members, DLWP_E_INVALID, "ens_diag: members is NULL");
    DLWP_REQUIRE(target, DLWP_E_INVALID, "ens_diag: target is NULL");
    DLWP_REQUIRE(sums, DLWP_E_INVALID, "ens_diag: sums is NULL");
    DLWP_REQUIRE(ranks, DLWP_E_INVALID, "ens_diag: ranks is NULL");
    DLWP_REQUIRE(ws, DLWP_E_INVALID, "ens_diag: ws is NULL (dlwp_ens_diag_ws_floats gives its size)");
    int rc = ens_check_shape("ens_diag", Bc, M, Tc, V, H, W);
    if (rc) return rc;
    DLWP_REQUIRE(T > 0, DLWP_E_INVALID, "ens_diag: T %d must be positive", T);
    DLWP_REQUIRE(bstride >= 0 && mstride >= 0 && tstride >= 0, DLWP_E_INVALID,
                 "ens_diag: negative stride of members (batch %lld, member %lld, time %lld)", bstride, mstride, tstride);
    DLWP_REQUIRE(t_begin >= 0 && (long long)t_begin + Tc <= T, DLWP_E_INVALID, "ens_diag: chunk t_begin %d + Tc %d is outside the rollout T %d",
                 t_begin, Tc, T);
    int bucket;
    rc = ens_bucket("ens_diag", M, &bucket);
    if (rc) return rc;
    EnsArgs a;
    a.members = members, a.target = target, a.roww = row_weights, a.bs = bstride, a.ms = mstride, a.ts = tstride;
    a.Bc = Bc, a.M = M, a.Tc = Tc, a.V = V, a.H = H, a.W = W, a.hw = H * W, a.K = ens_ppt(a.hw), a.nblk = ens_blocks(H, W);
    DLWP_REQUIRE((long long)Tc * a.nblk <= INT_MAX, DLWP_E_UNSUPPORTED, "ens_diag: Tc %d x %d pixel blocks are too many workgroups", Tc, a.nblk);
    const long long fields = (long long)Bc * Tc * V;
    a.part = ws;
    a.rpart = reinterpret_cast<int*>(ws + fields * a.nblk * 4);
    {
        dlwp_prof_scope prof((hipStream_t)stream, 0.0, 4.0 * (double)fields * a.hw * (M + 1), "ens_diag_m%d", bucket);
        const dim3 grid((unsigned)(Tc * a.nblk), V, Bc);
        if (bucket == 8) hipLaunchKernelGGL(ens_diag_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, a);
        else if (bucket == 16) hipLaunchKernelGGL(ens_diag_kernel<16>, grid, dim3(256), 0, (hipStream_t)stream, a);
        else if (bucket == 32) hipLaunchKernelGGL(ens_diag_kernel<32>, grid, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(ens_diag_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, a);
        DLWP_LAUNCH_CHECK();
    }
    const long long nf = fields * (M + 5);
    DLWP_REQUIRE((nf + 255) / 256 <= INT_MAX, DLWP_E_UNSUPPORTED, "ens_diag: %lld sums are too many", nf);
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 4.0 * nf * (a.nblk + 1), "ens_diag_fold");
    hipLaunchKernelGGL(ens_fold_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, a.rpart, sums, ranks, nf, Tc,
                       V, M, a.nblk, t_begin, T);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" long long dlwp_crps_loss_ws_floats(int B, int M, int T, int V, int H, int W) {
    const int rc = ens_check_shape("crps_loss_ws_floats", B, M, T, V, H, W);
    if (rc) return rc;
    return (long long)B * T * V * ens_blocks(H, W);      // one weighted pixel sum per block
}

extern "C" int dlwp_crps_loss_fwd_bwd(const float* members, long long bstride, long long mstride, long long tstride, const float* target,
                                      const float* row_weights, const float* var_weights, int B, int M, int T, int V, int H, int W,
                                      float pair_coeff, float* loss_out, float* grad, float* ws, void* stream) {
    DLWP_REQUIRE(members, DLWP_E_INVALID, "crps_loss: members is NULL");
    DLWP_REQUIRE(target, DLWP_E_INVALID, "crps_loss: target is NULL");
    DLWP_REQUIRE(loss_out, DLWP_E_INVALID, "crps_loss: loss_out is NULL");
    DLWP_REQUIRE(ws, DLWP_E_INVALID, "crps_loss: ws is NULL (dlwp_crps_loss_ws_floats gives its size)");
    int rc = ens_check_shape("crps_loss", B, M, T, V, H, W);
    if (rc) return rc;
    DLWP_REQUIRE(bstride >= 0 && mstride >= 0 && tstride >= 0, DLWP_E_INVALID,
                 "crps_loss: negative stride of members (batch %lld, member %lld, time %lld)", bstride, mstride, tstride);
    DLWP_REQUIRE(std::isfinite(pair_coeff) && pair_coeff >= 0.f && pair_coeff <= 1.f, DLWP_E_INVALID,
                 "crps_loss: pair_coeff %g must be finite and lie in [0, 1]", (double)pair_coeff);
    int bucket;
    rc = ens_bucket("crps_loss", M, &bucket);
    if (rc) return rc;
    CrpsArgs a;
    a.members = members, a.target = target, a.roww = row_weights, a.varw = var_weights, a.bs = bstride, a.ms = mstride, a.ts = tstride;
    a.M = M, a.Tc = T, a.V = V, a.W = W, a.hw = H * W, a.K = ens_ppt(a.hw), a.nblk = ens_blocks(H, W);
    DLWP_REQUIRE((long long)T * a.nblk <= INT_MAX, DLWP_E_UNSUPPORTED, "crps_loss: T %d x %d pixel blocks are too many workgroups", T, a.nblk);
    const long long fields = (long long)B * T * V;
    const double N = (double)fields * a.hw;
    a.gms = (long long)T * V * a.hw;
    a.invM = 1.f / (float)M, a.cp = (float)((double)pair_coeff / ((double)M * (M - 1)));
    a.a1 = 1.0 / (N * M), a.a2 = (double)pair_coeff / (N * M * (M - 1));
    a.grad = grad, a.part = ws;
    {
        dlwp_prof_scope prof((hipStream_t)stream, 0.0, 4.0 * (double)fields * a.hw * (M + 1 + (grad ? M : 0)), "crps_loss_%s_m%d",
                             grad ? "fwd_bwd" : "fwd", bucket);
        const dim3 grid((unsigned)(T * a.nblk), V, B);
        if (grad) crps_launch<true>(bucket, grid, (hipStream_t)stream, a);
        else crps_launch<false>(bucket, grid, (hipStream_t)stream, a);
        DLWP_LAUNCH_CHECK();
    }
    const long long n = fields * a.nblk;
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 4.0 * (double)(n + 1), "crps_loss_fold");
    hipLaunchKernelGGL(crps_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, n, (float)(1.0 / N), loss_out);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}
