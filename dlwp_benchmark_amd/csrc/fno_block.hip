// FNO block = SpectralConv (mode-truncated rfft2 -> per-mode complex channel mixing -> irfft2)
// + linear (1x1) skip + bias, forward and backward.  Arithmetic restated from neuralop
// SpectralConv/FNOBlocks (third-party); reference call sites
// `self.fno(x_t)` src/nsbench/models/fno/fno.py:38,96,246, src/dlwpbench/models/fno/fno.py:103.
//
// MI355X design.  Only m1 x m2c modes of the H x (W/2+1) spectrum are ever used (12 x 7 of
// 64 x 33 at the headline config), so no FFT is run: the transform is a pruned DFT factored
// into a W-axis step (a [C x W] x [W x 2*m2c] GEMM per image row) and an H-axis step
// (m1 complex dot products of length H per (channel, column)).  Three kernels per block:
//   rows   : one workgroup per image row (b,h), all channels: W-axis DFT on MFMA -> x1[b][h][kx][c]
//   mix    : one workgroup per kept mode (j,kx): H-axis step, complex channel contraction with
//            the mode's [C x C] weight slice (mode-major layout => contiguous 8*C*C bytes)
//   spatial: one workgroup per image row: inverse H-step (tiny), then ONE concatenated-K MFMA
//            GEMM  pre[o][w] = [Wskip | Y1(o,:)] . [x ; G]  (skip conv + inverse W-axis DFT),
//            bias, and optionally the next block's `rows` stage fused on the result.
// The backward pass reuses the same three kernels with adjoint tables.
#include "common.hip.h"
#include "dlwpmi_internal.h"
#include "fno_rows.hip.h"
#include "pwmlp_bwd.hip.h"
#include "pwmlp_fwd.hip.h"
#include <cmath>
#include <vector>

namespace {

struct SpatialDev {
    const float* tin; const float2* spec; const float* wskip; const float* bias;
    const float* pprev; float* out; float2* x1_out; float* g_wskip; float* g_bias;
    float* gslab; int gslab_accumulate;   // per-workgroup {g_wskip[C*C], g_bias[C]} partials (stride C*C+C padded to 4)
    const float2* twH; const float* G; const float* FT;
    int act_tin, transpose_w, act_prev, x1_act, is_bwd, vec_w;
    int C, H, W, m1, m2c, C_pad, NP;
    FastDiv dC;
};

struct RowsDev {
    const float* x; float2* x1; const float* FT;
    int act, C, H, W, m2c, C_pad, NP;
};

template <int NCB, int NBN>
__global__ __launch_bounds__(256) void fno_rows_kernel(RowsDev a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int LDP = a.W + 4;
    float* tile = smem;                    // [C_pad][LDP]
    float* ft = tile + a.C_pad * LDP;      // [NP][LDP]
    float* x1s = ft + a.NP * LDP;          // [4 waves][C_pad][NP]
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
    const int W4 = a.W / 4;
    for (int idx = tid; idx < a.C_pad * W4; idx += 256) {
        const int c = idx / W4, x4 = idx % W4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < a.C) v = *reinterpret_cast<const float4*>(&a.x[(((long long)b * a.C + c) * a.H + h) * a.W + 4 * x4]);
        *reinterpret_cast<float4*>(&tile[c * LDP + 4 * x4]) = v;
    }
    for (int idx = tid; idx < a.NP * W4; idx += 256) {
        const int n = idx / W4, x4 = idx % W4;
        *reinterpret_cast<float4*>(&ft[n * LDP + 4 * x4]) = *reinterpret_cast<const float4*>(&a.FT[n * a.W + 4 * x4]);
    }
    __syncthreads();
    tile_rows_dft<NCB, NBN>(tile, ft, x1s, LDP, a.NP, a.W / 16, a.act != 0);
    __syncthreads();
    store_x1(x1s, a.x1, b, h, a.H, a.m2c, a.C, a.C_pad, a.NP);
}

// ------------------------------------------------------------------------------------------
// The `spatial` chain: one image row (b,h) from its inputs to `out` and, fused, the next stage's row DFT.  256 threads (four
// waves) run it: the whole workgroup of fno_spatial_kernel, role A (waves 0-3) of fno_spatial_roles_kernel.  The phases below are
// its only copy, so the two kernels share thread-to-element mapping and arithmetic by construction; each kernel calls them in
// order and keeps the three barriers between them at its own top level.  Every stride is SPATIAL_NT, never blockDim.x.
constexpr int SPATIAL_NT = 256;
constexpr int SPATIAL_MJ = 16;   // H-step operands a thread holds in registers (modes j < 16; a larger m1 loops)

// LDS of the two kernels.  ROLES is the only place where the layouts differ: the four-wave kernel has the forward's bias_s, and
// its gks (bwd) lies over gs / ks / s1, which are dead after the main GEMM; in the two-role kernel role B fills gks while role A
// fills gs / ks / s1, so it is a region of its own (`lds` / `lds_roles` in dlwp_fno_spatial).
struct SpatialLds {
    float *tin_s, *tout_s, *pprev_s;   // [C_pad][LDP] each; pprev_s: bwd
    float* ft;                         // [NP][LDP]
    float* x1s;                        // [4 waves][C_pad][NP]
    float* bias_s;                     // [C_pad]          four-wave layout only
    float *gs, *ks, *s1;               // [NP][LDP], [C_pad][LDK], [C_pad][LDS1]: the operands of the main GEMM
    float* gks;                        // [4 waves][C_pad][C_pad]
    int LDP, LDK, LDS1;
};
template <bool ROLES>
__device__ __forceinline__ SpatialLds carve_spatial_lds(float* smem, const SpatialDev& a) {
    SpatialLds L;
    L.LDP = a.W + 4; L.LDK = a.C_pad + 4; L.LDS1 = a.NP + 4;
    L.tin_s = smem;
    L.tout_s = L.tin_s + a.C_pad * L.LDP;
    L.pprev_s = L.tout_s + a.C_pad * L.LDP;
    L.ft = L.pprev_s + a.C_pad * L.LDP;
    L.x1s = L.ft + a.NP * L.LDP;
    L.bias_s = ROLES ? nullptr : L.x1s + 4 * a.C_pad * a.NP;
    L.gs = L.x1s + 4 * a.C_pad * a.NP + (ROLES ? 0 : a.C_pad);
    L.ks = L.gs + a.NP * L.LDP;
    L.s1 = L.ks + a.C_pad * L.LDK;
    L.gks = ROLES ? L.s1 + a.C_pad * L.LDS1 : L.gs;
    return L;
}

// what the issue phase leaves in registers for the commit phase and the H-step
struct SpatialLoads {
    float4 tv[2], pv[2], gv, fv;
    MatLoad<1> lk;
    int nk;
    float2 sv[SPATIAL_MJ], twl;
    float bias_v;
};

// Issue phase: the first chunk of every independent input goes into registers before any LDS write, so the workgroup pays one
// global latency for all of them (larger shapes loop afterwards).  MODE 0 is the only one with a bias.
template <int MODE>
__device__ __forceinline__ void spatial_issue(const SpatialDev& a, int b, int h, bool need_prev, SpatialLoads& R) {
    const int tid = threadIdx.x, lane = lane_id(), W4 = a.W / 4;
    const int tile_units = a.C_pad * W4, tab_units = a.NP * W4;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int u = tid + SPATIAL_NT * k, c = u / W4, x4 = u - c * W4;
        R.tv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        R.pv[k] = R.tv[k];
        if (u < tile_units && c < a.C) {
            const long long off = (((long long)b * a.C + c) * a.H + h) * a.W + 4 * x4;
            R.tv[k] = *reinterpret_cast<const float4*>(&a.tin[off]);
            if (need_prev) R.pv[k] = *reinterpret_cast<const float4*>(&a.pprev[off]);
        }
    }
    R.gv = make_float4(0.f, 0.f, 0.f, 0.f);
    R.fv = R.gv;
    if (tid < tab_units) {
        R.gv = reinterpret_cast<const float4*>(a.G)[tid];
        if (a.x1_out) R.fv = reinterpret_cast<const float4*>(a.FT)[tid];
    }
    // wskip: one 16-byte unit per thread, the rest in the tail loop of the commit phase.  The unit count is written out, not
    // matload_units(): that caps by blockDim.x, which is 512 in the two-role kernel.  MatLoad itself indexes unit k with
    // k * blockDim.x: harmless here only because MAXU is 1 (k = 0)
    R.nk = a.vec_w ? min((a.C * a.C) >> 2, SPATIAL_NT) : 0;
    R.lk.issue(a.wskip, R.nk);
    // inverse H-axis step operands for this row: spec[b][j][kx][o], j < min(m1, 16)
    const int d_kx = tid / a.C_pad, d_o = tid - d_kx * a.C_pad;
    const bool d_valid = tid < a.C_pad * (a.NP / 2) && d_kx < a.m2c && d_o < a.C;
    // unconditional loads from clamped (always valid) addresses: a select right behind each load would
    // make the compiler wait for every load separately; invalid lanes/steps are ignored at use
    const float2* sp = a.spec + (((long long)b * a.m1) * a.m2c + (d_valid ? d_kx : 0)) * a.C + (d_valid ? d_o : 0);
    const long long jstride = (long long)a.m2c * a.C;
#pragma unroll
    for (int j = 0; j < SPATIAL_MJ; ++j) R.sv[j] = sp[(j < a.m1 ? j : a.m1 - 1) * jstride];
    // twiddles of this row: lane j (mod 16) holds tw[j]; a uniform index would become a chain of scalar loads
    // with a wait each.  Broadcast with shuffles at use.
    const int twj = (lane & 15) < a.m1 ? (lane & 15) : a.m1 - 1;
    R.twl = a.twH[twj * a.H + h];
    R.bias_v = 0.f;
    if (MODE == 0) {
        const float bias_raw = a.bias ? a.bias[tid < a.C ? tid : 0] : 0.f;
        R.bias_v = tid < a.C ? bias_raw : 0.f;
    }
}

// Commit phase: the tile (tin, pprev), the tables (G, FT), Wskip and, in MODE 0, the bias into LDS
template <int MODE>
__device__ __forceinline__ void spatial_commit(const SpatialDev& a, const SpatialLds& L, int b, int h, bool need_prev,
                                               const SpatialLoads& R) {
    const int tid = threadIdx.x, W4 = a.W / 4, LDP = L.LDP;
    const int tile_units = a.C_pad * W4, tab_units = a.NP * W4;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int u = tid + SPATIAL_NT * k, c = u / W4, x4 = u - c * W4;
        if (u < tile_units) {
            float4 v = R.tv[k];
            if (a.act_tin) { const f32x4 ga = gelu4(f32x4{v.x, v.y, v.z, v.w}); v = make_float4(ga[0], ga[1], ga[2], ga[3]); }
            *reinterpret_cast<float4*>(&L.tin_s[c * LDP + 4 * x4]) = v;
            if (need_prev) *reinterpret_cast<float4*>(&L.pprev_s[c * LDP + 4 * x4]) = R.pv[k];
        }
    }
    for (int idx = tid + 2 * SPATIAL_NT; idx < tile_units; idx += SPATIAL_NT) {
        const int c = idx / W4, x4 = idx % W4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f), pvv = v;
        if (c < a.C) {
            const long long off = (((long long)b * a.C + c) * a.H + h) * a.W + 4 * x4;
            v = *reinterpret_cast<const float4*>(&a.tin[off]);
            if (a.act_tin) { const f32x4 ga = gelu4(f32x4{v.x, v.y, v.z, v.w}); v = make_float4(ga[0], ga[1], ga[2], ga[3]); }
            if (need_prev) pvv = *reinterpret_cast<const float4*>(&a.pprev[off]);
        }
        *reinterpret_cast<float4*>(&L.tin_s[c * LDP + 4 * x4]) = v;
        if (need_prev) *reinterpret_cast<float4*>(&L.pprev_s[c * LDP + 4 * x4]) = pvv;
    }
    DLWP_STAMP(2);
    if (tid < tab_units) {
        const int n = tid / W4, x4 = tid - n * W4;
        *reinterpret_cast<float4*>(&L.gs[n * LDP + 4 * x4]) = R.gv;
        if (a.x1_out) *reinterpret_cast<float4*>(&L.ft[n * LDP + 4 * x4]) = R.fv;
    }
    for (int idx = tid + SPATIAL_NT; idx < tab_units; idx += SPATIAL_NT) {
        const int n = idx / W4, x4 = idx % W4;
        *reinterpret_cast<float4*>(&L.gs[n * LDP + 4 * x4]) = *reinterpret_cast<const float4*>(&a.G[n * a.W + 4 * x4]);
        if (a.x1_out)
            *reinterpret_cast<float4*>(&L.ft[n * LDP + 4 * x4]) = *reinterpret_cast<const float4*>(&a.FT[n * a.W + 4 * x4]);
    }
    if (a.transpose_w) {
        R.lk.commit<true>(L.ks, L.LDK, a.C, a.dC, R.nk);
        stage_matrix_tail<true, SPATIAL_NT>(L.ks, L.LDK, a.wskip, a.C, a.C, a.dC, R.nk);
    } else {
        R.lk.commit<false>(L.ks, L.LDK, a.C, a.dC, R.nk);
        stage_matrix_tail<false, SPATIAL_NT>(L.ks, L.LDK, a.wskip, a.C, a.C, a.dC, R.nk);
    }
    zero_padding<SPATIAL_NT>(L.ks, L.LDK, a.C, a.C, a.C_pad, a.C_pad);
    if (MODE == 0) {
        if (tid < a.C_pad) L.bias_s[tid] = R.bias_v;
        for (int idx = tid + SPATIAL_NT; idx < a.C_pad; idx += SPATIAL_NT) L.bias_s[idx] = (a.bias && idx < a.C) ? a.bias[idx] : 0.f;
    }
}

// Inverse H-axis step for this row: s1[o][2kx(+1)] = sum_j spec[b][j][kx][o] * conj(twH[j][h])
__device__ __forceinline__ void spatial_hstep(const SpatialDev& a, const SpatialLds& L, int b, int h, const SpatialLoads& R) {
    constexpr int MJ = SPATIAL_MJ;
    const int tid = threadIdx.x;
    const long long jstride = (long long)a.m2c * a.C;
    float twx[MJ], twy[MJ];   // broadcast the lane-held twiddles (every lane is active here)
#pragma unroll
    for (int j = 0; j < MJ; ++j) { twx[j] = __shfl(R.twl.x, j, 16); twy[j] = __shfl(R.twl.y, j, 16); }
    for (int idx = tid; idx < a.C_pad * (a.NP / 2); idx += SPATIAL_NT) {
        const int kx = idx / a.C_pad, o = idx - kx * a.C_pad;
        float re = 0.f, im = 0.f;
        if (idx == tid) {   // first chunk: operands already in registers
#pragma unroll
            for (int j = 0; j < MJ; ++j) {
                if (j < a.m1) {
                    re += R.sv[j].x * twx[j] + R.sv[j].y * twy[j];   // v * conj(t)
                    im += R.sv[j].y * twx[j] - R.sv[j].x * twy[j];
                }
            }
        }
        if (kx < a.m2c && o < a.C) {
            const float2* sp2 = a.spec + (((long long)b * a.m1) * a.m2c + kx) * a.C + o;
            for (int j = (idx == tid ? MJ : 0); j < a.m1; ++j) {
                const float2 v = sp2[j * jstride];
                const float2 t = a.twH[j * a.H + h];
                re += v.x * t.x + v.y * t.y;
                im += v.y * t.x - v.x * t.y;
            }
        }
        const bool ok = kx < a.m2c && o < a.C;
        L.s1[o * L.LDS1 + 2 * kx] = ok ? re : 0.f;
        L.s1[o * L.LDS1 + 2 * kx + 1] = ok ? im : 0.f;
    }
}

// Main concatenated-K GEMM of wave w (0-3): acc[o][w] = sum_i ks[o][i] tin[i][w] + sum_n s1[o][n] gs[n][w], epilogue into tout_s
template <int NCB, int NBN, int MODE>
__device__ __forceinline__ void spatial_gemm(const SpatialDev& a, const SpatialLds& L, int w) {
    const int lane = lane_id(), r = lane & 15, g = lane >> 4;
    const int nwb = a.W / 16, LDP = L.LDP;
    for (int wb = w; wb < nwb; wb += 4) {
        f32x4 acc[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < NCB; ++kc) {
            f32x4 b4;
#pragma unroll
            for (int s = 0; s < 4; ++s) b4[s] = L.tin_s[(kc * 16 + 4 * g + s) * LDP + wb * 16 + r];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const f32x4 a4 = *reinterpret_cast<const f32x4*>(&L.ks[(cb * 16 + r) * L.LDK + kc * 16 + 4 * g]);
                acc[cb] = mfma16_chunk(a4, b4, acc[cb]);
            }
        }
#pragma unroll
        for (int nc = 0; nc < NBN; ++nc) {
            f32x4 b4;
#pragma unroll
            for (int s = 0; s < 4; ++s) b4[s] = L.gs[(nc * 16 + 4 * g + s) * LDP + wb * 16 + r];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const f32x4 a4 = *reinterpret_cast<const f32x4*>(&L.s1[(cb * 16 + r) * L.LDS1 + nc * 16 + 4 * g]);
                acc[cb] = mfma16_chunk(a4, b4, acc[cb]);
            }
        }
        // epilogue: operands for all elements are fetched first, then applied (no per-element waits / branches)
        float ep[NCB][4];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = cb * 16 + 4 * g + j, x = wb * 16 + r;
                ep[cb][j] = MODE == 0 ? L.bias_s[o] : (MODE == 1 ? L.pprev_s[o * LDP + x] : 0.f);
            }
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            f32x4 v4 = acc[cb];
            const f32x4 e4 = f32x4{ep[cb][0], ep[cb][1], ep[cb][2], ep[cb][3]};
            if (MODE == 0) v4 += e4;
            else if (MODE == 1) v4 *= gelu_grad4(e4);              // packed fp32 polynomial
#pragma unroll
            for (int j = 0; j < 4; ++j) L.tout_s[(cb * 16 + 4 * g + j) * LDP + wb * 16 + r] = v4[j];
        }
    }
}

// tout_s to `out`, then the next stage's row DFT on it (per-wave partials into x1s; store_x1 sums them behind a barrier)
template <int NCB, int NBN>
__device__ __forceinline__ void spatial_out_dft(const SpatialDev& a, const SpatialLds& L, int b, int h) {
    const int W4 = a.W / 4;
    for (int idx = threadIdx.x; idx < a.C * W4; idx += SPATIAL_NT) {
        const int c = idx / W4, x4 = idx % W4;
        *reinterpret_cast<float4*>(&a.out[(((long long)b * a.C + c) * a.H + h) * a.W + 4 * x4]) =
            *reinterpret_cast<const float4*>(&L.tout_s[c * L.LDP + 4 * x4]);
    }
    DLWP_STAMP(8);
    if (a.x1_out) tile_rows_dft<NCB, NBN>(L.tout_s, L.ft, L.x1s, L.LDP, a.NP, a.W / 16, a.x1_act != 0);
}

// The backward's by-products (skip-weight and bias gradient) are formed per kernel; only how an element leaves is shared.
// Slab of this workgroup: {g_wskip[C*C], g_bias[C]} partials, stride C*C+C padded to 4
__device__ __forceinline__ long long spatial_slab_off(const SpatialDev& a) {
    return (long long)blockIdx.x * (((long long)a.C * a.C + a.C + 3) & ~3LL);
}
// element `e` of the slab becomes old + v (old: its running partial across net calls, 0.f on a first call); without a slab v is
// added to *dst with a float atomic (all workgroups hit the same words: slow, API path only)
__device__ __forceinline__ void spatial_flush(const SpatialDev& a, long long e, float* dst, float old, float v) {
    if (a.gslab) a.gslab[e] = old + v;
    else atomic_add_f32(dst, v);
}

// MODE 0: forward (+bias); 1: backward with GELU' of the block input; 2: backward, input was not activated
template <int NCB, int NBN, int MODE>
__global__ __launch_bounds__(256) void fno_spatial_kernel(SpatialDev a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const SpatialLds L = carve_spatial_lds<false>(smem, a);
    const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
    const int r = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
    const int nwb = a.W / 16;
    const bool need_prev = a.is_bwd && (a.act_prev || a.g_wskip || a.gslab);
    DLWP_SPAN_BEGIN();
    DLWP_STAMP(0);
    SpatialLoads R;
    spatial_issue<MODE>(a, b, h, need_prev, R);
    // running partials of this workgroup's gradient slab (read-modify-write across net calls): fetched here, with every
    // other input, instead of in front of the final store (a dependent global round trip at the very end of the kernel)
    constexpr int SLQ = 4;
    float slab_old[SLQ], slab_b_old = 0.f;
#pragma unroll
    for (int k = 0; k < SLQ; ++k) slab_old[k] = 0.f;
    const long long slab_off = spatial_slab_off(a);
    const bool slab_acc = a.is_bwd && a.gslab && a.gslab_accumulate;
    if (slab_acc) {
#pragma unroll
        for (int k = 0; k < SLQ; ++k) slab_old[k] = a.gslab[slab_off + min(tid + 256 * k, a.C * a.C - 1)];
        slab_b_old = a.gslab[slab_off + a.C * a.C + min(tid, a.C - 1)];
    }
    DLWP_STAMP(1);
    spatial_commit<MODE>(a, L, b, h, need_prev, R);
    DLWP_STAMP(3);
    spatial_hstep(a, L, b, h, R);
    DLWP_STAMP(4);
    __syncthreads();   // 1: tin_s, pprev_s, gs, ks, s1 complete
    DLWP_STAMP(5);
    spatial_gemm<NCB, NBN, MODE>(a, L, w);
    DLWP_STAMP(6);
    __syncthreads();   // 2: tout_s complete; gs / ks / s1 dead
    DLWP_STAMP(7);
    spatial_out_dft<NCB, NBN>(a, L, b, h);
    DLWP_STAMP(9);

    // by-products, behind the chain on the same four waves: from LDS, the partial tiles over the dead GEMM operands
    if (a.is_bwd && (a.g_wskip || a.gslab)) {
        // gK[o][i] += sum_w g_pre[o][w] * act(x)[i][w]
        f32x4 kacc[NCB][NCB];
#pragma unroll
        for (int ob = 0; ob < NCB; ++ob)
#pragma unroll
            for (int ib = 0; ib < NCB; ++ib) kacc[ob][ib] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kc = w; kc < nwb; kc += 4) {
#pragma unroll
            for (int ib = 0; ib < NCB; ++ib) {
                f32x4 b4 = *reinterpret_cast<const f32x4*>(&L.pprev_s[(ib * 16 + r) * L.LDP + kc * 16 + 4 * g]);
                if (a.act_prev) {
                    b4 = gelu4(b4);
                }
#pragma unroll
                for (int ob = 0; ob < NCB; ++ob) {
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(&L.tin_s[(ob * 16 + r) * L.LDP + kc * 16 + 4 * g]);
                    kacc[ob][ib] = mfma16_chunk(a4, b4, kacc[ob][ib]);
                }
            }
        }
#pragma unroll
        for (int ob = 0; ob < NCB; ++ob)
#pragma unroll
            for (int ib = 0; ib < NCB; ++ib)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    L.gks[((w * NCB + ob) * 16 + 4 * g + j) * a.C_pad + ib * 16 + r] = kacc[ob][ib][j];
    }
    DLWP_STAMP(10);
    __syncthreads();   // 3: x1s and the gK partials complete
    DLWP_STAMP(11);
    if (a.x1_out) store_x1<SPATIAL_NT>(L.x1s, a.x1_out, b, h, a.H, a.m2c, a.C, a.C_pad, a.NP);
    if (a.is_bwd && (a.g_wskip || a.gslab)) {
        int kq = 0;
        for (int idx = tid; idx < a.C * a.C; idx += 256, ++kq) {
            const int o = fastdiv(idx, a.dC), i = idx - o * a.C;
            float v = 0.f;
#pragma unroll
            for (int w2 = 0; w2 < 4; ++w2) v += L.gks[(w2 * a.C_pad + o) * a.C_pad + i];
            float old = 0.f;
            if (slab_acc) {
                old = kq == 0 ? slab_old[0] : kq == 1 ? slab_old[1] : kq == 2 ? slab_old[2] : kq == 3 ? slab_old[3]
                                                                                                        : a.gslab[slab_off + idx];
            }
            spatial_flush(a, slab_off + idx, &a.g_wskip[idx], old, v);
        }
    }
    if (a.is_bwd && (a.g_bias || a.gslab) && tid < a.C) {
        float s = 0.f;
        for (int x = 0; x < a.W; ++x) s += L.tin_s[tid * L.LDP + x];
        spatial_flush(a, slab_off + a.C * a.C + tid, &a.g_bias[tid], slab_b_old, s);
    }
    DLWP_STAMP(12);
    DLWP_SPAN_END();
}

// Backward `spatial` (MODE 1 / 2 with a gradient destination) as TWO ROLES in one workgroup of eight waves.  The by-products of
// the backward pass -- skip-weight gradient, bias gradient -- feed neither `out` nor `x1_out` and depend only on tin_s / pprev_s,
// which are complete at the first barrier; in fno_spatial_kernel they run behind the row DFT on the same four waves (one wave per
// SIMD, nothing to hide a wait behind) and the next launch of the chain waits for them.  Here
//   role A, waves 0-3: the chain.  The phase functions fno_spatial_kernel calls, in the same order between the same three
//           barriers: same mapping and same arithmetic by construction (need_prev is always true here, and there is no bias).
//   role B, waves 4-7: the by-products.  While role A stages (up to barrier 1, where the SIMDs mostly wait for global memory):
//           the old slab values, and the four per-wave partial tiles of gK -- its MFMA fragments are 16 contiguous bytes of a row
//           of `tin` / `pprev`, so they are read straight from global memory -- into an LDS region of their own (gks cannot alias
//           gs / ks / s1 here: role A is filling them).  Between barriers 1 and 2, next to the main GEMM: the cross-wave sum,
//           the bias row sums from tin_s, the slab write / atomics.  Then it only arrives at barriers 2 and 3.
// All eight waves meet at the same three barriers, on every path: each is at the top level of the kernel.  Role A's count is that
// of fno_spatial_kernel.  (Measured, profiles/r08_experiments.md: with role B's GEMM next to the main GEMM both slow down -- MFMA
// and VALU of one SIMD do not overlap -- and a dependent chain of additions next to MFMAs waits for one MFMA per addition.)
// The by-products are bit for bit those of fno_spatial_kernel: partial w2 is one mfma16_chunk chain from zero over the chunks
// kc = w2, w2 + 4, ... of the same values; the partials are summed w2 = 0 .. 3 from 0.f, then old + v; the bias gradient is the
// sequential sum over x = 0 .. W-1 from 0.f (16-byte LDS reads), then old + s.
template <int NCB, int NBN, int MODE>
__global__ __launch_bounds__(512) void fno_spatial_roles_kernel(SpatialDev a) {
    static_assert(MODE == 1 || MODE == 2, "backward modes only");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr bool ROLE_B = true;
#include "fno_spatial_roles_head.inc.h"

    if (role_a) {
        spatial_out_dft<NCB, NBN>(a, L, b, h);
        DLWP_STAMP(9);
    }
    // 3: x1s complete
    if (role_a) __syncthreads(); else __builtin_amdgcn_s_barrier();
    DLWP_STAMP(11);
    if (role_a && a.x1_out) store_x1<NTA>(L.x1s, a.x1_out, b, h, a.H, a.m2c, a.C, a.C_pad, a.NP);
    DLWP_STAMP(12);
    DLWP_STAMP_WAVE(24);
    DLWP_SPAN_END();
}

// Block 0's backward `spatial` and the lifting MLP's backward as ONE launch.  On 64-wide rows a `spatial` workgroup (one image row
// (b, h)) and a pwmlp_bwd workgroup (64 consecutive pixels of one sample) are the same pixels under the same blockIdx, and the
// gradient of h0 between them has no other reader: the row that role A finishes in tout_s[C_pad][W + 4] IS the gys[Cout_pad][PT + 4]
// tile the lifting backward stages first, so the tensor is neither stored nor loaded again and one kernel boundary goes.
//   phase 1: the two-role workgroup above up to its second barrier -- the same text (fno_spatial_roles_head.inc.h), so the same
//            thread-to-element mapping, sum orders and slab layout; `out` is not written and there is no fused row DFT.
//   phase 2: the body of pwmlp_bwd_kernel<NIB, NCB, 8> -- the same text (pwmlp_bwd_body.inc.h) -- on all eight waves with gys =
//            tout_s.  Its part 1, the loads that do not depend on phase 1 (each wave's first weight fragments, each thread's unit
//            of the input tile through the pointer table), is issued in front of phase 1 (25.2 -> 24.6 us at the headline shape).  Its input tile and the gx partial tiles lie behind tout_s, over regions of phase 1 that are dead after the
//            second barrier (pprev_s, ft, x1s, gs, ks, s1, gks), so the launch needs no more LDS than the larger of its phases.
// Same row, same blockIdx, hence the same skip-weight slab and the same lifting slab as the two launches: every output is bit for
// bit theirs.  MODE is 2: the input of block 0 is the lifting MLP's output, which is not activated.
// ROLE_B == false: phase 1 without role B's work, for a sweep whose per-mode launch has formed the by-products of block 0
// (fno_mix_bwd_skipgrad_kernel); waves 4-7 then only arrive at the two barriers of phase 1.
struct SpatialLiftDev {
    SpatialDev s;
    BwdArgs m;
};
template <int NCB, int NBN, int NIB, bool ROLE_B = true>
__global__ __launch_bounds__(512) void fno_spatial_lift_bwd_kernel(SpatialLiftDev f) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NOB = NCB, NW = 8;
    // three channel tiles with two input tiles hold 256 VGPRs as it is: the early loads would spill (4 VGPRs, 20 bytes of scratch)
    constexpr bool PWMLP_BWD_EARLY = !(NCB == 3 && NIB == 2);
    const BwdArgs& a = f.m;
#define PWMLP_BWD_FUSED
#define PWMLP_BWD_PART 1
#include "pwmlp_bwd_body.inc.h"
#undef PWMLP_BWD_PART
    {
        constexpr int MODE = 2;
        const SpatialDev& a = f.s;
#include "fno_spatial_roles_head.inc.h"
    }
#define PWMLP_BWD_PART 2
#include "pwmlp_bwd_body.inc.h"
#undef PWMLP_BWD_PART
#undef PWMLP_BWD_FUSED
    DLWP_SPAN_END();
}

// The launch above with a THIRD phase: the scalar-output projection backward of the PREVIOUS net call (pwmlp_bwd_kernel<NCB, 0, 8>,
// the next launch of the rollout's backward chain) on the same 64-pixel row under the same blockIdx.  Of this launch it needs only
// its own row of the closed-loop gradient: the rows of g_out that phase 2 of this very workgroup has just accumulated through the
// pointer table -- no other workgroup touches them.  Everything else it reads (`pre` of the previous call's last block, the
// projection weights, prediction and target) was finished by earlier launches; what it writes (its row of the gradient of that
// `pre`, its row of x1, its projection slab) has no reader in this launch except, where the gradient buffer is also this launch's
// g_pre, the same workgroup's phase 1, long past.
//   phases 1, 2: the text of fno_spatial_lift_bwd_kernel.
//   phase 3: the whole text of pwmlp_bwd_body.inc.h once more, in the stand-alone form: gy staging (closed-loop gradient + MSE
//            term), main loop, gx, adjoint rows DFT into x1.  Its LDS is carved from the start of smem, over the regions of
//            phase 2, behind one workgroup barrier (PWMLP_BWD_BEHIND) that also orders this workgroup's g_out stores in front of
//            their staging; each wave's first weight fragments and the DFT table are requested in front of that barrier (when
//            phase 2 has finished: not in front of phases 1 and 2, and the x tile not at all ahead of its staging).
// Same text, same row, same blockIdx: every output is bit for bit that of the two launches.
struct SpatialLiftProjDev {
    SpatialDev s;
    BwdArgs m, q;
};
template <int NCB, int NBN, int NIBL, bool ROLE_B = true>
__global__ __launch_bounds__(512) void fno_spatial_lift_proj_bwd_kernel(SpatialLiftProjDev f) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    {
        constexpr int NIB = NIBL, NOB = NCB, NW = 8;
        constexpr bool PWMLP_BWD_EARLY = true;      // instantiated for NCB <= 2 only
        const BwdArgs& a = f.m;
#define PWMLP_BWD_FUSED
#define PWMLP_BWD_PART 1
#include "pwmlp_bwd_body.inc.h"
#undef PWMLP_BWD_PART
        {
            constexpr int MODE = 2;
            const SpatialDev& a = f.s;
#include "fno_spatial_roles_head.inc.h"
        }
#define PWMLP_BWD_PART 2
#include "pwmlp_bwd_body.inc.h"
#undef PWMLP_BWD_PART
#undef PWMLP_BWD_FUSED
    }
    {
        constexpr int NIB = NCB, NOB = 0, NW = 8;
        const BwdArgs& a = f.q;
#define PWMLP_BWD_BEHIND
#include "pwmlp_bwd_body.inc.h"
#undef PWMLP_BWD_BEHIND
    }
    DLWP_SPAN_END();
}

// The last block's forward `spatial` and the projection MLP (chained, as in pwmlp_fwd_chain_kernel, with the next net call's lifting
// MLP and its rows DFT; NOB2 == 0: projection only) as ONE launch of 16 waves.  On 64-wide rows a `spatial` workgroup (one image row
// (b, h)) and a pointwise-MLP workgroup (64 consecutive pixels of one sample) are the same pixels under the same blockIdx: the row
// that spatial_gemm finishes in tout_s[C_pad][W + 4] IS the xs[Cin_pad][PT + 4] tile the projection stages first, in place.  `pre` of
// the last block is still written (the projection backward reads it) but not read back, one kernel boundary goes, and the MLPs'
// prologue -- two weight sets, about 100 KB of LDS images -- runs next to the `spatial` chain instead of behind it.
//   phase 1: waves 0-3 run the forward chain of fno_spatial_kernel<NCB, NBN, 0> (the same phase functions in the same order on the
//            same 256 threads, so every sum keeps its order; no pprev, no fused row DFT); waves 4-15 meanwhile request and commit the
//            weights and biases of the MLP(s) and the lifting input tile (768 threads share those loops: NTB, T0).
//   hand-over: tout_s = P.xs.  Its rows c >= C hold +0.f, which is what stage_pixels puts there: for such a row ks and s1 are zero
//            (zero_padding of ks up to C_pad rows; spatial_hstep writes 0.f for o >= C) and so is bias_s, so the accumulator is a
//            sum of (+-0) products from +0.f, plus 0.f.  `pre` leaves through spatial_out_dft's store loop.
//   phase 2: the sequence of pwmlp_fwd_chain_kernel / pwmlp_fwd_kernel behind its staging, on all 16 waves.
// Every barrier is at the top level and all 16 waves reach each of them.  The operands of the `spatial` GEMM lie behind the MLP
// images (20 KB at the headline shape: 160,320 bytes in all).
struct SpatialProjDev {
    SpatialDev s;
    ChainArgs c;
};
template <int NCB, int NBN, int NOB2>
__global__ __launch_bounds__(1024) void fno_spatial_proj_fwd_kernel(SpatialProjDev f) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NW = FWD_WAVES, HQ = NW / 4, T0 = SPATIAL_NT, NTB = NW * 64 - SPATIAL_NT;
    static_assert(NW * 64 == 1024 && 16 * (PT / 4) == SPATIAL_NT, "waves 0-3 hold the DFT table of fwd_finish");
    const SpatialDev& a = f.s;
    const ChainArgs& c = f.c;
    const FwdLds P = fwd_carve(smem, c.p, nullptr);
    float* behind = P.outs + HQ * c.p.Cout_pad * LDP;
    FwdLds Lq = P;
    if constexpr (NOB2 != 0) {     // second MLP: its partial tiles alias the first one's W1 image (dead by then)
        Lq = fwd_carve(behind, c.l, P.w1s);
        behind = Lq.b2s + c.l.Cout_pad;
    }
    SpatialLds S;
    S.LDP = a.W + 4; S.LDK = a.C_pad + 4; S.LDS1 = a.NP + 4;
    S.tout_s = P.xs;
    S.tin_s = behind;
    S.gs = S.tin_s + a.C_pad * S.LDP;
    S.ks = S.gs + a.NP * S.LDP;
    S.s1 = S.ks + a.C_pad * S.LDK;
    S.bias_s = S.s1 + a.C_pad * S.LDS1;
    S.pprev_s = S.ft = S.x1s = S.gks = nullptr;
    const int w = wave_id();
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H, p0 = h * PT;
    float4 ftv = make_float4(0.f, 0.f, 0.f, 0.f);      // DFT table of the lifting MLP's fused rows step: threads 0 .. 255
    if (w < 4) {
        SpatialLoads R;
        spatial_issue<0>(a, b, h, false, R);
        if constexpr (NOB2 != 0) if (c.l.x1_out) ftv = reinterpret_cast<const float4*>(c.l.FT)[threadIdx.x];
        spatial_commit<0>(a, S, b, h, false, R);
        spatial_hstep(a, S, b, h, R);
    } else {
        FwdLoadsT<3> qp, ql;
        fwd_issue<NTB, T0>(c.p, qp);
        if constexpr (NOB2 != 0) {
            fwd_issue<NTB, T0>(c.l, ql);
            stage_pixels<NTB, T0>(Lq.xs, c.l.x, b, c.l.Cin, c.l.Cin_pad, p0, c.l.P, c.l.vec_x != 0, c.skip);
        }
        fwd_commit<NTB, T0>(c.p, P, qp);
        if constexpr (NOB2 != 0) fwd_commit<NTB, T0>(c.l, Lq, ql);
    }
    __syncthreads();   // 1: the operands of the `spatial` GEMM and every MLP image but P.xs complete
    if (w < 4) spatial_gemm<NCB, NBN, 0>(a, S, w);
    __syncthreads();   // 2: tout_s = P.xs complete
    if (w < 4) spatial_out_dft<NCB, NBN>(a, S, b, h);      // `pre` (a.x1_out is NULL: no row DFT here)
    fwd_compute<1, NW>(c.p, P);
    __syncthreads();   // 3
    fwd_finish<1, NW>(c.p, P, make_float4(0.f, 0.f, 0.f, 0.f), b, p0, h, NOB2 != 0 ? Lq.xs : nullptr, c.next_ch);
    if constexpr (NOB2 != 0) {
        __syncthreads();   // 4
        fwd_compute<NOB2, NW>(c.l, Lq);
        __syncthreads();   // 5
        fwd_finish<NOB2, NW>(c.l, Lq, ftv, b, p0, h);
    }
}

// ------------------------------------------------------------------------------------------
// Per-mode stage.  One 512-thread workgroup per kept mode (j,kx).  Everything it reads is issued
// as batched independent loads up front (the mode's [C][C] weight slice as 16-byte loads straight
// into an LDS image with a +1 complex row pad, the twiddle row, then the x1 column in unrolled
// groups of 8), because at these sizes the kernel is pure load latency.
constexpr int MIXT = 512;

struct MixDev {
    const float2* x1; const float2* wspec; const float2* xhat_in; float2* xhat; float2* y;
    float2* g_wspec; const float2* twH;
    int B, C, H, m1, m2c;
    FastDiv dC, dBC, dBC2;   // exact division by C, B*C, B*C/2 without the ~40-instruction integer divide
};

// H-axis step, fast path (C even): every thread owns TWO adjacent channels (one 16-byte load per image row) and
// the rows h = hs, hs+HS, ...; loads are issued in batches of 8 BEFORE the twiddles are needed, so the weight
// slice, the twiddle row and the first x1 batch share one global-memory latency.
struct HstepLoads {
    float4 v[8];
    int bc2, hs, b, c, nh;
};
__device__ __forceinline__ void mix_hstep_issue(const MixDev& a, int kx, int HS, HstepLoads& L, int h0) {
    const int BC2 = a.B * a.C / 2;
    const int u = threadIdx.x;
    L.hs = fastdiv(u, a.dBC2); L.bc2 = u - L.hs * BC2;
    L.b = fastdiv(2 * L.bc2, a.dC); L.c = 2 * L.bc2 - L.b * a.C;
    const bool act = u < BC2 * HS;
    const float2* src = a.x1 + (((long long)L.b * a.H) * a.m2c + kx) * a.C + L.c;
    const long long hstride = (long long)a.m2c * a.C;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int h = h0 + L.hs + q * HS;
        const int hc = (act && h < a.H) ? h : 0;                       // clamped: always a valid address
        L.v[q] = *reinterpret_cast<const float4*>(src + hc * hstride);
    }
}
__device__ __forceinline__ void mix_hstep_accum(const MixDev& a, int HS, const HstepLoads& L, const float2* tws, int h0,
                                                float2& s0, float2& s1) {
    float2 tq[8];   // all LDS reads first: at this occupancy a read-then-use loop pays the LDS latency per iteration
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int h = h0 + L.hs + q * HS;
        tq[q] = tws[h < a.H ? h : 0];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int h = h0 + L.hs + q * HS;
        if (h < a.H) {
            const float2 t = tq[q];
            s0.x += L.v[q].x * t.x - L.v[q].y * t.y;
            s0.y += L.v[q].x * t.y + L.v[q].y * t.x;
            s1.x += L.v[q].z * t.x - L.v[q].w * t.y;
            s1.y += L.v[q].z * t.y + L.v[q].w * t.x;
        }
    }
}
// whole fast H-step after the first batch has been issued; returns the number of partial slots
__device__ __forceinline__ int mix_hstep_fast(const MixDev& a, int kx, int HS, HstepLoads& L, const float2* tws, float2* part) {
    const int BC = a.B * a.C, BC2 = BC / 2;
    float2 s0 = make_float2(0.f, 0.f), s1 = s0;
    mix_hstep_accum(a, HS, L, tws, 0, s0, s1);
    for (int h0 = 8 * HS; h0 < a.H; h0 += 8 * HS) {
        mix_hstep_issue(a, kx, HS, L, h0);
        mix_hstep_accum(a, HS, L, tws, h0, s0, s1);
    }
    if ((int)threadIdx.x < BC2 * HS) {
        part[L.hs * BC + 2 * L.bc2] = s0;
        part[L.hs * BC + 2 * L.bc2 + 1] = s1;
    }
    return HS;
}

// H-axis step into LDS partials (generic path): part[hs][b*C+c] = sum_{h = hs mod HS} x1[b][h][kx][c] * tw[h]; returns HS
__device__ __forceinline__ int mix_hstep(const MixDev& a, int kx, const float2* tws, float2* part, int HS) {
    const int BC = a.B * a.C;
    for (int u = threadIdx.x; u < BC * HS; u += MIXT) {
        const int hs = fastdiv(u, a.dBC), bc = u - hs * BC, b = fastdiv(bc, a.dC), c = bc - b * a.C;
        const float2* src = a.x1 + (((long long)b * a.H) * a.m2c + kx) * a.C + c;
        const long long hstride = (long long)a.m2c * a.C;
        float re = 0.f, im = 0.f;
#pragma unroll 8
        for (int h = hs; h < a.H; h += HS) {
            const float2 v = src[h * hstride];
            const float2 t = tws[h];
            re += v.x * t.x - v.y * t.y;
            im += v.x * t.y + v.y * t.x;
        }
        part[hs * BC + bc] = make_float2(re, im);
    }
    return HS;
}

// out[i] = sum_s part[s][i]
__device__ __forceinline__ void mix_fold(float2* out, const float2* part, int n, int ns) {
    for (int i = threadIdx.x; i < n; i += MIXT) {
        float2 v = make_float2(0.f, 0.f);
        for (int s0 = 0; s0 < ns; s0 += 8) {
            float2 p[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) p[q] = part[(s0 + q < ns ? s0 + q : 0) * n + i];
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (s0 + q < ns) { v.x += p[q].x; v.y += p[q].y; }
        }
        out[i] = v;
    }
}

// partial slots of the fast H-step: threads / (B*C/2), clamped to [1, H]
__device__ __host__ __forceinline__ int mix_slots2(int B, int C, int H) {
    const int bc2 = B * C / 2;
    int s = bc2 > 0 ? MIXT / bc2 : 1;
    if (s < 1) s = 1;
    if (s > H) s = H;
    return s;
}
// number of partial slots a phase splits its reduction over (threads / outputs, clamped)
__device__ __host__ __forceinline__ int mix_split(int outputs, int limit) {
    int s = MIXT / outputs;
    if (s < 1) s = 1;
    if (s > limit) s = limit;
    return s;
}

// ---- the per-mode complex channel contraction on the matrix cores (exact-f32 v_mfma_f32_16x16x4_f32).
// A complex product y[b][o] = sum_i x[b][i] w[i][o] is ONE real GEMM with the real and imaginary planes of the SAMPLE side
// stacked along M and the (re, im) pair of the weight interleaved along K:
//     rows (b, re) = [ xr_i, -xi_i ]_i      rows (b, im) = [ xi_i, xr_i ]_i      B[k = 2i + ri][n = o] = w[i][o][ri]
// => 8 B C^2 flops, every weight element used exactly once, M = 2 B rows (8 of the 16 tile rows at the headline batch of 4;
// full at B >= 8).  The same scheme gives the backward products: gx = ghat conj(w)^T (B[k = 2o + ri][n = i] = w[i][o][ri])
// and the weight gradient gw[i][o] += sum_b conj(xhat[b][i]) ghat[b][o] (K = 2 B: one 16x16x4 instruction per pair of samples).
// Weight operand: narrow layers (C <= 64) stage the mode's [C][C] slice in LDS with ONE 16-byte load per thread, in flight
// together with the x1 loads of the H-axis step (rows padded by one complex number: conflict-free 8-byte fragment reads along
// rows and columns); wide layers read every fragment once, straight from global memory / L2 into registers (two 8-byte loads
// per 16-deep K chunk, 128 contiguous bytes per 16 lanes) -- a 217-channel slice is 377 KB and is used once per workgroup.

// weight slice [C][C] complex -> LDS rows of (C+1) complex
__device__ __forceinline__ void mix_stage_w(const float2* wm, float2* ws, int C, FastDiv dC) {
    const int n2 = C * C / 2;  // pairs of complex numbers (C*C is even whenever C is even)
    if ((C & 1) == 0) {
#pragma unroll 4
        for (int u = threadIdx.x; u < n2; u += MIXT) {
            const float4 v = reinterpret_cast<const float4*>(wm)[u];
            const int e = 2 * u, i = fastdiv(e, dC), o = e - i * C;
            ws[i * (C + 1) + o] = make_float2(v.x, v.y);
            ws[i * (C + 1) + o + 1] = make_float2(v.z, v.w);
        }
    } else {
#pragma unroll 4
        for (int e = threadIdx.x; e < C * C; e += MIXT) ws[(e / C) * (C + 1) + e % C] = wm[e];
    }
}

// A fragment of chunk kc for tile row m = 16 mt + r: element s <-> k = 16 kc + 4 g + s, complex index i = 8 kc + 2 g + s / 2.
// CONJ = 0: rows (b, re) = (x, -y), (b, im) = (y, x)      [x * w]
// CONJ = 1: rows (b, re) = (x, y),  (b, im) = (y, -x)     [x * conj(w)]
template <int CONJ>
__device__ __forceinline__ f32x4 mix_afrag(const float2* xh, int B, int C, int mt, int kc, int r, int g) {
    const int m = 16 * mt + r, b = m >> 1, part = m & 1, i0 = 8 * kc + 2 * g;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (b < B) {
        const float2 v0 = i0 < C ? xh[b * C + i0] : make_float2(0.f, 0.f);
        const float2 v1 = i0 + 1 < C ? xh[b * C + i0 + 1] : make_float2(0.f, 0.f);
        if (CONJ == 0) a = part ? f32x4{v0.y, v0.x, v1.y, v1.x} : f32x4{v0.x, -v0.y, v1.x, -v1.y};
        else a = part ? f32x4{v0.y, -v0.x, v1.y, -v1.x} : f32x4{v0.x, v0.y, v1.x, v1.y};
    }
    return a;
}
// B fragment of chunk kc for tile column n = 16 nt + r from a [C][pitch] complex image (LDS: pitch C + 1; global: pitch C).
// TRW = 0: w[i = 8 kc + 2 g (+1)][o = n]; TRW = 1: w[i = n][o = 8 kc + 2 g (+1)].  Loads are unconditional from clamped
// addresses (selects afterwards), so that a group of them is in flight together.
template <int TRW>
__device__ __forceinline__ f32x4 mix_bfrag(const float2* wm, int pitch, int C, int nt, int kc, int r, int g) {
    const int n = 16 * nt + r, k0 = 8 * kc + 2 * g;
    const int nc = n < C ? n : C - 1, k0c = k0 < C ? k0 : C - 1, k1c = k0 + 1 < C ? k0 + 1 : C - 1;
    const float2 w0 = TRW ? wm[(long long)nc * pitch + k0c] : wm[(long long)k0c * pitch + nc];
    const float2 w1 = TRW ? wm[(long long)nc * pitch + k1c] : wm[(long long)k1c * pitch + nc];
    const bool ok0 = n < C && k0 < C, ok1 = n < C && k0 + 1 < C;
    return f32x4{ok0 ? w0.x : 0.f, ok0 ? w0.y : 0.f, ok1 ? w1.x : 0.f, ok1 ? w1.y : 0.f};
}

// store one accumulator tile: rows 4g .. 4g+3 = samples 2g, 2g+1 (+ 8 mt), (re, im) each; column n = 16 nt + r
__device__ __forceinline__ void mix_store_tile(float2* out, long long ostride_b, const f32x4 acc, int B, int C, int nt, int mt,
                                               int r, int g) {
    const int n = 16 * nt + r, b0 = 8 * mt + 2 * g;
    if (n < C) {
        if (b0 < B) out[(long long)b0 * ostride_b + n] = make_float2(acc[0], acc[1]);
        if (b0 + 1 < B) out[(long long)(b0 + 1) * ostride_b + n] = make_float2(acc[2], acc[3]);
    }
}

// out[b][n] (complex, global, index base + n) = sum over the K chunks of A(xh) . B(w); work items = (column tile, pair of row
// tiles), dealt to the waves round-robin
template <int CONJ, int TRW>
__device__ __forceinline__ void mix_contract(const float2* xh, const float2* wm, int pitch, float2* out, long long ostride_b,
                                             int B, int C, int nt_begin = 0, int nt_end = 1 << 30) {
    const int lane = lane_id(), w = wave_id(), r = lane & 15, g = lane >> 4;
    constexpr int NW = MIXT / 64;
    const int nkc = (2 * C + 15) / 16, nmt = (2 * B + 15) / 16, nmp = (nmt + 1) / 2;
    const int ntn = min((C + 15) / 16, nt_end) - nt_begin;        // column tiles [nt_begin, nt_end) of this workgroup
    for (int item = w; item < ntn * nmp; item += NW) {
        const int nt = nt_begin + item % ntn, mt0 = 2 * (item / ntn);
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;     // two row tiles share every weight fragment (B > 8)
        for (int kc0 = 0; kc0 < nkc; kc0 += 4) {
            f32x4 bf[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) bf[q] = mix_bfrag<TRW>(wm, pitch, C, nt, min(kc0 + q, nkc - 1), r, g);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (kc0 + q < nkc) {
                    acc0 = mfma16_chunk(mix_afrag<CONJ>(xh, B, C, mt0, kc0 + q, r, g), bf[q], acc0);
                    if (mt0 + 1 < nmt) acc1 = mfma16_chunk(mix_afrag<CONJ>(xh, B, C, mt0 + 1, kc0 + q, r, g), bf[q], acc1);
                }
        }
        mix_store_tile(out, ostride_b, acc0, B, C, nt, mt0, r, g);
        if (mt0 + 1 < nmt) mix_store_tile(out, ostride_b, acc1, B, C, nt, mt0 + 1, r, g);
    }
}

// LDSW: the mode's weight slice is staged in LDS (narrow layers)
template <bool LDSW>
__global__ __launch_bounds__(MIXT) void fno_mix_fwd_kernel(MixDev a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int BC = a.B * a.C, C = a.C;
    const int NS = mix_split(BC, a.H < C ? a.H : C);   // partial slots of the generic H-step
    const int NS2 = mix_slots2(a.B, C, a.H);           // partial slots of the two-channels-per-thread H-step
    float2* xh = reinterpret_cast<float2*>(smem);  // [BC]
    float2* part = xh + BC;                        // [max(NS, NS2)][BC]
    float2* tws = part + (NS > NS2 ? NS : NS2) * BC;   // [H]
    float2* ws = tws + a.H;                        // [C][C+1]   (LDSW)
    // XCD-aware mode order: workgroups go round-robin to the 8 XCDs; give every XCD a contiguous range of (kx, j) so that
    // the m1 row frequencies of one column kx -- which read the same x1 slice -- meet in one L2
    int mode = blockIdx.x;
    {
        const int nm = gridDim.x, full = (nm / 8) * 8;
        if (mode < full) mode = (mode % 8) * (nm / 8) + mode / 8;
    }
    const int kx = mode / a.m1, j = mode - kx * a.m1;
    const bool fast = (C % 2 == 0) && (BC / 2) * NS2 <= MIXT && NS2 >= 1;
    const float2* wm = a.wspec + ((long long)(j * a.m2c + kx) * C) * C;
    DLWP_STAMP(16);
    HstepLoads hl;
    if (fast) mix_hstep_issue(a, kx, NS2, hl, 0);            // x1 loads in flight before anything is waited for
    if (LDSW) mix_stage_w(wm, ws, C, a.dC);
    for (int i = threadIdx.x; i < a.H; i += MIXT) tws[i] = a.twH[j * a.H + i];
    DLWP_STAMP(17);
    __syncthreads();
    DLWP_STAMP(18);
    const int hs = fast ? mix_hstep_fast(a, kx, NS2, hl, tws, part) : mix_hstep(a, kx, tws, part, NS);
    DLWP_STAMP(19);
    __syncthreads();
    DLWP_STAMP(20);
    mix_fold(xh, part, BC, hs);
    __syncthreads();
    DLWP_STAMP(21);
    const long long mofs = ((long long)j * a.m2c + kx) * C, bstr = (long long)a.m1 * a.m2c * C;
    for (int bc = threadIdx.x; bc < BC; bc += MIXT) {
        const int b = fastdiv(bc, a.dC), c = bc - b * C;
        a.xhat[b * bstr + mofs + c] = xh[bc];
    }
    if (LDSW) mix_contract<0, 0>(xh, ws, C + 1, a.y + mofs, bstr, a.B, C);
    else mix_contract<0, 0>(xh, wm, C, a.y + mofs, bstr, a.B, C);
    DLWP_STAMP(24);
}

// The per-mode backward workgroup: the whole of fno_mix_bwd_kernel, and the mode workgroups of fno_mix_bwd_skipgrad_kernel.
// The XCD-aware order below needs the workgroup's index among the mode workgroups and their count: blockIdx.x and gridDim.x in
// the first kernel (read where they always were: its instruction stream stays what it was), `block` and `nmodes` when HOSTED.
template <bool LDSW, bool HOSTED>
__device__ __forceinline__ void mix_bwd_body(const MixDev& a, const int block, const int nmodes) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int BC = a.B * a.C, C = a.C;
    const int NS = mix_split(BC, a.H < C ? a.H : C);
    const int NS2 = mix_slots2(a.B, C, a.H);
    float2* gh = reinterpret_cast<float2*>(smem);  // [BC]  ghat
    float2* xsv = gh + BC;                         // [BC]  saved xhat
    float2* part = xsv + BC;                       // [max(NS, NS2)][BC]
    float2* tws = part + (NS > NS2 ? NS : NS2) * BC;   // [H]
    float2* ws = tws + a.H;                        // [C][C+1]   (LDSW)
    int mode = HOSTED ? block : (int)blockIdx.x;
    {
        const int nm = HOSTED ? nmodes : (int)gridDim.x, full = (nm / 8) * 8;
        if (mode < full) mode = (mode % 8) * (nm / 8) + mode / 8;
    }
    const int kx = mode / a.m1, j = mode - kx * a.m1;
    const long long wofs = ((long long)(j * a.m2c + kx) * C) * C;
    const bool fast = (C % 2 == 0) && (BC / 2) * NS2 <= MIXT && NS2 >= 1;
    const float2* wm = a.wspec + wofs;
    HstepLoads hl;
    if (fast) mix_hstep_issue(a, kx, NS2, hl, 0);
    if (LDSW) mix_stage_w(wm, ws, C, a.dC);
    for (int i = threadIdx.x; i < a.H; i += MIXT) tws[i] = a.twH[j * a.H + i];
    const long long mofs = ((long long)j * a.m2c + kx) * C, bstr = (long long)a.m1 * a.m2c * C;
    for (int bc = threadIdx.x; bc < BC; bc += MIXT) {
        const int b = fastdiv(bc, a.dC), c = bc - b * C;
        xsv[bc] = a.xhat_in[b * bstr + mofs + c];
    }
    float2* gw = a.g_wspec + wofs;  // this workgroup owns the mode's weight-gradient slice
    __syncthreads();
    const int hs = fast ? mix_hstep_fast(a, kx, NS2, hl, tws, part) : mix_hstep(a, kx, tws, part, NS);
    __syncthreads();
    mix_fold(gh, part, BC, hs);
    __syncthreads();
    // gw[i][o] += sum_b conj(xhat[b][i]) ghat[b][o]: tile [16 i x 16 o], K = 2 B, k = 2 b' + ri on the lane group g.
    // Tiles are dealt from the LAST wave downwards and the gx column tiles below from the first wave upwards, so that at
    // narrow widths (4 + 2 work items for 8 waves) no wave gets both.
    {
        const int lane = lane_id(), w = wave_id(), r = lane & 15, g = lane >> 4;
        constexpr int NW = MIXT / 64;
        const int nt = (C + 15) / 16, ri = g & 1;
        for (int t = NW - 1 - w; t < nt * nt; t += NW) {
            const int it = t / nt, ot = t - it * nt;
            const int i = 16 * it + r, o = 16 * ot + r;          // A row (i) / B column (o) of this lane
            float2 old[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int io = min(16 * it + 4 * g + q, C - 1);
                old[q] = gw[(long long)io * C + min(o, C - 1)];
            }
            f32x4 are = {0.f, 0.f, 0.f, 0.f}, aim = {0.f, 0.f, 0.f, 0.f};
            for (int b0 = 0; b0 < a.B; b0 += 2) {
                const int b = b0 + (g >> 1);
                const bool okb = b < a.B;
                const float2 xv = (okb && i < C) ? xsv[b * C + i] : make_float2(0.f, 0.f);
                const float2 gv = (okb && o < C) ? gh[b * C + o] : make_float2(0.f, 0.f);
                const float av = ri ? xv.y : xv.x;
                are = mfma16(av, ri ? gv.y : gv.x, are);         // xr gr + xi gi
                aim = mfma16(av, ri ? -gv.x : gv.y, aim);        // xr gi - xi gr
            }
            if (o < C) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int io = 16 * it + 4 * g + q;
                    if (io < C) gw[(long long)io * C + o] = make_float2(old[q].x + are[q], old[q].y + aim[q]);
                }
            }
        }
    }
    // gx[b][i] = sum_o ghat[b][o] conj(w[i][o])
    if (LDSW) mix_contract<1, 1>(gh, ws, C + 1, a.y + mofs, bstr, a.B, C);
    else mix_contract<1, 1>(gh, wm, C, a.y + mofs, bstr, a.B, C);
}

template <bool LDSW>
__global__ __launch_bounds__(MIXT) void fno_mix_bwd_kernel(MixDev a) {
    mix_bwd_body<LDSW, false>(a, 0, 0);
}

// ---- the per-mode backward launch as host of the backward `spatial` by-products.  The skip-weight gradient gK and the bias
// gradient of block l need only g_pre of the block (`tin`) and its stored input (`pprev`), both complete before the block's
// per-mode launch starts, and feed nothing on the chain; the per-mode launch has one workgroup per kept mode (84 at the headline
// shape), so most CUs idle through it.  Here the launch has m1 * m2c + ceil(B * H / 2) workgroups:
//   blockIdx.x <  m1 * m2c : mix_bwd_body, unchanged (lowest indices: dispatched first)
//   the others             : TWO image rows each, rows 2 p and 2 p + 1 with p = blockIdx.x - m1 * m2c.  Waves 0-3 form the first
//                            row's gK partial and bias gradient into that row's slab, waves 4-7 the second row's: each half does
//                            what role B of fno_spatial_roles_kernel does for its row, with the same mapping of chunks to waves
//                            and of elements to threads, so every slab float is bit for bit role B's: partial w2 is one
//                            mfma16_chunk chain from zero over the chunks kc = w2, w2 + 4, ... on fragments read straight from
//                            global memory; the partials are summed w2 = 0 .. 3 from 0.f, then old + v; the bias gradient is the
//                            sequential sum over x = 0 .. W-1 from 0.f (read from global `tin`, the values tin_s holds), then
//                            old + s.
// Two rows per workgroup keep the launch at 212 workgroups for the headline's 256 rows, one per CU: with one row per workgroup
// (340 workgroups) mode and row workgroups shared CUs and the launch took 7.3 us instead of 6.1; with two it takes 6.4
// (profiles/r12_experiments.md).  The `spatial` launch behind it runs the chain alone.  No workgroup reads what another one of
// the launch writes.
struct SkipGradDev {
    const float* tin; const float* pprev; float* gslab;
    int gslab_accumulate, act_prev;
    int C, H, W, C_pad, nmodes, nrows;
    FastDiv dC;
};
struct MixSkipDev {
    MixDev m;
    SkipGradDev s;
};

template <int NCB>
__device__ __forceinline__ void skipgrad_rows(const SkipGradDev& a, float* smem, const int pair) {
    constexpr int NTB = 256;                      // threads of one half
    const int tid = threadIdx.x, lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(wave_id());   // wave-uniform: `live` and the loop bounds are scalar
    const int w2 = w & 3, half = w >> 2, tb = tid & (NTB - 1);
    const int r = lane & 15, g = lane >> 4;
    const int row = 2 * pair + half;
    const bool live = row < a.nrows;              // an odd row count leaves the last workgroup's second half idle
    const int b = row / a.H, h = row - b * a.H;
    const int W4 = a.W / 4, nwb = a.W / 16, CC = a.C * a.C;
    float* gks = smem + half * 4 * a.C_pad * a.C_pad;   // [4 waves][C_pad][C_pad] of this half
    const long long slab_off = (long long)row * (((long long)CC + a.C + 3) & ~3LL);   // spatial_slab_off of the row's index
    const bool slab_acc = a.gslab_accumulate != 0;
    constexpr int SLQ = 4;
    float slab_old[SLQ], slab_b_old = 0.f;
#pragma unroll
    for (int k = 0; k < SLQ; ++k) slab_old[k] = 0.f;
    const int bias_c = 4 * lane + w2;             // bias-gradient channel of this lane (lanes 0-15 of each wave)
    constexpr int BQ = 16;                        // ... its row pieces read ahead (a whole row at W = 64)
    const bool bias_on = live && lane < 16 && bias_c < a.C;
    float4 bq[BQ];
    const float4* brow = nullptr;
    if (live) {
        // ---- issue phase: the running partials of the row's slab, the bias rows, then the fragments of the first chunk
        if (slab_acc) {
#pragma unroll
            for (int k = 0; k < SLQ; ++k) slab_old[k] = a.gslab[slab_off + min(tb + NTB * k, CC - 1)];
            slab_b_old = a.gslab[slab_off + CC + min(bias_c, a.C - 1)];
        }
        brow = reinterpret_cast<const float4*>(a.tin + (((long long)b * a.C + min(bias_c, a.C - 1)) * a.H + h) * a.W);
        if (bias_on) {
#pragma unroll
            for (int q = 0; q < BQ; ++q) bq[q] = brow[min(q, W4 - 1)];
        }
        // gK partial of wave w2: sum over its 16-pixel chunks of g_pre[o][w] * act(x)[i][w]
        f32x4 kacc[NCB][NCB];
#pragma unroll
        for (int ob = 0; ob < NCB; ++ob)
#pragma unroll
            for (int ib = 0; ib < NCB; ++ib) kacc[ob][ib] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kc = w2; kc < nwb; kc += 4) {
            f32x4 ta[NCB], pb[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {   // clamped addresses, selects afterwards: all loads in flight together
                const int c = cb * 16 + r;
                const long long off = (((long long)b * a.C + min(c, a.C - 1)) * a.H + h) * a.W + kc * 16 + 4 * g;
                ta[cb] = *reinterpret_cast<const f32x4*>(&a.tin[off]);
                pb[cb] = *reinterpret_cast<const f32x4*>(&a.pprev[off]);
            }
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const bool ok = cb * 16 + r < a.C;
                ta[cb] = ok ? ta[cb] : f32x4{0.f, 0.f, 0.f, 0.f};
                pb[cb] = ok ? pb[cb] : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int ib = 0; ib < NCB; ++ib) {
                f32x4 b4 = pb[ib];
                if (a.act_prev) {
                    b4 = gelu4(b4);
                }
#pragma unroll
                for (int ob = 0; ob < NCB; ++ob) kacc[ob][ib] = mfma16_chunk(ta[ob], b4, kacc[ob][ib]);
            }
        }
#pragma unroll
        for (int ob = 0; ob < NCB; ++ob)
#pragma unroll
            for (int ib = 0; ib < NCB; ++ib)
#pragma unroll
                for (int j = 0; j < 4; ++j) gks[((w2 * NCB + ob) * 16 + 4 * g + j) * a.C_pad + ib * 16 + r] = kacc[ob][ib][j];
    }
    __syncthreads();   // the four gK partials of both rows complete
    if (!live) return;
    // cross-wave sum of the partials (w2 = 0 .. 3 from 0.f), then old + v into the slab: all LDS reads first, then the sums
    float pq[SLQ][4];
#pragma unroll
    for (int k = 0; k < SLQ; ++k) {
        const int idx = min(tb + NTB * k, CC - 1), o = fastdiv(idx, a.dC), i = idx - o * a.C;
#pragma unroll
        for (int q = 0; q < 4; ++q) pq[k][q] = gks[(q * a.C_pad + o) * a.C_pad + i];
    }
#pragma unroll
    for (int k = 0; k < SLQ; ++k) {
        const int idx = tb + NTB * k;
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) v += pq[k][q];
        if (idx < CC) a.gslab[slab_off + idx] = slab_old[k] + v;
    }
    for (int idx = tb + NTB * SLQ; idx < CC; idx += NTB) {
        const int o = fastdiv(idx, a.dC), i = idx - o * a.C;
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) v += gks[(q * a.C_pad + o) * a.C_pad + i];
        const float old = slab_acc ? a.gslab[slab_off + idx] : 0.f;
        a.gslab[slab_off + idx] = old + v;
    }
    if (bias_on) {
        float bias_sum = 0.f;
#pragma unroll
        for (int q = 0; q < BQ; ++q)
            if (q < W4) { bias_sum += bq[q].x; bias_sum += bq[q].y; bias_sum += bq[q].z; bias_sum += bq[q].w; }
        for (int x4 = BQ; x4 < W4; ++x4) {
            const float4 v = brow[x4];
            bias_sum += v.x; bias_sum += v.y; bias_sum += v.z; bias_sum += v.w;
        }
        a.gslab[slab_off + CC + bias_c] = slab_b_old + bias_sum;
    }
}

template <bool LDSW, int NCB>
__global__ __launch_bounds__(MIXT) void fno_mix_bwd_skipgrad_kernel(MixSkipDev f) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int block = __builtin_amdgcn_readfirstlane(blockIdx.x);
    if (block < f.s.nmodes) mix_bwd_body<LDSW, true>(f.m, block, f.s.nmodes);
    else skipgrad_rows<NCB>(f.s, smem, block - f.s.nmodes);
}

// ---- wide layers (and 3-D plans): the per-mode stage as TWO launches, so that the weight stream can be split over the chip.
// The fused kernel above has one workgroup per mode: at 217 channels each streams a 377 KB weight slice alone (84 workgroups on
// 256 CUs, 0.9 TB/s), and splitting it would make every part re-read the mode's x1 slice for the H-axis step.
//   hstep : xhat[b][j][kx][c] = sum_h twH[j][h] x1[b][h][kx][c] on the matrix cores -- per kept column kx it is the complex GEMM
//           [m1 x H] . [H x C] with the row-frequency twiddles as the A operand (rows (j, re) = [tr, -ti], (j, im) = [ti, tr],
//           K = (h, re|im) interleaved), x1 read ONCE; one wave = (sample, column, 16 channels, pair of 16-row tiles)
//   cmix  : the complex channel contraction of mix_contract, grid = modes x column-tile groups; backward: gx and the weight
//           gradient for the group's rows of the weight slice (contiguous rows: read once, updated in place)
struct HstepDev {
    const float2* x1; const float2* twH; float2* out;
    int B, C, H, m1, m2c, ntc, nmp;       // ntc = channel tiles, nmp = pairs of 16-row (j, re|im) tiles
};

__global__ __launch_bounds__(256) void fno_hstep_kernel(HstepDev a) {
    const int lane = lane_id(), r = lane & 15, g = lane >> 4;
    long long item = (long long)blockIdx.x * 4 + wave_id();
    const long long nitems = (long long)a.B * a.m2c * a.ntc * a.nmp;
    if (item >= nitems) return;
    const int mp = (int)(item % a.nmp); item /= a.nmp;
    const int ct = (int)(item % a.ntc); item /= a.ntc;
    const int kx = (int)(item % a.m2c), b = (int)(item / a.m2c);
    const int c = 16 * ct + r, cc = c < a.C ? c : a.C - 1;
    const float2* xb = a.x1 + (((long long)b * a.H) * a.m2c + kx) * a.C + cc;
    const long long hstride = (long long)a.m2c * a.C;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const int nkc = (2 * a.H + 15) / 16;
    for (int kc0 = 0; kc0 < nkc; kc0 += 4) {
        f32x4 bf[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {          // B fragment: x1 rows h0, h0 + 1 (clamped loads, masked afterwards)
            const int h0 = 8 * (kc0 + q) + 2 * g;
            const float2 v0 = xb[(long long)min(h0, a.H - 1) * hstride], v1 = xb[(long long)min(h0 + 1, a.H - 1) * hstride];
            const bool ok0 = h0 < a.H && c < a.C, ok1 = h0 + 1 < a.H && c < a.C;
            bf[q] = f32x4{ok0 ? v0.x : 0.f, ok0 ? v0.y : 0.f, ok1 ? v1.x : 0.f, ok1 ? v1.y : 0.f};
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int h0 = 8 * (kc0 + q) + 2 * g;
#pragma unroll
            for (int t = 0; t < 2; ++t) {      // A fragment of row m = (j, part): twiddles of rows h0, h0 + 1
                const int m = 16 * (2 * mp + t) + r, j = m >> 1, part = m & 1;
                f32x4 af = {0.f, 0.f, 0.f, 0.f};
                if (j < a.m1 && h0 < a.H) {
                    const float2 t0 = a.twH[(long long)j * a.H + h0];
                    const float2 t1 = h0 + 1 < a.H ? a.twH[(long long)j * a.H + h0 + 1] : make_float2(0.f, 0.f);
                    af = part ? f32x4{t0.y, t0.x, t1.y, t1.x} : f32x4{t0.x, -t0.y, t1.x, -t1.y};
                }
                acc[t] = mfma16_chunk(af, bf[q], acc[t]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {              // rows 4g .. 4g+3 = frequencies j0, j0 + 1, (re, im) each
        const int j0 = 8 * (2 * mp + t) + 2 * g;
        if (c < a.C) {
            if (j0 < a.m1) a.out[(((long long)b * a.m1 + j0) * a.m2c + kx) * a.C + c] = make_float2(acc[t][0], acc[t][1]);
            if (j0 + 1 < a.m1) a.out[(((long long)b * a.m1 + j0 + 1) * a.m2c + kx) * a.C + c] = make_float2(acc[t][2], acc[t][3]);
        }
    }
}

struct CmixDev {
    const float2* xhat; const float2* ghat; const float2* wspec; float2* y; float2* g_wspec;
    int B, C, m1, m2c, tiles_per_wg;
    FastDiv dC;
};

// forward: y[b][mode][o] = sum_i xhat[b][mode][i] w[mode][i][o] for the workgroup's column tiles
__global__ __launch_bounds__(MIXT) void fno_cmix_fwd_kernel(CmixDev a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* xh = reinterpret_cast<float2*>(smem);      // [B][C]
    const int C = a.C, mode = blockIdx.x;
    const long long mofs = (long long)mode * C, bstr = (long long)a.m1 * a.m2c * C;
    for (int bc = threadIdx.x; bc < a.B * C; bc += MIXT) {
        const int b = fastdiv(bc, a.dC), c = bc - b * C;
        xh[bc] = a.xhat[b * bstr + mofs + c];
    }
    __syncthreads();
    const int nt0 = blockIdx.y * a.tiles_per_wg;
    mix_contract<0, 0>(xh, a.wspec + mofs * C, C, a.y + mofs, bstr, a.B, C, nt0, nt0 + a.tiles_per_wg);
}

// backward: gx[b][mode][i] = sum_o ghat[b][o] conj(w[i][o]) and gw[i][o] += sum_b conj(xhat[b][i]) ghat[b][o] for the workgroup's rows i
__global__ __launch_bounds__(MIXT) void fno_cmix_bwd_kernel(CmixDev a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* gh = reinterpret_cast<float2*>(smem);      // [B][C]
    float2* xsv = gh + a.B * a.C;                      // [B][C]
    const int C = a.C, mode = blockIdx.x;
    const long long mofs = (long long)mode * C, bstr = (long long)a.m1 * a.m2c * C;
    for (int bc = threadIdx.x; bc < a.B * C; bc += MIXT) {
        const int b = fastdiv(bc, a.dC), c = bc - b * C;
        gh[bc] = a.ghat[b * bstr + mofs + c];
        xsv[bc] = a.xhat[b * bstr + mofs + c];
    }
    __syncthreads();
    const int nt = (C + 15) / 16, it0 = blockIdx.y * a.tiles_per_wg, it1 = min(nt, it0 + a.tiles_per_wg);
    const float2* wm = a.wspec + mofs * C;
    float2* gw = a.g_wspec + mofs * C;
    mix_contract<1, 1>(gh, wm, C, a.y + mofs, bstr, a.B, C, it0, it1);
    {
        const int lane = lane_id(), w = wave_id(), r = lane & 15, g = lane >> 4;
        constexpr int NW = MIXT / 64;
        const int ri = g & 1;
        for (int t = NW - 1 - w; t < (it1 - it0) * nt; t += NW) {
            const int it = it0 + t / nt, ot = t % nt;
            const int i = 16 * it + r, o = 16 * ot + r;
            float2 old[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) old[q] = gw[(long long)min(16 * it + 4 * g + q, C - 1) * C + min(o, C - 1)];
            f32x4 are = {0.f, 0.f, 0.f, 0.f}, aim = {0.f, 0.f, 0.f, 0.f};
            for (int b0 = 0; b0 < a.B; b0 += 2) {
                const int b = b0 + (g >> 1);
                const bool okb = b < a.B;
                const float2 xv = (okb && i < C) ? xsv[b * C + i] : make_float2(0.f, 0.f);
                const float2 gv = (okb && o < C) ? gh[b * C + o] : make_float2(0.f, 0.f);
                const float av = ri ? xv.y : xv.x;
                are = mfma16(av, ri ? gv.y : gv.x, are);
                aim = mfma16(av, ri ? -gv.x : gv.y, aim);
            }
            if (o < C) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int io = 16 * it + 4 * g + q;
                    if (io < C) gw[(long long)io * C + o] = make_float2(old[q].x + are[q], old[q].y + aim[q]);
                }
            }
        }
    }
}

template <typename K>
int set_lds(K kernel, size_t bytes, const char* what) {
    return dlwp_ensure_lds(reinterpret_cast<const void*>(kernel), bytes, what);
}

template <typename T>
int upload(T** dst, const std::vector<T>& host) {
    DLWP_HIP(hipMalloc(reinterpret_cast<void**>(dst), host.size() * sizeof(T)));
    DLWP_HIP(hipMemcpy(*dst, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return DLWP_OK;
}

}  // namespace

// kept signed frequencies of an fftshift-ed axis of length n (neuralop SpectralConv slicing, App. A-1)
static std::vector<int> kept_freqs(int n, int m) {
    const int start = n - m, lo = start / 2;
    std::vector<int> k(m);
    for (int j = 0; j < m; ++j) k[j] = lo + j - n / 2;
    return k;
}

// T == 1: the 2-D plan.  T > 1: the (T*H) x W image of a [T][H][W] volume with m0*m1 separable (time, row) frequencies.
static int plan_create_impl(int C, int T, int H, int W, int m0, int m1, int m2c, dlwp_fno_plan** out) {
    DLWP_REQUIRE(out, DLWP_E_INVALID, "fno_plan_create: out is NULL");
    DLWP_REQUIRE(C > 0 && T > 0 && H > 0 && W > 0 && m0 > 0 && m1 > 0 && m2c > 0, DLWP_E_INVALID, "fno_plan_create: bad dims");
    DLWP_REQUIRE(W % 16 == 0, DLWP_E_UNSUPPORTED, "fno_plan_create: W must be a multiple of 16 (got %d)", W);
    DLWP_REQUIRE(H % 2 == 0, DLWP_E_UNSUPPORTED, "fno_plan_create: H must be even (got %d)", H);
    DLWP_REQUIRE(T == 1 || T % 2 == 0, DLWP_E_UNSUPPORTED, "fno_plan_create3d: the time axis must be even (got %d)", T);
    DLWP_REQUIRE(m1 <= H && m0 <= T && m2c <= W / 2 + 1, DLWP_E_INVALID, "fno_plan_create: more modes than the grid has");
    DLWP_REQUIRE(C <= 1024, DLWP_E_UNSUPPORTED, "fno_plan_create: hidden_channels <= 1024 supported (got %d)", C);
    DLWP_REQUIRE(2 * m2c <= 32, DLWP_E_UNSUPPORTED, "fno_plan_create: n_modes[-1]/2+1 <= 16 supported (got %d)", m2c);
    dlwp_fno_plan* p = new dlwp_fno_plan();
    const int HH = T * H, MM = m0 * m1;
    p->C = C; p->H = HH; p->W = W; p->m1 = MM; p->m2c = m2c;
    p->C_pad = round_up(C, 16);
    p->NP = round_up(2 * m2c, 16);
    p->force_wide = T > 1;
    const double PI = 3.14159265358979323846;
    const std::vector<int> kt = kept_freqs(T, m0), kh = kept_freqs(H, m1);
    std::vector<float2> tw((size_t)MM * HH);
    for (int a = 0; a < m0; ++a)
        for (int j = 0; j < m1; ++j)
            for (int t = 0; t < T; ++t)
                for (int h = 0; h < H; ++h) {
                    const long long at = (((long long)kt[a] * t) % T + T) % T, ah = (((long long)kh[j] * h) % H + H) % H;
                    const double ang = -2.0 * PI * ((double)at / T + (double)ah / H);
                    tw[((size_t)a * m1 + j) * HH + (size_t)t * H + h] = make_float2((float)cos(ang), (float)sin(ang));
                }
    std::vector<float> ft_fwd((size_t)p->NP * W, 0.f), ft_adj(ft_fwd), g_inv(ft_fwd), g_adj(ft_fwd);
    const double inv_hw = 1.0 / ((double)HH * W);
    for (int kx = 0; kx < m2c; ++kx) {
        const double ck = (kx == 0 || (W % 2 == 0 && kx == W / 2)) ? 1.0 : 2.0;
        for (int w = 0; w < W; ++w) {
            const long long kw = ((long long)kx * w) % W;
            const double ang = 2.0 * PI * (double)kw / W;
            const double c = cos(ang), s = sin(ang);
            ft_fwd[(size_t)(2 * kx) * W + w] = (float)(c * inv_hw);
            ft_fwd[(size_t)(2 * kx + 1) * W + w] = (float)(-s * inv_hw);
            ft_adj[(size_t)(2 * kx) * W + w] = (float)(c * ck);
            ft_adj[(size_t)(2 * kx + 1) * W + w] = (float)(-s * ck);
            g_inv[(size_t)(2 * kx) * W + w] = (float)(c * ck);
            g_inv[(size_t)(2 * kx + 1) * W + w] = (float)(-s * ck);
            g_adj[(size_t)(2 * kx) * W + w] = (float)(c * inv_hw);
            g_adj[(size_t)(2 * kx + 1) * W + w] = (float)(-s * inv_hw);
        }
    }
    int rc;
    if ((rc = upload(&p->twH, tw)) || (rc = upload(&p->FT_fwd, ft_fwd)) || (rc = upload(&p->FT_adj, ft_adj)) ||
        (rc = upload(&p->G_inv, g_inv)) || (rc = upload(&p->G_adj, g_adj))) {
        delete p;
        return rc;
    }
    *out = p;
    return DLWP_OK;
}

extern "C" int dlwp_fno_plan_create(int C, int H, int W, int m1, int m2c, dlwp_fno_plan** out) {
    return plan_create_impl(C, 1, H, W, 1, m1, m2c, out);
}

extern "C" int dlwp_fno_plan_create3d(int C, int T, int H, int W, int m0, int m1, int m2c, dlwp_fno_plan** out) {
    DLWP_REQUIRE(T > 1, DLWP_E_INVALID, "fno_plan_create3d: T must be > 1 (use dlwp_fno_plan_create for images)");
    return plan_create_impl(C, T, H, W, m0, m1, m2c, out);
}

extern "C" void dlwp_fno_plan_destroy(dlwp_fno_plan* p) {
    if (!p) return;
    (void)hipFree(p->twH); (void)hipFree(p->FT_fwd); (void)hipFree(p->FT_adj);
    (void)hipFree(p->G_inv); (void)hipFree(p->G_adj);
    delete p;
}

static size_t x1_elems(const dlwp_fno_plan* p, int B) { return (size_t)B * p->H * p->m2c * p->C; }
static size_t spec_elems(const dlwp_fno_plan* p, int B) { return (size_t)B * p->m1 * p->m2c * p->C; }
static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
static size_t ws_x1_bytes(const dlwp_fno_plan* p, int B) { return align256(x1_elems(p, B) * sizeof(float2)); }

extern "C" size_t dlwp_fno_block_workspace_bytes(const dlwp_fno_plan* p, int B) {
    return ws_x1_bytes(p, B) + align256(spec_elems(p, B) * sizeof(float2));
}
// the two halves of a block workspace: the rows DFT (x1 / g1) and the per-mode stage's result (y / gxhat)
struct BlockWs { float2 *x1, *spec; };
static BlockWs carve_ws(const dlwp_fno_plan* p, int B, void* workspace) {
    return BlockWs{static_cast<float2*>(workspace), reinterpret_cast<float2*>(static_cast<char*>(workspace) + ws_x1_bytes(p, B))};
}

constexpr size_t CU_LDS_BYTES = (size_t)160 * 1024;      // LDS of one gfx950 CU: the most a workgroup can ask for

#define DISPATCH_NCB_NBN(NCBV, NBNV, MACRO)                      \
    switch ((NCBV) * 10 + (NBNV)) {                              \
        case 11: MACRO(1, 1) break; case 12: MACRO(1, 2) break;  \
        case 21: MACRO(2, 1) break; case 22: MACRO(2, 2) break;  \
        case 31: MACRO(3, 1) break; case 32: MACRO(3, 2) break;  \
        case 41: MACRO(4, 1) break; case 42: MACRO(4, 2) break;  \
        default:                                                 \
            dlwp_set_error("fno: unsupported tile shape");       \
            return DLWP_E_UNSUPPORTED;                           \
    }

int dlwp_fno_rows_dft(const dlwp_fno_plan* p, const float* x, int act_in, int adjoint, float2* x1, int B,
                      hipStream_t stream) {
    if (dlwp_fno_is_wide(p)) return dlwp_fno_rows_dft_wide(p, x, act_in, adjoint, x1, B, stream);
    RowsDev a{x, x1, adjoint ? p->FT_adj : p->FT_fwd, act_in, p->C, p->H, p->W, p->m2c, p->C_pad, p->NP};
    const int LDP = p->W + 4;
    const size_t lds = sizeof(float) * ((size_t)p->C_pad * LDP + (size_t)p->NP * LDP + (size_t)4 * p->C_pad * p->NP);
    const dim3 grid(B * p->H), block(256);
    int rc;
#define LAUNCH(N, M)                                                                   \
    if ((rc = set_lds(fno_rows_kernel<N, M>, lds, "fno_rows")) != DLWP_OK) return rc; \
    hipLaunchKernelGGL((fno_rows_kernel<N, M>), grid, block, lds, stream, a);
    DISPATCH_NCB_NBN(p->C_pad / 16, p->NP / 16, LAUNCH)
#undef LAUNCH
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

// the argument block of a per-mode launch (forward: xhat_in == g_wspec == NULL; backward: xhat == NULL)
static MixDev make_mix_dev(const dlwp_fno_plan* p, const float2* x1, const float2* wspec, const float2* xhat_in, float2* xhat,
                           float2* y, float2* g_wspec, int B) {
    return MixDev{x1, wspec, xhat_in, xhat, y, g_wspec, p->twH, B, p->C, p->H, p->m1, p->m2c,
                  make_fastdiv(p->C), make_fastdiv(B * p->C), make_fastdiv(B * p->C / 2 > 0 ? B * p->C / 2 : 1)};
}

static size_t mix_lds_bytes(const MixDev& a, bool bwd, bool ldsw) {
    const int BC = a.B * a.C;
    int ns = MIXT / BC;
    if (ns < 1) ns = 1;
    const int lim = a.H < a.C ? a.H : a.C;
    if (ns > lim) ns = lim;
    const int ns2 = mix_slots2(a.B, a.C, a.H);
    if (ns2 > ns) ns = ns2;
    return sizeof(float2) * ((size_t)BC * ((bwd ? 2 : 1) + ns) + a.H + (ldsw ? (size_t)a.C * (a.C + 1) : 0));
}

static int mix_launch(const dlwp_fno_plan* p, bool bwd, MixDev& a, hipStream_t stream) {
    const bool ldsw = a.C <= 64;                    // the [C][C+1] complex weight image fits beside the H-step partials
    const size_t lds = mix_lds_bytes(a, bwd, ldsw);
    const dim3 grid(p->m1 * p->m2c), block(MIXT);
    int rc;
#define MIX_LAUNCH(KERNEL, NAME)                                                    \
    do {                                                                            \
        if ((rc = set_lds(KERNEL, lds, NAME)) != DLWP_OK) return rc;                \
        hipLaunchKernelGGL(KERNEL, grid, block, lds, stream, a);                    \
    } while (0)
    if (bwd) {
        if (ldsw) MIX_LAUNCH(fno_mix_bwd_kernel<true>, "fno_mix_bwd"); else MIX_LAUNCH(fno_mix_bwd_kernel<false>, "fno_mix_bwd");
    } else {
        if (ldsw) MIX_LAUNCH(fno_mix_fwd_kernel<true>, "fno_mix_fwd"); else MIX_LAUNCH(fno_mix_fwd_kernel<false>, "fno_mix_fwd");
    }
#undef MIX_LAUNCH
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

static int hstep_launch(const dlwp_fno_plan* p, const float2* x1, float2* out, int B, hipStream_t stream) {
    HstepDev a{x1, p->twH, out, B, p->C, p->H, p->m1, p->m2c, ceil_div(p->C, 16), ceil_div(ceil_div(2 * p->m1, 16), 2)};
    const long long items = (long long)B * p->m2c * a.ntc * a.nmp;
    hipLaunchKernelGGL(fno_hstep_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, stream, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

// column-tile groups per mode: enough workgroups to cover the chip about twice (every group streams its own part of the slice)
static int cmix_tiles_per_wg(const dlwp_fno_plan* p) {
    const int nt = ceil_div(p->C, 16), modes = p->m1 * p->m2c;
    int groups = ceil_div(512, modes);
    if (groups > nt) groups = nt;
    if (groups < 1) groups = 1;
    return ceil_div(nt, groups);
}

int dlwp_fno_mix_fwd(const dlwp_fno_plan* p, const float2* x1, const float2* wspec, float2* xhat, float2* y,
                     int B, hipStream_t stream) {
    if (dlwp_fno_is_wide(p)) {
        int rc = hstep_launch(p, x1, xhat, B, stream);
        if (rc) return rc;
        CmixDev a{xhat, nullptr, wspec, y, nullptr, B, p->C, p->m1, p->m2c, cmix_tiles_per_wg(p), make_fastdiv(p->C)};
        const size_t lds = sizeof(float2) * (size_t)B * p->C;
        if ((rc = set_lds(fno_cmix_fwd_kernel, lds, "fno_cmix_fwd")) != DLWP_OK) return rc;
        hipLaunchKernelGGL(fno_cmix_fwd_kernel, dim3(p->m1 * p->m2c, ceil_div(ceil_div(p->C, 16), a.tiles_per_wg)), dim3(MIXT), lds,
                           stream, a);
        DLWP_LAUNCH_CHECK();
        return DLWP_OK;
    }
    MixDev a = make_mix_dev(p, x1, wspec, nullptr, xhat, y, nullptr, B);
    return mix_launch(p, false, a, stream);
}

// (wide layers: the H-step result ghat [B][m1][m2c][C] is produced in gxhat and moved into the storage of g1 -- dead once the
// H-step has read it, and at least as large since m1 <= H -- because the contraction reads ghat of ALL channels while it
// writes gx into gxhat; the caller's g1 buffer is therefore overwritten)
int dlwp_fno_mix_bwd(const dlwp_fno_plan* p, const float2* g1, const float2* wspec, const float2* xhat,
                     float2* gxhat, float2* g_wspec, int B, hipStream_t stream) {
    if (dlwp_fno_is_wide(p)) {
        DLWP_REQUIRE(p->m1 <= p->H, DLWP_E_INVALID, "fno_mix_bwd: more row frequencies than rows");
        int rc = hstep_launch(p, g1, gxhat, B, stream);
        if (rc) return rc;
        const size_t n = (size_t)B * p->m1 * p->m2c * p->C;
        float2* ghat = const_cast<float2*>(g1);
        DLWP_HIP(hipMemcpyAsync(ghat, gxhat, n * sizeof(float2), hipMemcpyDeviceToDevice, stream));
        CmixDev a{xhat, ghat, wspec, gxhat, g_wspec, B, p->C, p->m1, p->m2c, cmix_tiles_per_wg(p), make_fastdiv(p->C)};
        const size_t lds = sizeof(float2) * (size_t)2 * B * p->C;
        if ((rc = set_lds(fno_cmix_bwd_kernel, lds, "fno_cmix_bwd")) != DLWP_OK) return rc;
        hipLaunchKernelGGL(fno_cmix_bwd_kernel, dim3(p->m1 * p->m2c, ceil_div(ceil_div(p->C, 16), a.tiles_per_wg)), dim3(MIXT), lds,
                           stream, a);
        DLWP_LAUNCH_CHECK();
        return DLWP_OK;
    }
    MixDev a = make_mix_dev(p, g1, wspec, xhat, nullptr, gxhat, g_wspec, B);
    return mix_launch(p, true, a, stream);
}

// dlwp_fno_mix_bwd whose launch also forms the by-products of the block's backward `spatial` (fno_mix_bwd_skipgrad_kernel): the
// gK partial and bias gradient of every image row from tin (g_pre of the block) and pprev (its stored input, GELU applied when
// act_prev) into gslab, as the two-role `spatial` launch would.  The caller then runs `spatial` with neither gslab nor g_wskip /
// g_bias.  Only where dlwp_fno_bwd_decide() says `hosted`: a narrow plan whose two-role layout fits.
static int mix_bwd_skipgrad_launch(const dlwp_fno_plan* p, const float2* g1, const float2* wspec, const float2* xhat, float2* gxhat,
                                   float2* g_wspec, const float* tin, const float* pprev, int act_prev, float* gslab,
                                   int gslab_accumulate, int B, hipStream_t stream) {
    const int ncb = p->C_pad / 16;
    MixSkipDev f{};
    f.m = make_mix_dev(p, g1, wspec, xhat, nullptr, gxhat, g_wspec, B);
    f.s = SkipGradDev{tin, pprev, gslab, gslab_accumulate, act_prev, p->C, p->H, p->W, p->C_pad, p->m1 * p->m2c, B * p->H,
                      make_fastdiv(p->C)};
    const size_t lds_mix = mix_lds_bytes(f.m, true, true), lds_rows = sizeof(float) * (size_t)2 * 4 * p->C_pad * p->C_pad;
    const size_t lds = lds_mix > lds_rows ? lds_mix : lds_rows;
    const dim3 grid(p->m1 * p->m2c + (B * p->H + 1) / 2), block(MIXT);
    const double pix = (double)B * p->H * p->W;
    dlwp_prof_scope prof(stream, 2.0 * pix * p->C * p->C + 8.0 * B * p->C * p->C * 2.0 * p->m1 * p->m2c,
                         8.0 * pix * p->C + 16.0 * p->m1 * p->m2c * p->C * p->C, "fno_mix_bwd_skipgrad_kernel<true, %d>", ncb);
    int rc;
#define LAUNCH(N)                                                                                                     \
    if ((rc = set_lds(fno_mix_bwd_skipgrad_kernel<true, N>, lds, "fno_mix_bwd_skipgrad")) != DLWP_OK) return rc;      \
    hipLaunchKernelGGL((fno_mix_bwd_skipgrad_kernel<true, N>), grid, block, lds, stream, f);
    switch (ncb) {
        case 1: LAUNCH(1) break;
        case 2: LAUNCH(2) break;
        case 3: LAUNCH(3) break;
        default: LAUNCH(4) break;
    }
#undef LAUNCH
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

// the device argument block of a `spatial` launch, and the LDS bytes of its two layouts (four-wave / two-role)
static SpatialDev make_spatial_dev(const dlwp_fno_plan* p, const dlwp_fno_spatial_args* s) {
    SpatialDev a{};
    a.tin = s->tin; a.spec = s->spec; a.wskip = s->wskip; a.bias = s->bias; a.pprev = s->pprev;
    a.out = s->out; a.x1_out = s->x1_out; a.g_wskip = s->g_wskip; a.g_bias = s->g_bias;
    a.gslab = s->gslab; a.gslab_accumulate = s->gslab_accumulate;
    a.twH = p->twH;
    a.G = s->inverse_adjoint ? p->G_adj : p->G_inv;
    a.FT = s->x1_adjoint ? p->FT_adj : p->FT_fwd;
    a.act_tin = s->act_tin; a.transpose_w = s->transpose_w; a.act_prev = s->act_prev;
    a.x1_act = s->x1_act; a.is_bwd = s->inverse_adjoint;
    a.vec_w = (reinterpret_cast<uintptr_t>(s->wskip) & 15) == 0;
    a.dC = make_fastdiv(p->C);
    a.C = p->C; a.H = p->H; a.W = p->W; a.m1 = p->m1; a.m2c = p->m2c; a.C_pad = p->C_pad; a.NP = p->NP;
    return a;
}
static void spatial_lds_bytes(const dlwp_fno_plan* p, size_t& lds, size_t& lds_roles) {
    const int LDP = p->W + 4;
    const size_t gemm_ops = (size_t)p->NP * LDP + (size_t)p->C_pad * (p->C_pad + 4) + (size_t)p->C_pad * (p->NP + 4);   // gs, ks, s1
    const size_t gks = (size_t)4 * p->C_pad * p->C_pad;
    const size_t live = (size_t)3 * p->C_pad * LDP + (size_t)p->NP * LDP + (size_t)4 * p->C_pad * p->NP;
    lds = sizeof(float) * (live + p->C_pad + (gemm_ops > gks ? gemm_ops : gks));
    // two-role form of the backward kernel: gks next to gs / ks / s1 instead of over them
    lds_roles = sizeof(float) * (live + gemm_ops + gks);
}
// The two-role layout fits the LDS of a CU: on 64-wide rows C_pad 16 / 32 / 48 (65 KiB at C_pad 32), on 32-wide rows C_pad 64 too.
// It does not fit for C_pad 64 on 64-wide rows (161.5 KiB: C 49 .. 64 at the published grid) nor for C_pad 32 on 256-wide rows
// (161 KiB).
static bool two_role_fits(const dlwp_fno_plan* p) {
    size_t lds, lds_roles;
    spatial_lds_bytes(p, lds, lds_roles);
    return lds_roles <= CU_LDS_BYTES;
}

int dlwp_fno_spatial(const dlwp_fno_plan* p, const dlwp_fno_spatial_args* s, hipStream_t stream) {
    if (dlwp_fno_is_wide(p)) {
        // channel-blocked form: the fused by-products (next block's row DFT, skip-weight / bias gradients) are separate launches
        int rc = dlwp_fno_spatial_wide(p, s, stream);
        if (rc) return rc;
        if (s->inverse_adjoint && (s->g_wskip || s->g_bias)) {
            DLWP_REQUIRE(s->g_wskip && s->g_bias && !s->gslab, DLWP_E_INVALID, "fno_spatial (wide): needs g_wskip and g_bias, no slab");
            if ((rc = dlwp_fno_skip_wgrad(p, s->tin, s->pprev, s->act_prev, s->g_wskip, s->g_bias, s->B, stream))) return rc;
        }
        if (s->x1_out) return dlwp_fno_rows_dft_wide(p, s->out, s->x1_act, s->x1_adjoint, s->x1_out, s->B, stream);
        return DLWP_OK;
    }
    const SpatialDev a = make_spatial_dev(p, s);
    size_t lds, lds_roles;
    spatial_lds_bytes(p, lds, lds_roles);
    const dim3 grid(s->B * p->H);
    int rc;
    const int mode = !a.is_bwd ? 0 : (a.act_prev ? 1 : 2);
    // The by-products get waves of their own when the backward launch has a skip-weight gradient to form and the larger
    // footprint fits: other shapes keep the four-wave kernel, as does a backward launch without g_wskip / slab.
    const bool roles = a.is_bwd && (a.g_wskip || a.gslab) && two_role_fits(p);
    const double pix = (double)s->B * p->H * p->W;
    dlwp_prof_scope prof(stream, 2.0 * pix * p->C * (p->C * (roles ? 2 : 1) + 2 * p->m2c), 4.0 * pix * p->C * (a.is_bwd ? 3 : 2),
                         roles ? "fno_spatial_roles_kernel<%d, %d, %d>" : "fno_spatial_kernel<%d, %d, %d>", p->C_pad / 16,
                         p->NP / 16, mode);              // the instantiation this call launches, as the live accounting reports it
#define LAUNCH_KERNEL(K, NT, BYTES)                                              \
    if ((rc = set_lds(K, BYTES, "fno_spatial")) != DLWP_OK) return rc;           \
    hipLaunchKernelGGL(K, grid, dim3(NT), BYTES, stream, a);
#define LAUNCH(N, M)                                                                       \
    if (mode == 0) { LAUNCH_KERNEL((fno_spatial_kernel<N, M, 0>), 256, lds) }              \
    else if (mode == 1) {                                                                  \
        if (roles) { LAUNCH_KERNEL((fno_spatial_roles_kernel<N, M, 1>), 512, lds_roles) }  \
        else { LAUNCH_KERNEL((fno_spatial_kernel<N, M, 1>), 256, lds) }                    \
    } else {                                                                               \
        if (roles) { LAUNCH_KERNEL((fno_spatial_roles_kernel<N, M, 2>), 512, lds_roles) }  \
        else { LAUNCH_KERNEL((fno_spatial_kernel<N, M, 2>), 256, lds) }                    \
    }
    DISPATCH_NCB_NBN(p->C_pad / 16, p->NP / 16, LAUNCH)
#undef LAUNCH
#undef LAUNCH_KERNEL
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" long long dlwp_fno_block_slab_floats(const dlwp_fno_plan* p, int B) {
    return p && B > 0 ? (long long)B * p->H * dlwp_fno_gslab_stride(p->C) : 0;
}

// ---- block 0's backward `spatial` + the lifting MLP's backward in one launch (fno_spatial_lift_bwd_kernel).
// LDS bytes of that launch, or 0 where the shapes take the two launches: 64-wide rows (a `spatial` row is a pwmlp pixel tile),
// a narrow 2-D plan whose two-role layout fits (C_pad <= 48), and the lifting phase's tiles -- behind tout_s, over the regions
// the `spatial` phase no longer needs -- inside the LDS of a CU.  Instantiated are the (C_pad / 16, Cin_pad / 16) pairs that
// compile without scratch and without vector spills: (1, 1), (2, 1), (2, 2), (3, 1), (3, 2); like pwmlp_bwd_kernel's own, the
// wider ones spill, and they keep the two launches.
static size_t lift_bwd_fused_lds(const dlwp_fno_plan* p, int Cin) {
    if (dlwp_fno_is_wide(p) || p->W != PT || Cin < 1 || Cin > 32 || (p->C_pad == 16 && Cin > 16)) return 0;
    size_t lds, lds_roles;
    spatial_lds_bytes(p, lds, lds_roles);
    const size_t phase2 = sizeof(float) * ((size_t)2 * p->C_pad * LDP + (size_t)(1 + BWD_WAVES) * round_up(Cin, 16) * LDP);
    const size_t need = lds_roles > phase2 ? lds_roles : phase2;
    return need <= CU_LDS_BYTES ? need : 0;       // need >= lds_roles: the two-role layout fits too
}

// The same launch with the previous net call's projection backward as its third phase (fno_spatial_lift_proj_bwd_kernel): LDS
// bytes, or 0 where that projection backward keeps its own launch.  Taken where the stand-alone launch would be the scalar-output
// kernel with the rows DFT in its epilogue (dlwp_pwmlp_bwd_rows_ex's own conditions: 64-wide rows, NP == 16, 16-byte access to
// every view, a dense gx), at most two channel tiles (the instantiations that compile without scratch and without vector
// spills), and all three phases inside the LDS of a CU.
static size_t proj_bwd_fused_lds(const dlwp_fno_plan* p, int Cin, const dlwp_fno_proj_bwd_tail* q) {
    const size_t lift = lift_bwd_fused_lds(p, Cin);
    const int P = p->H * p->W;
    if (!lift || !q || q->Cout != 1 || q->Ch < 1 || p->C_pad > 32 || !dlwp_pwmlp_rows_fusable(p, p->C, P)) return 0;
    if (!q->x || !q->gy || !q->pred || !q->target || !q->gx || !q->gx->base || !q->x1_out || !q->slab) return 0;
    if (!view_vec_ok(*q->x) || !view_vec_ok(*q->gy) || !view_vec_ok(*q->gx) || q->gx->bstride != (long long)p->C * P ||
        q->gx->cstride != P) return 0;
    const size_t phase3 = sizeof(float) * ((size_t)(1 + BWD_WAVES) * p->C_pad + 16) * LDP;
    const size_t need = lift > phase3 ? lift : phase3;
    return need <= CU_LDS_BYTES ? need : 0;
}

// `s`: the backward `spatial` arguments of block 0 (no activation in front of it, neither `out` nor a fused row DFT); t: the lifting
// backward's operands, as for dlwp_pwmlp_bwd_ex with gy = the gradient `spatial` would have written.  Only where
// dlwp_fno_bwd_decide() names the fused form.  s->gslab == NULL: the by-products of block 0 were formed by the per-mode launch
// (mix_bwd_skipgrad_launch), and phase 1 runs the chain alone.  q != NULL (only where dlwp_fno_bwd_decide() says `proj`): the
// previous net call's projection backward as the third phase, its argument block filled as dlwp_pwmlp_bwd_rows_ex fills it.
static int spatial_lift_bwd_launch(const dlwp_fno_plan* p, const dlwp_fno_spatial_args* s, const dlwp_fno_lift_bwd_tail* t,
                                   const dlwp_fno_proj_bwd_tail* q, hipStream_t stream) {
    const int Cin = t->Cin, Ch = t->Ch;
    const size_t lds = q ? proj_bwd_fused_lds(p, Cin, q) : lift_bwd_fused_lds(p, Cin);
    const bool role_b = s->gslab != nullptr;
    SpatialLiftProjDev fq{};
    SpatialLiftDev f{};
    f.s = make_spatial_dev(p, s);
    BwdArgs& a = f.m;
    a.x = *t->x; a.w1 = t->w1; a.b1 = t->b1; a.w2 = t->w2;
    if (t->gx) a.gx = *t->gx;
    a.gx_accumulate = t->gx_accumulate;
    a.B = s->B; a.Cin = Cin; a.Ch = Ch; a.Cout = p->C; a.P = p->H * p->W;
    a.tiles_per_sample = p->H;
    a.Cin_pad = round_up(Cin, 16); a.Ch_pad = round_up(Ch, 16); a.Cout_pad = p->C_pad;
    a.slab = t->slab; a.slab_stride = dlwp_pwmlp_slab_stride(Cin, Ch, p->C); a.slab_accumulate = t->slab_accumulate;
    a.vec_w = aligned16(t->w1);
    a.dCin = make_fastdiv(Cin); a.dCh = make_fastdiv(Ch);
    a.vec_x = view_vec_ok(a.x);
    const int ncb = p->C_pad / 16, nbn = p->NP / 16, nib = a.Cin_pad / 16;
    const dim3 grid(s->B * p->H);
    const double pix = (double)s->B * a.P;
    double flops = 2.0 * pix * (p->C * (2.0 * p->C + 2 * p->m2c) + Ch * (3.0 * Cin + 2.0 * p->C));
    double bytes = 4.0 * pix * (2.0 * p->C + 2.0 * Cin);
    if (q) {
        fq.s = f.s; fq.m = f.m;
        BwdArgs& c = fq.q;
        c.x = *q->x; c.w1 = q->w1; c.b1 = q->b1; c.w2 = q->w2;
        c.gy = *q->gy; c.pred = *q->pred; c.target = *q->target; c.mse_scale = q->mse_scale;
        c.gx = *q->gx; c.gx_accumulate = 0;
        c.B = s->B; c.Cin = p->C; c.Ch = q->Ch; c.Cout = q->Cout; c.P = a.P;
        c.tiles_per_sample = p->H;
        c.Cin_pad = p->C_pad; c.Ch_pad = round_up(q->Ch, 16); c.Cout_pad = round_up(q->Cout, 16);
        c.slab = q->slab; c.slab_stride = dlwp_pwmlp_slab_stride(p->C, q->Ch, q->Cout); c.slab_accumulate = q->slab_accumulate;
        c.vec_w = aligned16(q->w1);
        c.dCin = make_fastdiv(p->C); c.dCh = make_fastdiv(q->Ch);
        c.vec_x = 1;                      // proj_bwd_fused_lds() has checked the views
        c.x1_out = q->x1_out; c.FT = p->FT_adj; c.rows_H = p->H; c.m2c = p->m2c;
        flops += 2.0 * pix * q->Ch * (3.0 * p->C + 2.0 * q->Cout);
        bytes += 4.0 * pix * (2.0 * p->C + q->Cout);
    }
    // one accounting row for both forms of phase 1, with or without the third phase
    dlwp_prof_scope prof(stream, flops, bytes, "fno_spatial_lift_bwd_kernel<%d, %d, %d>", ncb, nbn, nib);
    int rc;
#define LAUNCH(N, M, I)                                                                                                 \
    if (role_b) {                                                                                                       \
        if ((rc = set_lds(fno_spatial_lift_bwd_kernel<N, M, I>, lds, "fno_spatial_lift_bwd")) != DLWP_OK) return rc;    \
        hipLaunchKernelGGL((fno_spatial_lift_bwd_kernel<N, M, I>), grid, dim3(512), lds, stream, f);                    \
    } else {                                                                                                            \
        if ((rc = set_lds(fno_spatial_lift_bwd_kernel<N, M, I, false>, lds, "fno_spatial_lift_bwd")) != DLWP_OK) return rc; \
        hipLaunchKernelGGL((fno_spatial_lift_bwd_kernel<N, M, I, false>), grid, dim3(512), lds, stream, f);             \
    }
#define LAUNCH3(N, I)                                                                                                    \
    if (role_b) {                                                                                                        \
        if ((rc = set_lds(fno_spatial_lift_proj_bwd_kernel<N, 1, I>, lds, "fno_spatial_lift_proj_bwd")) != DLWP_OK) return rc; \
        hipLaunchKernelGGL((fno_spatial_lift_proj_bwd_kernel<N, 1, I>), grid, dim3(512), lds, stream, fq);                \
    } else {                                                                                                             \
        if ((rc = set_lds(fno_spatial_lift_proj_bwd_kernel<N, 1, I, false>, lds, "fno_spatial_lift_proj_bwd")) != DLWP_OK) return rc; \
        hipLaunchKernelGGL((fno_spatial_lift_proj_bwd_kernel<N, 1, I, false>), grid, dim3(512), lds, stream, fq);         \
    }
#define ROW(N, M)                                      \
    if (nib == 1) { LAUNCH(N, M, 1) } else { LAUNCH(N, M, 2) }
    if (q) switch (ncb * 10 + nib) {    // proj_bwd_fused_lds() has refused everything else (NP == 16: nbn == 1)
        case 11: LAUNCH3(1, 1) break;
        case 21: LAUNCH3(2, 1) break; case 22: LAUNCH3(2, 2) break;
        default: return DLWP_E_UNSUPPORTED;
    }
    else switch (ncb * 10 + nbn) {      // lift_bwd_fused_lds() has refused everything else
        case 11: LAUNCH(1, 1, 1) break; case 12: LAUNCH(1, 2, 1) break;
        case 21: ROW(2, 1) break; case 22: ROW(2, 2) break;
        case 31: ROW(3, 1) break; case 32: ROW(3, 2) break;
        default: return DLWP_E_UNSUPPORTED;
    }
#undef ROW
#undef LAUNCH3
#undef LAUNCH
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

// ---- the last block's forward `spatial` + the projection MLP (+ the next net call's lifting MLP) in one launch
// (fno_spatial_proj_fwd_kernel).  Dispatched are the instantiations that compile for gfx950 without scratch and without vector
// spills: C_pad 16 / 32 / 48 projection only, C_pad 16 / 32 with the chained lifting MLP (whose fused rows DFT needs NP == 16).
struct ProjFwdLaunch {
    SpatialProjDev f;
    size_t lds;
    int nob2;
    double flops, bytes;
};
// fills the launch where dlwp_fno_fwd_decide() names the fused form.  What only shows while the projection chain's arguments are
// built is refused here, still in front of every launch: DLWP_E_UNSUPPORTED from chain_make_args (vector access to the views, the
// chained lifting's own limits) or for more LDS than a CU has.
static int proj_fwd_prepare(ProjFwdLaunch& q, const dlwp_fno_plan* p, const dlwp_fno_spatial_args* s, const dlwp_fno_proj_fwd_tail* t) {
    const bool second = t->x2v != nullptr;
    const int Ch1 = t->Ch1, Cout1 = t->Cout1, Cin2 = t->Cin2, Ch2 = t->Ch2;
    const int HW = p->H * p->W;
    const dlwp_chan_src ps{s->out, (long long)p->C * HW, HW, nullptr, nullptr};     // what the projection would read back
    size_t lds_floats;
    const int rc = chain_make_args(q.f.c, lds_floats, &ps, t->pw1, t->pb1, t->pw2, t->pb2, t->y1, t->res1, p->C, Ch1, Cout1, second,
                                   t->x2v, t->lw1, t->lb1, t->lw2, t->lb2, t->y2, Cin2, Ch2, p->C, t->next_ch, s->B, HW, p, t->x1_next);
    if (rc) return rc;
    if (second && !q.f.c.l.x1_out) return DLWP_E_UNSUPPORTED;
    // the operands of the `spatial` GEMM behind the MLP images: tin_s, gs, ks, s1, bias_s
    lds_floats += (size_t)p->C_pad * LDP + (size_t)p->NP * LDP + (size_t)p->C_pad * (p->C_pad + 4) + (size_t)p->C_pad * (p->NP + 4) + p->C_pad;
    q.lds = sizeof(float) * lds_floats;
    if (q.lds > CU_LDS_BYTES) return DLWP_E_UNSUPPORTED;
    q.f.s = make_spatial_dev(p, s);
    q.nob2 = second ? p->C_pad / 16 : 0;
    const double pix = (double)s->B * HW;
    q.flops = 2.0 * pix * p->C * (p->C + 2 * p->m2c) + 2.0 * pix * Ch1 * (p->C + Cout1);
    q.bytes = 4.0 * pix * p->C * 2 + 4.0 * pix * (p->C + Cout1);
    if (second) { q.flops += 2.0 * pix * Ch2 * (Cin2 + p->C); q.bytes += 4.0 * pix * (Cin2 + p->C); }
    return DLWP_OK;
}
static int proj_fwd_launch(const ProjFwdLaunch& q, const dlwp_fno_plan* p, int B, hipStream_t stream) {
    const int ncb = p->C_pad / 16, nbn = p->NP / 16;
    const dim3 grid(B * p->H);
    dlwp_prof_scope prof(stream, q.flops, q.bytes, "fno_spatial_proj_fwd_kernel<%d, %d, %d>", ncb, nbn, q.nob2);
    int rc;
#define LAUNCH(N, M, O)                                                                                            \
    {                                                                                                              \
        if ((rc = set_lds(fno_spatial_proj_fwd_kernel<N, M, O>, q.lds, "fno_spatial_proj_fwd")) != DLWP_OK) return rc; \
        hipLaunchKernelGGL((fno_spatial_proj_fwd_kernel<N, M, O>), grid, dim3(1024), q.lds, stream, q.f);           \
    }
    switch (ncb * 100 + nbn * 10 + q.nob2) {       // proj_fwd_prepare() has refused everything else
        case 110: LAUNCH(1, 1, 0) break; case 120: LAUNCH(1, 2, 0) break;
        case 210: LAUNCH(2, 1, 0) break; case 220: LAUNCH(2, 2, 0) break;
        case 310: LAUNCH(3, 1, 0) break; case 320: LAUNCH(3, 2, 0) break;
        case 111: LAUNCH(1, 1, 1) break; case 212: LAUNCH(2, 1, 2) break;
        default: return DLWP_E_UNSUPPORTED;
    }
#undef LAUNCH
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

// ---- one block: which launch forms, and their sequence.  The only readers of the four FNO knobs.
// (A narrow plan has 16 | W, one to four channel tiles and one or two frequency tiles -- plan_create_impl -- so every launcher
// below has an instantiation for what these functions let through.)

// Backward.  hosted: extra workgroups of the per-mode launch (most CUs idle through it) form the skip-weight / bias partials,
// which need only g_pre and the block's input, into the slab, and `spatial` runs its chain alone -- wherever that `spatial` would
// have taken the two-role kernel.  Block 0 takes this form only together with its fused lifting launch; where that one is
// refused it keeps the two-role `spatial`.  proj: the caller's next launch, the previous net call's projection backward, runs as
// the third phase of that fused launch (FNO_FUSE_PROJ_BWD); never without it, so FNO_FUSE_LIFT_BWD = 0 switches both off.
dlwp_fno_forms dlwp_fno_bwd_decide(const dlwp_fno_plan* p, const dlwp_fno_block_bwd_args* a) {
    const bool skip_in_mix = dlwp_tune_or("FNO_SKIP_WGRAD_IN_MIX", 1) != 0, fuse_lift = dlwp_tune_or("FNO_FUSE_LIFT_BWD", 1) != 0;
    const bool slab = a->gslab != nullptr, fits = !dlwp_fno_is_wide(p) && two_role_fits(p);
    const bool can_host = slab && fits && skip_in_mix;
    const dlwp_fno_lift_bwd_tail* t = a->lift;
    const bool can_lift = t && slab && !a->g_wskip && !a->g_bias && !a->act_in && !a->x1_out && t->slab && t->Ch >= 1 &&
                          lift_bwd_fused_lds(p, t->Cin) != 0 && fuse_lift;
    const bool can_proj = a->proj && can_lift && dlwp_tune_or("FNO_FUSE_PROJ_BWD", 1) != 0 && proj_bwd_fused_lds(p, t->Cin, a->proj) != 0;
    dlwp_fno_forms d{DLWP_OK, false, DLWP_FNO_SPATIAL_FOUR_WAVE, false};
    bool lift = false;
    switch (a->route) {
        case DLWP_FNO_ROUTE_PLAIN: break;
        case DLWP_FNO_ROUTE_HOSTED: d.hosted = true; if (!can_host) d.rc = DLWP_E_UNSUPPORTED; break;
        case DLWP_FNO_ROUTE_FUSED_TAIL:         // with a projection tail: forced as well
            lift = true; d.hosted = can_host; d.proj = a->proj != nullptr;
            if (!can_lift || (a->proj && !can_proj)) d.rc = DLWP_E_UNSUPPORTED;
            break;
        default: lift = a->first && can_lift; d.hosted = can_host && (!a->first || lift); d.proj = lift && can_proj; break;
    }
    if (lift) d.spatial = DLWP_FNO_SPATIAL_FUSED_TAIL;
    else if (!d.hosted && (slab || a->g_wskip) && fits) d.spatial = DLWP_FNO_SPATIAL_TWO_ROLE;   // dlwp_fno_spatial's own choice
    return d;
}

// Forward.  The last block's `spatial`, the projection and, behind it, the next call's lifting MLP as one launch on the training
// path (activations kept): the fused launch was built for and measured on the training step, and pwmlp_fwd_chain_kernel stays the
// kernel an evaluation rollout is tested on.  Instantiated without scratch and vector spills are C_pad 16 / 32 / 48 with the
// projection only, C_pad 16 / 32 with the chained lifting MLP (whose fused rows DFT needs NP == 16).
dlwp_fno_forms dlwp_fno_fwd_decide(const dlwp_fno_plan* p, const dlwp_fno_block_fwd_args* a) {
    const bool fuse_proj = dlwp_tune_or("FNO_FUSE_PROJ_FWD", 1) != 0;
    const dlwp_fno_proj_fwd_tail* t = a->proj;
    const bool second = t && t->x2v;
    const bool can_fuse = t && a->keep && fuse_proj && !dlwp_fno_is_wide(p) && p->W == PT && p->C_pad <= 48 && !a->x1_out && t->y1 &&
                          t->Ch1 >= 1 && t->Cout1 >= 1 && t->Cout1 <= 8 &&
                          (!second || (p->C_pad <= 32 && p->NP == 16 && t->x1_next && t->y2 && t->Cin2 >= 1 && t->Cin2 <= 64 && t->Ch2 >= 1));
    dlwp_fno_forms d{DLWP_OK, false, DLWP_FNO_SPATIAL_FOUR_WAVE, false};
    const bool fused = a->route == DLWP_FNO_ROUTE_FUSED_TAIL || (a->route == DLWP_FNO_ROUTE_AUTO && can_fuse);
    if (fused) d.spatial = DLWP_FNO_SPATIAL_FUSED_TAIL;
    if (fused && !can_fuse) d.rc = DLWP_E_UNSUPPORTED;
    return d;
}

int dlwp_fno_block_bwd_run(const dlwp_fno_plan* p, const dlwp_fno_block_bwd_args* a, hipStream_t stream) {
    const dlwp_fno_forms d = dlwp_fno_bwd_decide(p, a);
    if (d.rc) return d.rc;
    const bool fused = d.spatial == DLWP_FNO_SPATIAL_FUSED_TAIL;
    if (a->proj && a->proj->taken) *a->proj->taken = d.proj;
    int rc;
    if (a->rows_dft && (rc = dlwp_fno_rows_dft(p, a->g_pre, 0, 1, a->x1, a->B, stream))) return rc;
    rc = d.hosted ? mix_bwd_skipgrad_launch(p, a->x1, a->wspec, a->xhat, a->spec, a->g_wspec, a->g_pre, a->x, a->act_in, a->gslab,
                                            a->gslab_accumulate, a->B, stream)
                  : dlwp_fno_mix_bwd(p, a->x1, a->wspec, a->xhat, a->spec, a->g_wspec, a->B, stream);
    if (rc) return rc;
    dlwp_fno_spatial_args s{};
    s.tin = a->g_pre; s.spec = a->spec; s.wskip = a->wskip; s.transpose_w = 1; s.pprev = a->x; s.act_prev = a->act_in;
    s.out = fused ? nullptr : a->g_x;            // fused: the gradient of the lifting output stays in LDS
    s.x1_out = a->x1_out; s.x1_adjoint = 1; s.inverse_adjoint = 1; s.B = a->B;
    s.gslab_accumulate = a->gslab_accumulate;
    if (!d.hosted) { s.g_wskip = a->g_wskip; s.g_bias = a->g_bias; s.gslab = a->gslab; }
    const dlwp_fno_lift_bwd_tail* t = a->lift;
    if (fused) return spatial_lift_bwd_launch(p, &s, t, d.proj ? a->proj : nullptr, stream);
    if ((rc = dlwp_fno_spatial(p, &s, stream)) || !t) return rc;
    const int HW = p->H * p->W;
    const dlwp_chan_src gy{a->g_x, (long long)p->C * HW, HW, nullptr, nullptr};
    return dlwp_pwmlp_bwd_ex(t->x, t->w1, t->b1, t->w2, &gy, nullptr, nullptr, 0.f, t->gx, t->gx_accumulate, nullptr, t->gw1, t->gb1,
                             t->gw2, t->gb2, t->slab, t->slab_accumulate, a->B, t->Cin, t->Ch, p->C, HW, stream);
}

int dlwp_fno_block_fwd_run(const dlwp_fno_plan* p, const dlwp_fno_block_fwd_args* a, hipStream_t stream) {
    const dlwp_fno_forms d = dlwp_fno_fwd_decide(p, a);
    if (d.rc) return d.rc;
    const dlwp_fno_proj_fwd_tail* t = a->proj;
    bool fused = d.spatial == DLWP_FNO_SPATIAL_FUSED_TAIL;
    dlwp_fno_spatial_args s{};
    s.tin = a->x; s.act_tin = a->act_in; s.spec = a->spec; s.wskip = a->wskip; s.bias = a->bias; s.out = a->pre;
    s.x1_out = a->x1_out; s.x1_act = 1; s.B = a->B;
    ProjFwdLaunch q;
    int rc;
    if (fused && (rc = proj_fwd_prepare(q, p, &s, t))) {
        if (rc != DLWP_E_UNSUPPORTED || a->route != DLWP_FNO_ROUTE_AUTO) return rc;
        fused = false;                           // the projection chain's own refusal: the separate launches below
    }
    if (a->rows_dft && (rc = dlwp_fno_rows_dft(p, a->x, a->act_in, 0, a->x1, a->B, stream))) return rc;
    if ((rc = dlwp_fno_mix_fwd(p, a->x1, a->wspec, a->xhat, a->spec, a->B, stream))) return rc;
    if (t && t->lifted) *t->lifted = fused && t->x2v;
    if (fused) return proj_fwd_launch(q, p, a->B, stream);
    if ((rc = dlwp_fno_spatial(p, &s, stream)) || !t) return rc;
    // the projection chained with the next call's lifting MLP (the frames just produced go to the next window in LDS), or alone
    const int HW = p->H * p->W;
    const dlwp_chan_src ps{a->pre, (long long)p->C * HW, HW, nullptr, nullptr};
    if (t->x2v) {
        rc = dlwp_pwmlp_fwd_chain_ex(&ps, t->pw1, t->pb1, t->pw2, t->pb2, t->y1, t->res1, p->C, t->Ch1, t->Cout1, t->x2v, t->lw1, t->lb1,
                                     t->lw2, t->lb2, t->y2, t->Cin2, t->Ch2, p->C, t->next_ch, a->B, HW, p, t->x1_next, stream);
        if (rc == DLWP_OK && t->lifted) *t->lifted = 1;
        if (rc != DLWP_E_UNSUPPORTED) return rc;
    }
    return dlwp_pwmlp_fwd_ex(&ps, t->pw1, t->pb1, t->pw2, t->pb2, t->y1, t->res1, a->B, p->C, t->Ch1, t->Cout1, HW, stream);
}

// ---- exported entry points on contiguous tensors: argument adapters around the two routines (they add the leading rows DFT)
static dlwp_fno_block_bwd_args bwd_entry_args(const dlwp_fno_plan* p, const float* x, int act_in, const float* wspec,
                                              const float* wskip, const float* g_pre, const float* xhat, float* g_x, float* g_wspec,
                                              int B, void* workspace, int route) {
    const BlockWs ws = carve_ws(p, B, workspace);
    dlwp_fno_block_bwd_args a{};
    a.g_pre = g_pre; a.x = x; a.act_in = act_in; a.wspec = reinterpret_cast<const float2*>(wspec); a.wskip = wskip;
    a.xhat = reinterpret_cast<const float2*>(xhat); a.g_x = g_x; a.g_wspec = reinterpret_cast<float2*>(g_wspec);
    a.x1 = ws.x1; a.spec = ws.spec; a.rows_dft = 1; a.route = route; a.B = B;
    return a;
}
static dlwp_fno_block_fwd_args fwd_entry_args(const dlwp_fno_plan* p, const float* x, int act_in, const float* wspec,
                                              const float* wskip, const float* bias, float* pre, float* xhat, int B,
                                              void* workspace) {
    const BlockWs ws = carve_ws(p, B, workspace);
    dlwp_fno_block_fwd_args a{};
    a.x = x; a.act_in = act_in; a.wspec = reinterpret_cast<const float2*>(wspec); a.wskip = wskip; a.bias = bias; a.pre = pre;
    a.xhat = reinterpret_cast<float2*>(xhat); a.x1 = ws.x1; a.spec = ws.spec; a.rows_dft = 1; a.B = B;
    return a;
}

extern "C" int dlwp_fno_block_fwd(const dlwp_fno_plan* p, const float* x, int act_in, const float* wspec,
                                  const float* wskip, const float* bias, float* pre, float* xhat, int B,
                                  void* workspace, void* stream_) {
    DLWP_REQUIRE(p && x && wspec && wskip && pre && xhat && workspace && B > 0, DLWP_E_INVALID,
                 "fno_block_fwd: NULL argument or B<=0");
    const dlwp_fno_block_fwd_args a = fwd_entry_args(p, x, act_in, wspec, wskip, bias, pre, xhat, B, workspace);
    return dlwp_fno_block_fwd_run(p, &a, static_cast<hipStream_t>(stream_));
}

// dlwp_fno_block_bwd / _bwd_slab: `spatial` forms the skip gradients whatever the knobs say -- the reference of the bit-for-bit tests
extern "C" int dlwp_fno_block_bwd(const dlwp_fno_plan* p, const float* x, int act_in, const float* wspec,
                                  const float* wskip, const float* g_pre, const float* xhat, float* g_x,
                                  float* g_wspec, float* g_wskip, float* g_bias, int B, void* workspace,
                                  void* stream_) {
    DLWP_REQUIRE(p && x && wspec && wskip && g_pre && xhat && g_x && g_wspec && workspace && B > 0,
                 DLWP_E_INVALID, "fno_block_bwd: NULL argument or B<=0");
    dlwp_fno_block_bwd_args a = bwd_entry_args(p, x, act_in, wspec, wskip, g_pre, xhat, g_x, g_wspec, B, workspace, DLWP_FNO_ROUTE_PLAIN);
    a.g_wskip = g_wskip; a.g_bias = g_bias;
    return dlwp_fno_block_bwd_run(p, &a, static_cast<hipStream_t>(stream_));
}

extern "C" int dlwp_fno_block_bwd_slab(const dlwp_fno_plan* p, const float* x, int act_in, const float* wspec,
                                       const float* wskip, const float* g_pre, const float* xhat, float* g_x,
                                       float* g_wspec, float* slab, int slab_accumulate, int B, void* workspace,
                                       void* stream_) {
    DLWP_REQUIRE(p && x && wspec && wskip && g_pre && xhat && g_x && g_wspec && slab && workspace && B > 0,
                 DLWP_E_INVALID, "fno_block_bwd_slab: NULL argument or B<=0");
    DLWP_REQUIRE(!dlwp_fno_is_wide(p), DLWP_E_UNSUPPORTED, "fno_block_bwd_slab: narrow layers only (hidden_channels <= 64, 2-D plan)");
    dlwp_fno_block_bwd_args a = bwd_entry_args(p, x, act_in, wspec, wskip, g_pre, xhat, g_x, g_wspec, B, workspace, DLWP_FNO_ROUTE_PLAIN);
    a.gslab = slab; a.gslab_accumulate = slab_accumulate;
    return dlwp_fno_block_bwd_run(p, &a, static_cast<hipStream_t>(stream_));
}

// dlwp_fno_block_bwd_slab as the rollout trainer runs a block l > 0 with FNO_SKIP_WGRAD_IN_MIX on: rows DFT, the per-mode launch
// that also forms the slab, then the four-wave `spatial` chain without by-products.  Every output bit for bit
// dlwp_fno_block_bwd_slab's.  DLWP_E_UNSUPPORTED (error string untouched, nothing launched) for wide and 3-D plans, for shapes
// whose two-role layout does not fit, and with the knob at 0.
extern "C" int dlwp_fno_block_bwd_slab_split(const dlwp_fno_plan* p, const float* x, int act_in, const float* wspec,
                                             const float* wskip, const float* g_pre, const float* xhat, float* g_x,
                                             float* g_wspec, float* slab, int slab_accumulate, int B, void* workspace,
                                             void* stream_) {
    DLWP_REQUIRE(p && x && wspec && wskip && g_pre && xhat && g_x && g_wspec && slab && workspace && B > 0,
                 DLWP_E_INVALID, "fno_block_bwd_slab_split: NULL argument or B<=0");
    dlwp_fno_block_bwd_args a = bwd_entry_args(p, x, act_in, wspec, wskip, g_pre, xhat, g_x, g_wspec, B, workspace, DLWP_FNO_ROUTE_HOSTED);
    a.gslab = slab; a.gslab_accumulate = slab_accumulate;
    return dlwp_fno_block_bwd_run(p, &a, static_cast<hipStream_t>(stream_));
}

// block 0's backward with the lifting MLP's backward in its `spatial` launch, the per-mode form as the trainer picks it for
// block 0 (hosting the skip-gradient workgroups unless FNO_SKIP_WGRAD_IN_MIX = 0)
extern "C" int dlwp_fno_block_lift_bwd_slab(const dlwp_fno_plan* p, const float* h0, const float* wspec, const float* wskip,
                                            const float* g_pre, const float* xhat, float* g_wspec, float* slab_skip,
                                            int slab_skip_accumulate, const float* x, const float* w1, const float* b1,
                                            const float* w2, float* gx, int gx_accumulate, float* slab_lift,
                                            int slab_lift_accumulate, int B, int Cin, int Ch, void* workspace, void* stream_) {
    DLWP_REQUIRE(p && h0 && wspec && wskip && g_pre && xhat && g_wspec && slab_skip && x && w1 && b1 && w2 && slab_lift &&
                     workspace && B > 0 && Cin > 0 && Ch > 0,
                 DLWP_E_INVALID, "fno_block_lift_bwd_slab: NULL argument or non-positive dimension");
    const long long P = (long long)p->H * p->W;
    const dlwp_chan_src xs{x, (long long)Cin * P, P, nullptr, nullptr};
    const dlwp_chan_dst gxd{gx, (long long)Cin * P, P, nullptr, nullptr};
    dlwp_fno_lift_bwd_tail t{};
    t.x = &xs; t.w1 = w1; t.b1 = b1; t.w2 = w2; t.gx = gx ? &gxd : nullptr; t.gx_accumulate = gx_accumulate;
    t.slab = slab_lift; t.slab_accumulate = slab_lift_accumulate; t.Cin = Cin; t.Ch = Ch;
    dlwp_fno_block_bwd_args a = bwd_entry_args(p, h0, 0, wspec, wskip, g_pre, xhat, nullptr, g_wspec, B, workspace, DLWP_FNO_ROUTE_FUSED_TAIL);
    a.first = 1; a.gslab = slab_skip; a.gslab_accumulate = slab_skip_accumulate; a.lift = &t;
    const int rc = dlwp_fno_block_bwd_run(p, &a, static_cast<hipStream_t>(stream_));
    DLWP_REQUIRE(rc != DLWP_E_UNSUPPORTED, DLWP_E_UNSUPPORTED,
                 "fno_block_lift_bwd_slab: needs 64-wide rows, a narrow 2-D plan of at most 48 channels, Cin <= 32 and "
                 "FNO_FUSE_LIFT_BWD != 0 (use dlwp_fno_block_bwd_slab + dlwp_pwmlp_bwd_slab)");
    return rc;
}

// dlwp_fno_block_lift_bwd_slab with the scalar-output projection backward of the previous net call as the launch's third phase,
// forced.  px = that call's `pre` [B][C][H W]; gy = its closed-loop gradient plane, one [H W] plane per sample gy_bstride floats
// apart (in the rollout: a plane of the tensor the lifting phase accumulates into through gx); pred, target [B][1][H W]; gcur
// [B][C][H W] and x1_out [B][H][m2c][C] complex are overwritten.  DLWP_E_UNSUPPORTED, nothing launched, where the trainer keeps
// the projection backward on its own launch.
extern "C" int dlwp_fno_block_lift_proj_bwd_slab(const dlwp_fno_plan* p, const float* h0, const float* wspec, const float* wskip,
                                                 const float* g_pre, const float* xhat, float* g_wspec, float* slab_skip,
                                                 int slab_skip_accumulate, const float* x, const float* w1, const float* b1,
                                                 const float* w2, float* gx, int gx_accumulate, float* slab_lift,
                                                 int slab_lift_accumulate, int B, int Cin, int Ch, const float* px,
                                                 const float* pw1, const float* pb1, const float* pw2, const float* gy,
                                                 long long gy_bstride, const float* pred, const float* target, float mse_scale,
                                                 const float* gres, float* gcur, float* x1_out, float* slab_proj,
                                                 int slab_proj_accumulate, int PCh, int PCout, void* workspace, void* stream_) {
    DLWP_REQUIRE(p && h0 && wspec && wskip && g_pre && xhat && g_wspec && slab_skip && x && w1 && b1 && w2 && slab_lift &&
                     px && pw1 && pb1 && pw2 && gy && pred && target && gcur && x1_out && slab_proj && workspace && B > 0 &&
                     Cin > 0 && Ch > 0 && PCh > 0 && PCout > 0,
                 DLWP_E_INVALID, "fno_block_lift_proj_bwd_slab: NULL argument or non-positive dimension");
    if (gres) return DLWP_E_UNSUPPORTED;            // a residual path's gradient: the stand-alone launch only
    const long long P = (long long)p->H * p->W;
    const dlwp_chan_src xs{x, (long long)Cin * P, P, nullptr, nullptr};
    const dlwp_chan_dst gxd{gx, (long long)Cin * P, P, nullptr, nullptr};
    dlwp_fno_lift_bwd_tail t{};
    t.x = &xs; t.w1 = w1; t.b1 = b1; t.w2 = w2; t.gx = gx ? &gxd : nullptr; t.gx_accumulate = gx_accumulate;
    t.slab = slab_lift; t.slab_accumulate = slab_lift_accumulate; t.Cin = Cin; t.Ch = Ch;
    const dlwp_chan_src ps{px, p->C * P, P, nullptr, nullptr}, gys{gy, gy_bstride, P, nullptr, nullptr};
    const dlwp_chan_src pr{pred, PCout * P, P, nullptr, nullptr}, tg{target, PCout * P, P, nullptr, nullptr};
    const dlwp_chan_dst gc{gcur, p->C * P, P, nullptr, nullptr};
    dlwp_fno_proj_bwd_tail q{};
    q.x = &ps; q.w1 = pw1; q.b1 = pb1; q.w2 = pw2; q.gy = &gys; q.pred = &pr; q.target = &tg; q.mse_scale = mse_scale; q.gx = &gc;
    q.x1_out = reinterpret_cast<float2*>(x1_out); q.slab = slab_proj; q.slab_accumulate = slab_proj_accumulate; q.Ch = PCh; q.Cout = PCout;
    dlwp_fno_block_bwd_args a = bwd_entry_args(p, h0, 0, wspec, wskip, g_pre, xhat, nullptr, g_wspec, B, workspace, DLWP_FNO_ROUTE_FUSED_TAIL);
    a.first = 1; a.gslab = slab_skip; a.gslab_accumulate = slab_skip_accumulate; a.lift = &t; a.proj = &q;
    return dlwp_fno_block_bwd_run(p, &a, static_cast<hipStream_t>(stream_));
}

// the second of the two launches dlwp_fno_block_lift_proj_bwd_slab replaces, on the same tensors: the projection backward as the
// rollout trainer issues it (dlwp_pwmlp_bwd_rows_ex in slab mode with the MSE term and the adjoint rows DFT)
extern "C" int dlwp_pwmlp_proj_bwd_rows_slab(const dlwp_fno_plan* p, const float* px, const float* pw1, const float* pb1,
                                             const float* pw2, const float* gy, long long gy_bstride, const float* pred,
                                             const float* target, float mse_scale, float* gcur, float* x1_out, float* slab_proj,
                                             int slab_proj_accumulate, int B, int PCh, int PCout, void* stream_) {
    DLWP_REQUIRE(p && px && pw1 && pb1 && pw2 && gy && pred && target && gcur && x1_out && slab_proj && B > 0 && PCh > 0 && PCout > 0,
                 DLWP_E_INVALID, "pwmlp_proj_bwd_rows_slab: NULL argument or non-positive dimension");
    const long long P = (long long)p->H * p->W;
    const dlwp_chan_src ps{px, p->C * P, P, nullptr, nullptr}, gys{gy, gy_bstride, P, nullptr, nullptr};
    const dlwp_chan_src pr{pred, PCout * P, P, nullptr, nullptr}, tg{target, PCout * P, P, nullptr, nullptr};
    const dlwp_chan_dst gc{gcur, p->C * P, P, nullptr, nullptr};
    return dlwp_pwmlp_bwd_rows_ex(&ps, pw1, pb1, pw2, &gys, &pr, &tg, mse_scale, &gc, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  slab_proj, slab_proj_accumulate, B, p->C, PCh, PCout, (int)P, p, reinterpret_cast<float2*>(x1_out),
                                  static_cast<hipStream_t>(stream_));
}

// Test entry points.  dlwp_fno_block_proj_fwd: one FNO block (rows DFT, per-mode stage) whose `spatial` stage is the fused launch:
// pre, xhat as dlwp_fno_block_fwd; frame [B, Cout1, H, W] = projection(pre) (+ res); and, with window != NULL,
// h0_next [B, C, H, W] = lifting(window [B, Cin2, H, W] with channel next_ch[o] >= 0 taken from frame channel o, in LDS) and its
// rows DFT x1_next [B][H][m2c][C] complex.  DLWP_E_UNSUPPORTED, nothing launched, where the trainer keeps the two launches.
// dlwp_pwmlp_proj_lift_fwd: the second of those two launches (pwmlp_fwd_chain_kernel, or pwmlp_fwd_kernel without a window) on
// the same tensors, behind dlwp_fno_block_fwd.
extern "C" int dlwp_fno_block_proj_fwd(const dlwp_fno_plan* p, const float* x, int act_in, const float* wspec, const float* wskip,
                                       const float* bias, float* pre, float* xhat, const float* pw1, const float* pb1,
                                       const float* pw2, const float* pb2, const float* res, float* frame, int Ch1, int Cout1,
                                       const float* window, const float* lw1, const float* lb1, const float* lw2, const float* lb2,
                                       float* h0_next, float* x1_next, int Cin2, int Ch2, const signed char* next_ch, int B,
                                       void* workspace, void* stream_) {
    DLWP_REQUIRE(p && x && wspec && wskip && pre && xhat && pw1 && pb1 && pw2 && pb2 && frame && workspace && B > 0 &&
                     (!window || (lw1 && lb1 && lw2 && lb2 && h0_next && x1_next && next_ch)),
                 DLWP_E_INVALID, "fno_block_proj_fwd: NULL argument or B<=0");
    const long long HW = (long long)p->H * p->W;
    const dlwp_chan_dst fd{frame, Cout1 * HW, HW, nullptr, nullptr};
    const dlwp_chan_src rs{res, Cout1 * HW, HW, nullptr, nullptr};
    const dlwp_chan_src wsrc{window, Cin2 * HW, HW, nullptr, nullptr};
    const dlwp_chan_dst hd{h0_next, p->C * HW, HW, nullptr, nullptr};
    dlwp_fno_proj_fwd_tail t{};
    t.pw1 = pw1; t.pb1 = pb1; t.pw2 = pw2; t.pb2 = pb2; t.y1 = &fd; t.res1 = res ? &rs : nullptr; t.Ch1 = Ch1; t.Cout1 = Cout1;
    t.x2v = window ? &wsrc : nullptr; t.lw1 = lw1; t.lb1 = lb1; t.lw2 = lw2; t.lb2 = lb2; t.y2 = &hd; t.Cin2 = Cin2; t.Ch2 = Ch2;
    t.next_ch = next_ch; t.x1_next = reinterpret_cast<float2*>(x1_next);
    dlwp_fno_block_fwd_args a = fwd_entry_args(p, x, act_in, wspec, wskip, bias, pre, xhat, B, workspace);
    a.proj = &t; a.keep = 1; a.route = DLWP_FNO_ROUTE_FUSED_TAIL;
    return dlwp_fno_block_fwd_run(p, &a, static_cast<hipStream_t>(stream_));
}

extern "C" int dlwp_pwmlp_proj_lift_fwd(const dlwp_fno_plan* p, const float* pre, const float* pw1, const float* pb1,
                                        const float* pw2, const float* pb2, const float* res, float* frame, int Ch1, int Cout1,
                                        const float* window, const float* lw1, const float* lb1, const float* lw2,
                                        const float* lb2, float* h0_next, float* x1_next, int Cin2, int Ch2,
                                        const signed char* next_ch, int B, void* stream_) {
    DLWP_REQUIRE(p && pre && pw1 && pb1 && pw2 && pb2 && frame && B > 0 &&
                     (!window || (lw1 && lb1 && lw2 && lb2 && h0_next && x1_next && next_ch)),
                 DLWP_E_INVALID, "pwmlp_proj_lift_fwd: NULL argument or B<=0");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const long long HW = (long long)p->H * p->W;
    const dlwp_chan_src ps{pre, p->C * HW, HW, nullptr, nullptr};
    const dlwp_chan_dst fd{frame, Cout1 * HW, HW, nullptr, nullptr};
    const dlwp_chan_src rs{res, Cout1 * HW, HW, nullptr, nullptr};
    if (!window) return dlwp_pwmlp_fwd_ex(&ps, pw1, pb1, pw2, pb2, &fd, res ? &rs : nullptr, B, p->C, Ch1, Cout1, (int)HW, stream);
    const dlwp_chan_src wsrc{window, Cin2 * HW, HW, nullptr, nullptr};
    const dlwp_chan_dst hd{h0_next, p->C * HW, HW, nullptr, nullptr};
    const int rc = dlwp_pwmlp_fwd_chain_ex(&ps, pw1, pb1, pw2, pb2, &fd, res ? &rs : nullptr, p->C, Ch1, Cout1, &wsrc, lw1, lb1, lw2, lb2,
                                           &hd, Cin2, Ch2, p->C, next_ch, B, (int)HW, p, reinterpret_cast<float2*>(x1_next), stream);
    DLWP_REQUIRE(rc != DLWP_E_UNSUPPORTED, DLWP_E_UNSUPPORTED, "pwmlp_proj_lift_fwd: these shapes do not take the chained launch");
    return rc;
}

extern "C" int dlwp_fno_block_slab_fold(const dlwp_fno_plan* p, const float* slab, float* g_wskip, float* g_bias, int B,
                                        void* stream) {
    DLWP_REQUIRE(p && slab && g_wskip && g_bias && B > 0, DLWP_E_INVALID, "fno_block_slab_fold: NULL argument or B<=0");
    dlwp_fold_job q{};
    q.slab = slab; q.nslab = B * p->H; q.stride = dlwp_fno_gslab_stride(p->C);
    q.d1 = g_wskip; q.n1 = (long long)p->C * p->C; q.d2 = g_bias; q.n2 = p->C;
    return dlwp_fold_slabs(&q, 1, static_cast<hipStream_t>(stream));
}

#ifdef DLWP_STAMPS
extern "C" int dlwp_debug_span_fno(unsigned long long* host_out, int reset) {
    DLWP_HIP(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_dlwp_span), sizeof(unsigned long long) * 2));
    if (reset) {
        const unsigned long long init[2] = {~0ull, 0ull};
        DLWP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_dlwp_span), init, sizeof(init)));
    }
    return DLWP_OK;
}
extern "C" int dlwp_debug_stamps_fno(unsigned long long* host_out) {
    DLWP_HIP(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_dlwp_stamps), sizeof(unsigned long long) * 32));
    return DLWP_OK;
}
#endif

long long dlwp_fno_gslab_stride(int C) { return ((long long)C * C + C + 3) & ~3LL; }

// one forward `spatial` launch exactly as the rollout issues it for an inner block (GELU on load,
// fused rows-DFT of gelu(result)); exposed so bench.py can time the dominant kernel with HIP events.
extern "C" int dlwp_fno_spatial_fwd_probe(const dlwp_fno_plan* p, const float* x, const float* spec, const float* wskip,
                                          const float* bias, float* pre, float* x1_out, int B, void* stream) {
    DLWP_REQUIRE(p && x && spec && wskip && pre && x1_out && B > 0, DLWP_E_INVALID, "spatial_fwd_probe: NULL argument");
    dlwp_fno_spatial_args s{};
    s.tin = x; s.act_tin = 1; s.spec = reinterpret_cast<const float2*>(spec); s.wskip = wskip; s.bias = bias;
    s.out = pre; s.x1_out = reinterpret_cast<float2*>(x1_out); s.x1_act = 1; s.B = B;
    return dlwp_fno_spatial(p, &s, static_cast<hipStream_t>(stream));
}

// one forward per-mode launch (H-axis step + complex channel contraction on MFMA) exactly as the rollout issues it; exposed
// so bench.py can time the spectral contraction with HIP events (roofline_mix)
extern "C" int dlwp_fno_mix_fwd_probe(const dlwp_fno_plan* p, const float* x1, const float* wspec, float* xhat, float* y, int B,
                                      void* stream) {
    DLWP_REQUIRE(p && x1 && wspec && xhat && y && B > 0, DLWP_E_INVALID, "mix_fwd_probe: NULL argument");
    return dlwp_fno_mix_fwd(p, reinterpret_cast<const float2*>(x1), reinterpret_cast<const float2*>(wspec),
                            reinterpret_cast<float2*>(xhat), reinterpret_cast<float2*>(y), B, static_cast<hipStream_t>(stream));
}
