// What the pointwise-MLP backward body (pwmlp_bwd_body.inc.h) needs around it: tile constants, channel views, weight
// fragments straight from global memory, the pixel-tile staging and the argument block.  Shared by pwmlp.hip and by the
// fused FNO `spatial` + lifting backward launches of fno_block.hip (the second of which runs the body twice: the lifting backward
// and the previous net call's projection backward).
#pragma once
#include "common.hip.h"
#include "dlwpmi_internal.h"

namespace {

constexpr int PT = 64;        // pixels per workgroup
constexpr int BWD_WAVES = 8;   // (4 waves with two hidden blocks in flight each, 352 VGPRs, was measured: 1884 samples/s against 2020;
                               // plain 4 waves: 1858)
constexpr int LDP = PT + 4;   // LDS row stride of pixel tiles (4*LDP % 32 == 16: conflict-free B reads)

__device__ __forceinline__ const float* chan_ptr(const dlwp_chan_src& s, int b, int c) {
    if (s.tab) return s.tab[c] ? s.tab[c] + (long long)b * s.tab_bstride[c] : nullptr;
    return s.base + (long long)b * s.bstride + (long long)c * s.cstride;
}
__device__ __forceinline__ float* chan_ptr(const dlwp_chan_dst& s, int b, int c) {
    if (s.tab) return s.tab[c] ? s.tab[c] + (long long)b * s.tab_bstride[c] : nullptr;
    return s.base ? s.base + (long long)b * s.bstride + (long long)c * s.cstride : nullptr;
}

// MFMA fragments of a dense row-major [R][K] matrix straight from global memory (L2 / L1 resident weights), zero outside the
// matrix.  Loads are unconditional from clamped addresses with the select afterwards, so that a group of them is in flight
// together.  frag_row: element s = M[row][k + s] (vec: K % 4 == 0 and a 16-byte aligned base, k a multiple of 4);
// frag_col: element s = M[row + s][col].
__device__ __forceinline__ f32x4 frag_row(const float* __restrict__ M, int R, int K, int row, int k, bool vec) {
    f32x4 v;
    if (vec) {
        const bool ok = row < R && k < K;
        v = *reinterpret_cast<const f32x4*>(M + (ok ? (long long)row * K + k : 0));
        if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bool ok = row < R && k + s < K;
            const float x = M[ok ? (long long)row * K + k + s : 0];
            v[s] = ok ? x : 0.f;
        }
    }
    return v;
}
__device__ __forceinline__ f32x4 frag_col(const float* __restrict__ M, int R, int K, int row, int col) {
    f32x4 v;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const bool ok = row + s < R && col < K;
        const float x = M[ok ? (long long)(row + s) * K + col : 0];
        v[s] = ok ? x : 0.f;
    }
    return v;
}

// pixel tile [C_pad][PT] of a channel view -> LDS (row stride LDP); 16-byte loads along pixels
// (channels in `skip` are left alone: a fused producer in the same workgroup writes them); NT, T0: see wg_stride / wg_thread
template <int NT = 0, int T0 = 0, typename SRC>
__device__ __forceinline__ void stage_pixels(float* dst, const SRC& s, int b, int C, int C_pad, int p0, int P,
                                             bool vec_ok, unsigned long long skip = 0ull) {
    if (vec_ok) {
#pragma unroll 2
        for (int u = wg_thread<T0>(); u < C_pad * (PT / 4); u += wg_stride<NT>()) {
            const int c = u / (PT / 4), q = u % (PT / 4);
            if (c < 64 && ((skip >> c) & 1ull)) continue;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < C && p0 + 4 * q < P) {
                const float* src = chan_ptr(s, b, c);
                if (src) v = *reinterpret_cast<const float4*>(src + p0 + 4 * q);
            }
            *reinterpret_cast<float4*>(&dst[c * LDP + 4 * q]) = v;
        }
    } else {
        for (int idx = wg_thread<T0>(); idx < C_pad * PT; idx += wg_stride<NT>()) {
            const int c = idx / PT, p = idx % PT;
            if (c < 64 && ((skip >> c) & 1ull)) continue;
            float v = 0.f;
            if (c < C && p0 + p < P) {
                const float* src = chan_ptr(s, b, c);
                if (src) v = src[p0 + p];
            }
            dst[c * LDP + p] = v;
        }
    }
}

struct BwdArgs {
    dlwp_chan_src x;
    const float *w1, *b1, *w2;
    dlwp_chan_src gy;            // upstream gradient (may be absent)
    dlwp_chan_src pred, target;  // optional MSE term: gy_eff += mse_scale * (pred - target)
    float mse_scale;
    dlwp_chan_dst gx;            // nullable; per-channel nullable in table mode
    int gx_accumulate;
    dlwp_chan_dst gres;          // optional: gres += effective upstream gradient (identity path of a residual)
    float *gw1, *gb1, *gw2, *gb2;  // accumulated with float atomics (slab == nullptr)
    // optional per-workgroup partial slab [grid][slab_stride] laid out {gw1,gb1,gw2,gb2}: plain
    // stores (slab_accumulate == 0) or read-modify-write by the owning workgroup; deterministic and
    // not bound by the chip-wide float-atomic rate.  dlwp_pwmlp_slab_reduce folds it into the grads.
    float* slab;
    long long slab_stride;
    int slab_accumulate;
    int B, Cin, Ch, Cout, P, tiles_per_sample;
    int Cin_pad, Ch_pad, Cout_pad;
    int vec_w, vec_x;
    FastDiv dCin, dCh;
    // optional fused W-axis DFT (adjoint table) of the finished gx row -- projection backward -> last spectral block's
    // backward without a separate rows launch; needs PT == W, NP == 16, dense gx, gx_accumulate == 0
    float2* x1_out;
    const float* FT;
    int rows_H, m2c;
};

__device__ __forceinline__ void grad_flush(float* slab_ptr, float* grad_ptr, bool accumulate, float v) {
    if (slab_ptr) *slab_ptr = accumulate ? *slab_ptr + v : v;
    else atomic_add_f32(grad_ptr, v);
}

constexpr int TPS = 20;       // row stride of a wave's 16 x 16 transpose tile: 16-byte row writes and 4-byte column reads both conflict-free

// orders a wave's own LDS writes against its own later reads of other lanes' words (the LDS executes one wave's instructions in
// order; this only keeps the compiler from moving them): no workgroup barrier, no instruction
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
template <typename V>
bool view_vec_ok(const V& v) {
    if (v.tab) return true;  // table views are built by the trainer from 16-byte aligned planes
    if (!v.base) return true;
    return aligned16(v.base) && v.bstride % 4 == 0 && v.cstride % 4 == 0;
}

}  // namespace
