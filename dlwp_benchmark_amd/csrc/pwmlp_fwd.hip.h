// The forward pointwise MLP of one 64-pixel tile in pieces (argument block, LDS images, issue / commit / compute / finish) and
// the argument block of the chained projection -> next lifting launch.  Shared by pwmlp.hip (pwmlp_fwd_kernel,
// pwmlp_fwd_chain_kernel) and by the fused last-block `spatial` + projection chain launch of fno_block.hip.
#pragma once
#include "common.hip.h"
#include "dlwpmi_internal.h"
#include "fno_rows.hip.h"
#include "pwmlp_bwd.hip.h"

namespace {

constexpr int FWD_WAVES = 16; // 4 waves per SIMD: the forward kernel needs 54 VGPRs and its main loop is bound by the dependent
                              // z -> GELU -> second-GEMM chain of a wave, not by the matrix pipe (8 waves: 1993, 16 waves: 2007 samples/s)

struct FwdArgs {
    dlwp_chan_src x;
    const float *w1, *b1, *w2, *b2;
    dlwp_chan_dst y;
    dlwp_chan_src res;  // optional residual added to y (base==nullptr && tab==nullptr: none)
    int B, Cin, Ch, Cout, P, tiles_per_sample;
    int Cin_pad, Ch_pad, Cout_pad;
    int vec_w, vec_x;   // 16-byte loads allowed for the weights / the pixel planes
    FastDiv dCin, dCh;
    // optional fused W-axis DFT of the output row (lifting MLP -> first spectral block): needs PT == W, NP == 16
    float2* x1_out;
    const float* FT;
    int rows_H, m2c;
};

// ---- forward MLP of one 64-pixel tile, in pieces that a kernel strings together (pwmlp_fwd_kernel and the chained
// projection -> next lifting kernel of pwmlp.hip, fno_spatial_proj_fwd_kernel of fno_block.hip): issue (global loads into registers) -> commit (LDS images) -> barrier ->
// compute (both GEMMs) -> barrier -> finish (reduce the hidden groups' partial tiles, bias, residual, store, optional rows DFT).
struct FwdLds {
    float *xs, *w1s, *w2s, *b1s, *b2s, *outs;
};
// LDS floats of one MLP: input tile, the two weight images, biases (the partial output tiles `outs` are counted separately)
__host__ __device__ __forceinline__ size_t fwd_lds_floats(int Cin_pad, int Ch_pad, int Cout_pad) {
    return (size_t)Cin_pad * LDP + (size_t)Ch_pad * (Cin_pad + 4) + (size_t)Cout_pad * (Ch_pad + 4) + Ch_pad + Cout_pad;
}
__device__ __forceinline__ FwdLds fwd_carve(float* base, const FwdArgs& a, float* outs) {
    FwdLds L;
    L.xs = base;
    L.w1s = L.xs + a.Cin_pad * LDP;
    L.w2s = L.w1s + a.Ch_pad * (a.Cin_pad + 4);
    L.b1s = L.w2s + a.Cout_pad * (a.Ch_pad + 4);
    L.b2s = L.b1s + a.Ch_pad;
    L.outs = outs ? outs : L.b2s + a.Cout_pad;      // [HQ][Cout_pad][LDP] per-hidden-group partial output tiles
    return L;
}
// U1: 16-byte units of W1 a thread holds (2 with the whole workgroup of 1024 staging; 3 where 768 threads do)
template <int U1>
struct FwdLoadsT {
    MatLoad<4> l2;
    MatLoad<U1> l1;
    float4 ftv;          // DFT table [16][PT] of the fused rows step
    int n1, n2;
};
using FwdLoads = FwdLoadsT<2>;
// NTS, T0: the threads that stage (see wg_stride / wg_thread; the whole workgroup by default).  A sub-range (T0 != 0) leaves the
// DFT table to the kernel: fwd_finish takes it from threads 0 .. 255.
template <int NTS = 0, int T0 = 0, int U1 = 2>
__device__ __forceinline__ void fwd_issue(const FwdArgs& a, FwdLoadsT<U1>& q) {
    q.n2 = matload_units<NTS>(a.Cout, a.Ch, a.vec_w != 0, 4);
    q.n1 = matload_units<NTS>(a.Ch, a.Cin, a.vec_w != 0, U1);
    q.l2.template issue<NTS, T0>(a.w2, q.n2);
    q.l1.template issue<NTS, T0>(a.w1, q.n1);
    q.ftv = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (T0 == 0)
        if (a.x1_out && threadIdx.x < 16 * (PT / 4)) q.ftv = reinterpret_cast<const float4*>(a.FT)[threadIdx.x];
}
template <int NTS = 0, int T0 = 0, int U1 = 2>
__device__ __forceinline__ void fwd_commit(const FwdArgs& a, const FwdLds& L, const FwdLoadsT<U1>& q) {
    const int LD1 = a.Cin_pad + 4, LD2 = a.Ch_pad + 4, tid = wg_thread<T0>(), NT = wg_stride<NTS>();
    q.l2.template commit<false, NTS, T0>(L.w2s, LD2, a.Ch, a.dCh, q.n2);
    q.l1.template commit<false, NTS, T0>(L.w1s, LD1, a.Cin, a.dCin, q.n1);
    stage_matrix_tail<false, NTS, T0>(L.w2s, LD2, a.w2, a.Cout, a.Ch, a.dCh, q.n2);
    stage_matrix_tail<false, NTS, T0>(L.w1s, LD1, a.w1, a.Ch, a.Cin, a.dCin, q.n1);
    zero_padding<NTS, T0>(L.w1s, LD1, a.Ch, a.Cin, a.Ch_pad, a.Cin_pad);
    zero_padding<NTS, T0>(L.w2s, LD2, a.Cout, a.Ch, a.Cout_pad, a.Ch_pad);
    for (int idx = tid; idx < a.Ch_pad; idx += NT) L.b1s[idx] = idx < a.Ch ? a.b1[idx] : 0.f;
    for (int idx = tid; idx < a.Cout_pad; idx += NT) L.b2s[idx] = idx < a.Cout ? a.b2[idx] : 0.f;
}
// NW waves: wave w owns pixel block (w & 3) and the hidden blocks hq, hq+HQ, ... (hq = w >> 2,
// HQ = NW/4); two or more waves per SIMD overlap one wave's GELU (VALU) with another's MFMAs.
template <int NOB, int NW>
__device__ __forceinline__ void fwd_compute(const FwdArgs& a, const FwdLds& L) {
    constexpr int HQ = NW / 4;
    const int LD1 = a.Cin_pad + 4, LD2 = a.Ch_pad + 4;
    const int lane = lane_id(), w = wave_id(), r = lane & 15, g = lane >> 4;
    const int pw0 = (w & 3) * 16, hq = w >> 2;
    const int nkc = a.Cin_pad / 16, nhb = a.Ch_pad / 16;
    f32x4 oacc[NOB];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) oacc[ob] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int hb = hq; hb < nhb; hb += HQ) {
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int kc = 0; kc < nkc; ++kc) {
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(&L.w1s[(hb * 16 + r) * LD1 + kc * 16 + 4 * g]);
            f32x4 b4;
#pragma unroll
            for (int s = 0; s < 4; ++s) b4[s] = L.xs[(kc * 16 + 4 * g + s) * LDP + pw0 + r];
            z = mfma16_chunk(a4, b4, z);
        }
        {
            const f32x4 zb = z + *reinterpret_cast<const f32x4*>(&L.b1s[hb * 16 + 4 * g]);
            f32x4 dz;
            gelu_both4(zb, z, dz);                      // packed fp32 polynomial (the derivative half is dead code here)
        }
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) {
            const f32x4 w4 = *reinterpret_cast<const f32x4*>(&L.w2s[(ob * 16 + r) * LD2 + hb * 16 + 4 * g]);
            oacc[ob] = mfma16_chunk(w4, z, oacc[ob]);
        }
    }
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            L.outs[(hq * a.Cout_pad + ob * 16 + 4 * g + j) * LDP + pw0 + r] = oacc[ob][j];
        }
}
// next_xs / next_ch: a chained MLP's input tile in LDS and, per output channel, the input channel of that tile the finished
// values are copied to (-1: none) -- the consumer then never reads them back from global memory
template <int NOB, int NW>
__device__ __forceinline__ void fwd_finish(const FwdArgs& a, const FwdLds& L, const float4 ftv, int b, int p0, int tile,
                                           float* next_xs = nullptr, const signed char* next_ch = nullptr) {
    constexpr int NT = NW * 64, HQ = NW / 4;
    const int tid = threadIdx.x, w = wave_id();
    float* outs = L.outs;
    const bool has_res = a.res.base || a.res.tab;
    if (a.vec_x) {
        for (int u = tid; u < a.Cout * (PT / 4); u += NT) {
            const int o = u / (PT / 4), q = u % (PT / 4), p = p0 + 4 * q;
            if (p < a.P) {
                float4 v = *reinterpret_cast<const float4*>(&outs[o * LDP + 4 * q]);
#pragma unroll
                for (int h2 = 1; h2 < HQ; ++h2) {
                    const float4 pv = *reinterpret_cast<const float4*>(&outs[(h2 * a.Cout_pad + o) * LDP + 4 * q]);
                    v.x += pv.x; v.y += pv.y; v.z += pv.z; v.w += pv.w;
                }
                const float bb = L.b2s[o];
                v.x += bb; v.y += bb; v.z += bb; v.w += bb;
                if (has_res) {
                    const float* rp = chan_ptr(a.res, b, o);
                    if (rp) {
                        const float4 rv = *reinterpret_cast<const float4*>(rp + p);
                        v.x += rv.x; v.y += rv.y; v.z += rv.z; v.w += rv.w;
                    }
                }
                float* dst = chan_ptr(a.y, b, o);
                if (dst) *reinterpret_cast<float4*>(dst + p) = v;
                if (a.x1_out) *reinterpret_cast<float4*>(&outs[o * LDP + 4 * q]) = v;   // finished row tile, in place
                if (next_xs && o < 8 && next_ch[o] >= 0) *reinterpret_cast<float4*>(&next_xs[next_ch[o] * LDP + 4 * q]) = v;
            }
        }
        if (a.x1_out) {
            // W-axis pruned DFT of the finished row, so that the first spectral block needs no separate rows kernel.
            // The W2 image is dead: it hosts the table and the per-wave partial spectra.
            float* ft = L.w2s;                       // [16][LDP]
            float* x1s = L.w2s + 16 * LDP;           // [4 waves][Cout_pad][16]
            if (tid < 16 * (PT / 4)) *reinterpret_cast<float4*>(&ft[(tid / (PT / 4)) * LDP + 4 * (tid % (PT / 4))]) = ftv;
            for (int idx = a.Cout * LDP + tid; idx < a.Cout_pad * LDP; idx += NT) outs[idx] = 0.f;
            __syncthreads();
            if (w < 4) tile_rows_dft<NOB, 1>(outs, ft, x1s, LDP, 16, PT / 16, false);
            __syncthreads();
            store_x1(x1s, a.x1_out, b, tile, a.rows_H, a.m2c, a.Cout, a.Cout_pad, 16);
        }
    } else {
        for (int idx = tid; idx < a.Cout * PT; idx += NT) {
            const int o = idx / PT, p = p0 + idx % PT;
            if (p < a.P) {
                float v = L.b2s[o];
#pragma unroll
                for (int h2 = 0; h2 < HQ; ++h2) v += outs[(h2 * a.Cout_pad + o) * LDP + idx % PT];
                if (has_res) {
                    const float* rp = chan_ptr(a.res, b, o);
                    if (rp) v += rp[p];
                }
                float* dst = chan_ptr(a.y, b, o);
                if (dst) dst[p] = v;
            }
        }
    }
}

// Projection of net call k chained with the lifting of net call k + 1 (both pointwise, the same 64-pixel tile): the rollout's
// closed loop feeds the frame the projection has just produced straight into the next lifting layer's input tile, in LDS.
struct ChainArgs {
    FwdArgs p, l;
    signed char next_ch[8];        // output channel o of the first MLP -> input channel of the second (-1: none)
    unsigned long long skip;       // input channels of the second MLP that come from the first
};

// fills and validates the launch arguments of one forward MLP; rows_after: the rows DFT was asked for but the epilogue
// cannot host it (the caller runs the separate rows kernel)
int fwd_make_args(FwdArgs& a, const dlwp_chan_src* x, const float* w1, const float* b1, const float* w2,
                         const float* b2, const dlwp_chan_dst* y, const dlwp_chan_src* res, int B, int Cin, int Ch, int Cout,
                         int P, const dlwp_fno_plan* rows_plan, float2* x1_out, bool& rows_after) {
    DLWP_REQUIRE(B > 0 && Cin > 0 && Ch > 0 && Cout > 0 && P > 0, DLWP_E_INVALID,
                 "pwmlp_fwd: non-positive dimension");
    a = FwdArgs{};
    a.x = *x; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.y = *y;
    if (res) a.res = *res;
    a.B = B; a.Cin = Cin; a.Ch = Ch; a.Cout = Cout; a.P = P;
    a.tiles_per_sample = ceil_div(P, PT);
    a.Cin_pad = round_up(Cin, 16); a.Ch_pad = round_up(Ch, 16); a.Cout_pad = round_up(Cout, 16);
    a.vec_w = aligned16(w1) && aligned16(w2);
    a.dCin = make_fastdiv(Cin); a.dCh = make_fastdiv(Ch);
    a.vec_x = P % 4 == 0 && view_vec_ok(a.x);
    const int nob = a.Cout_pad / 16;
    DLWP_REQUIRE(nob <= 4 && a.Cin_pad <= 64, DLWP_E_UNSUPPORTED,
                 "pwmlp_fwd: Cin<=64 and Cout<=64 supported (got %d, %d)", Cin, Cout);
    a.vec_x = a.vec_x && view_vec_ok(a.y) && view_vec_ok(a.res);
    rows_after = false;
    if (x1_out) {
        DLWP_REQUIRE(rows_plan && y->base, DLWP_E_INVALID, "pwmlp_fwd: the rows DFT needs a plan and a dense output");
        const bool fuse = dlwp_pwmlp_rows_fusable(rows_plan, Cout, P) && a.vec_x &&
                          (size_t)a.Cout_pad * (a.Ch_pad + 4) >= (size_t)16 * LDP + (size_t)4 * a.Cout_pad * 16;
        if (fuse) { a.x1_out = x1_out; a.FT = rows_plan->FT_fwd; a.rows_H = rows_plan->H; a.m2c = rows_plan->m2c; }
        else rows_after = true;       // shapes the epilogue cannot host: separate rows kernel, same result
    }
    return DLWP_OK;
}

// fills and validates the arguments of the chained launch (second: with the second MLP; without it only c.p is filled, under the
// same conditions) and gives its LDS floats.  DLWP_E_UNSUPPORTED, error string untouched, where the shapes do not allow the chain.
int chain_make_args(ChainArgs& c, size_t& lds_floats, const dlwp_chan_src* x1v, const float* w11, const float* b11,
                    const float* w12, const float* b12, const dlwp_chan_dst* y1, const dlwp_chan_src* res1, int Cin1, int Ch1,
                    int Cout1, bool second, const dlwp_chan_src* x2v, const float* w21, const float* b21, const float* w22,
                    const float* b22, const dlwp_chan_dst* y2, int Cin2, int Ch2, int Cout2, const signed char* next_ch, int B,
                    int P, const dlwp_fno_plan* rows_plan, float2* x1_out) {
    c = ChainArgs{};
    bool ra1, ra2 = false;
    int rc = fwd_make_args(c.p, x1v, w11, b11, w12, b12, y1, res1, B, Cin1, Ch1, Cout1, P, nullptr, nullptr, ra1);
    if (rc) return rc;
    constexpr int HQ = FWD_WAVES / 4;
    lds_floats = fwd_lds_floats(c.p.Cin_pad, c.p.Ch_pad, c.p.Cout_pad) + (size_t)HQ * c.p.Cout_pad * LDP;
    for (int o = 0; o < 8; ++o) c.next_ch[o] = (signed char)-1;
    if (!c.p.vec_x || Cout1 > 8 || c.p.Cout_pad != 16) return DLWP_E_UNSUPPORTED;
    if (second) {
        if ((rc = fwd_make_args(c.l, x2v, w21, b21, w22, b22, y2, nullptr, B, Cin2, Ch2, Cout2, P, rows_plan, x1_out, ra2))) return rc;
        lds_floats += fwd_lds_floats(c.l.Cin_pad, c.l.Ch_pad, c.l.Cout_pad);
        const bool alias_ok = (size_t)HQ * c.l.Cout_pad * LDP <= (size_t)c.p.Ch_pad * (c.p.Cin_pad + 4);
        if (ra2 || !c.l.vec_x || !alias_ok || c.l.Cout_pad > 32) return DLWP_E_UNSUPPORTED;
        for (int o = 0; o < Cout1; ++o) {
            c.next_ch[o] = next_ch[o];
            if (c.next_ch[o] >= 0) {
                if (c.next_ch[o] >= Cin2) return DLWP_E_UNSUPPORTED;
                c.skip |= 1ull << c.next_ch[o];
            }
        }
    }
    if (sizeof(float) * lds_floats > (size_t)160 * 1024) return DLWP_E_UNSUPPORTED;
    return DLWP_OK;
}

}  // namespace
