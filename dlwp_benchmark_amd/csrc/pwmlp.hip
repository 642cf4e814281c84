// Pointwise two-layer channel MLP on channels-first fields (the FNO lifting / projection
// networks: 1x1 conv -> GELU -> 1x1 conv).  Reference call sites: neuralop.FNO.lifting /
// .projection constructed at src/nsbench/models/fno/fno.py:19-27,205-215 and
// src/dlwpbench/models/fno/fno.py:38-47 (third-party arithmetic).
//
// MI355X design: one workgroup = 64 consecutive pixels of one sample x all channels.
// Both GEMMs run on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32); the hidden activations
// (Ch x 64) never leave registers: the accumulator of GEMM1 (rows = hidden channel 4g+j,
// col = pixel) is directly the B operand of GEMM2 when the A operand (W2) is read with the
// matching permuted-k order (common.hip.h: mfma16_chunk).  Backward recomputes the hidden
// layer, keeps weight-gradient partials in registers over the 64 pixels and leaves them in a
// per-workgroup slab in accumulator-tile order (plain 16-byte stores; one slab-parallel launch
// folds every slab of a training step, fold_slabs_kernel below); without a slab they go out as
// hardware float atomics (API path).  The backward kernel's waves own their hidden blocks alone, so they read their weight
// fragments straight from L2 into registers (no LDS images; measured equal to the staged form, 22.1 / 20.6 us, and it frees
// 55 KB of LDS); the forward kernel's four pixel-block waves share every fragment, there the LDS images stay (the register
// form re-read each fragment four times through L1: 14.9 / 12.4 us against 11.4 / 10.1).  The forward kernel can append the W-axis DFT of its output
// rows (lifting -> first spectral block), the backward kernel the adjoint DFT of its input
// gradient rows (projection backward -> last spectral block's backward).
//
// The exact-f32 MFMA issues at the fp32 vector rate (32 cycles per 16x16x4 per SIMD) and does not overlap VALU work of the same
// SIMD, so the backward kernel's main loop costs its MFMA count; two products that multiply zeros or an identity are kept off
// the matrix pipe, both exactly (every output is bit for bit what the all-MFMA form gave):
//  - Cout == 1 (the projection of every scalar-field FNO, pwmlp_bwd_kernel<NIB, 0, 8>): g_a = W2^T gy has one real row of 16,
//    so g_a[p][h] = gy[p] * w2[h] is one VALU multiply, bit-identical to the zero-padded MFMA (one rounded product + zeros).
//  - every backward: gz^T -> gz goes through a wave-private 16 x 16 LDS tile (one 16-byte write, four 4-byte reads, row stride
//    20 floats: conflict-free both ways, no workgroup barrier) instead of a 4-MFMA product with the identity.
// 36 -> 28 MFMAs per 16 x 16 tile in the projection backward, 32 -> 28 in the lifting backward.  The other one-row products
// (dW2 in the backward, the second GEMM of the forward) stay on the MFMA: as VALU sums they were 0.8 - 1 us faster per launch
// but reorder fp32 additions, which moved the training step's parameters (profiles/r07_experiments.md).
// Step table of the headline (64 x 64, B 4): projection backward 22.4 -> 20.5 us, lifting backward 20.4 -> 19.3 us.
#include "common.hip.h"
#include "dlwpmi_internal.h"
#include "fno_rows.hip.h"
#include "pwmlp_bwd.hip.h"
#include "pwmlp_fwd.hip.h"

namespace {

template <int NOB, int NW>
__global__ __launch_bounds__(NW * 64) void pwmlp_fwd_kernel(FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FwdLds L = fwd_carve(smem, a, nullptr);
    const int b = blockIdx.x / a.tiles_per_sample, tile = blockIdx.x % a.tiles_per_sample;
    const int p0 = tile * PT;
    DLWP_STAMP(0);
    // issue every independent global load first, then fill the LDS images
    FwdLoads q;
    fwd_issue(a, q);
    DLWP_STAMP(1);
    stage_pixels(L.xs, a.x, b, a.Cin, a.Cin_pad, p0, a.P, a.vec_x != 0);
    DLWP_STAMP(2);
    fwd_commit(a, L, q);
    DLWP_STAMP(4);
    __syncthreads();
    DLWP_STAMP(5);
    fwd_compute<NOB, NW>(a, L);
    DLWP_STAMP(6);
    __syncthreads();
    DLWP_STAMP(7);
    fwd_finish<NOB, NW>(a, L, q.ftv, b, p0, tile);
    DLWP_STAMP(8);
}

// Projection of net call k chained with the lifting of net call k + 1 (both pointwise, the same 64-pixel tile): the rollout's
// closed loop feeds the frame the projection has just produced straight into the next lifting layer's input tile, in LDS;
// one launch, one prologue (both weight sets are requested together) instead of two, and the frame is not read back.
template <int NOB1, int NOB2, int NW>
__global__ __launch_bounds__(NW * 64) void pwmlp_fwd_chain_kernel(ChainArgs c) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int HQ = NW / 4;
    // first MLP with its partial tiles, then the second MLP whose partial tiles alias the first one's W1 image (dead by then)
    const FwdLds P = fwd_carve(smem, c.p, nullptr);
    float* base2 = P.outs + HQ * c.p.Cout_pad * LDP;
    const FwdLds Lq = fwd_carve(base2, c.l, P.w1s);
    const int b = blockIdx.x / c.p.tiles_per_sample, tile = blockIdx.x % c.p.tiles_per_sample;
    const int p0 = tile * PT;
    FwdLoads qp, ql;
    fwd_issue(c.p, qp);
    fwd_issue(c.l, ql);
    stage_pixels(P.xs, c.p.x, b, c.p.Cin, c.p.Cin_pad, p0, c.p.P, c.p.vec_x != 0);
    stage_pixels(Lq.xs, c.l.x, b, c.l.Cin, c.l.Cin_pad, p0, c.l.P, c.l.vec_x != 0, c.skip);
    fwd_commit(c.p, P, qp);
    fwd_commit(c.l, Lq, ql);
    __syncthreads();
    fwd_compute<NOB1, NW>(c.p, P);
    __syncthreads();
    fwd_finish<NOB1, NW>(c.p, P, qp.ftv, b, p0, tile, Lq.xs, c.next_ch);
    __syncthreads();
    fwd_compute<NOB2, NW>(c.l, Lq);
    __syncthreads();
    fwd_finish<NOB2, NW>(c.l, Lq, ql.ftv, b, p0, tile);
}


// NOB == 0 is the scalar-output form (Cout == 1): g_a^T[p][h] = gy[p] * w2[h] is one VALU multiply (bit-identical to the
// zero-padded MFMA: one rounded product plus exact zeros); everything else, dW2 included, is as for NOB == 1.  (It is an
// instantiation of this template and not a second kernel around a shared body: a body that takes the arguments by reference
// loads the whole argument block up front and spills scalar registers, +1.1 us on every instantiation.)
template <int NIB, int NOB, int NW>
__global__ __launch_bounds__(NW * 64) void pwmlp_bwd_kernel(BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // the body is text shared with fno_spatial_lift_bwd_kernel (fno_block.hip), which runs it behind a `spatial` phase
#include "pwmlp_bwd_body.inc.h"
}


// ---- one launch that folds EVERY partial slab of a training step into the gradient buffer.
// (The first version folded each slab set with its own launch, every thread walking the slab dimension serially: 256
// dependent-free but serial loads per thread, 12-17 us per launch, six launches per step.)  A workgroup owns 64 consecutive slab offsets (coalesced 256-byte rows) and its four
// waves each sum a quarter of the slabs, 16 loads in flight per lane, combined through LDS; the destination of an offset
// is found by inverting the slab layout (tile order of pwmlp_bwd, plain order of the skip-weight slabs).
constexpr int FOLD_MAX_JOBS = 8;
struct FoldJobDev {
    const float* slab;
    long long stride;           // floats between consecutive slabs
    int nslab, kind;            // kind 0: plain {d1[n1] | d2[n2]}; 1: pwmlp accumulator-tile layout
    int blk0, nblk;             // block range of this job inside the launch
    float *d1, *d2, *d3, *d4;   // kind 0: d1, d2;  kind 1: gw1, gb1, gw2, gb2
    int n1, n2;                 // kind 0 segment lengths
    int Cin, Ch, Cout, nob, nib, Ch_pad, Cout_pad;
};
struct FoldArgs {
    FoldJobDev j[FOLD_MAX_JOBS];
    int njobs;
};

__device__ __forceinline__ float* fold_dst(const FoldJobDev& J, long long off) {
    if (J.kind == 0) {
        if (off < J.n1) return J.d1 + off;
        if (off < (long long)J.n1 + J.n2) return J.d2 + (off - J.n1);
        return nullptr;
    }
    const long long o_t1 = (long long)(J.Ch_pad / 16) * J.nob * 256, o_gb1 = o_t1 + (long long)(J.Ch_pad / 16) * J.nib * 256;
    const long long o_gb2 = o_gb1 + J.Ch_pad;
    if (off < o_t1) {            // dW2 tile (hb, ob): lane = (o%16/4)*16 + h%16, register j = o%4
        const int j = (int)(off & 3), lane = (int)((off >> 2) & 63), t = (int)(off >> 8);
        const int hb = t / J.nob, ob = t - hb * J.nob;
        const int o = ob * 16 + (lane >> 4) * 4 + j, h = hb * 16 + (lane & 15);
        return (o < J.Cout && h < J.Ch) ? J.d3 + (long long)o * J.Ch + h : nullptr;
    }
    if (off < o_gb1) {           // dW1 tile (hb, ib): lane = (h%16/4)*16 + i%16, register j = h%4
        const long long e = off - o_t1;
        const int j = (int)(e & 3), lane = (int)((e >> 2) & 63), t = (int)(e >> 8);
        const int hb = t / J.nib, ib = t - hb * J.nib;
        const int h = hb * 16 + (lane >> 4) * 4 + j, i = ib * 16 + (lane & 15);
        return (h < J.Ch && i < J.Cin) ? J.d1 + (long long)h * J.Cin + i : nullptr;
    }
    if (off < o_gb2) {
        const int h = (int)(off - o_gb1);
        return h < J.Ch ? J.d2 + h : nullptr;
    }
    const int o = (int)(off - o_gb2);
    return o < J.Cout ? J.d4 + o : nullptr;
}

__global__ __launch_bounds__(256) void fold_slabs_kernel(FoldArgs a) {
    __shared__ float part[4][64];
    int ji = 0;
#pragma unroll
    for (int k = 1; k < FOLD_MAX_JOBS; ++k)
        if (k < a.njobs && (int)blockIdx.x >= a.j[k].blk0) ji = k;
    const FoldJobDev& J = a.j[ji];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long off = (long long)((int)blockIdx.x - J.blk0) * 64 + lane;
    float* dst = off < J.stride ? fold_dst(J, off) : nullptr;
    float acc = 0.f;
    if (dst) {
        const int per = (J.nslab + 3) / 4, s0 = w * per, s1 = min(J.nslab, s0 + per);
        const float* p = J.slab + off;
        int s = s0;
        for (; s + 16 <= s1; s += 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = p[(long long)(s + u) * J.stride];
#pragma unroll
            for (int u = 0; u < 16; ++u) acc += v[u];
        }
        for (; s < s1; ++s) acc += p[(long long)s * J.stride];
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && dst) *dst += (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

template <typename K>
int set_lds(K kernel, size_t bytes) {
    return dlwp_ensure_lds(reinterpret_cast<const void*>(kernel), bytes, "pwmlp");
}

}  // namespace

int dlwp_pwmlp_fwd_ex(const dlwp_chan_src* x, const float* w1, const float* b1, const float* w2,
                      const float* b2, const dlwp_chan_dst* y, const dlwp_chan_src* res, int B,
                      int Cin, int Ch, int Cout, int P, hipStream_t stream) {
    return dlwp_pwmlp_fwd_rows_ex(x, w1, b1, w2, b2, y, res, B, Cin, Ch, Cout, P, nullptr, nullptr, stream);
}

bool dlwp_pwmlp_rows_fusable(const dlwp_fno_plan* p, int Cout, int P) {
    return p && p->W == PT && p->NP == 16 && p->C == Cout && P == p->H * p->W && p->C_pad <= 64;
}

int dlwp_pwmlp_fwd_rows_ex(const dlwp_chan_src* x, const float* w1, const float* b1, const float* w2,
                           const float* b2, const dlwp_chan_dst* y, const dlwp_chan_src* res, int B,
                           int Cin, int Ch, int Cout, int P, const dlwp_fno_plan* rows_plan, float2* x1_out,
                           hipStream_t stream) {
    FwdArgs a;
    bool rows_after;
    int rc = fwd_make_args(a, x, w1, b1, w2, b2, y, res, B, Cin, Ch, Cout, P, rows_plan, x1_out, rows_after);
    if (rc) return rc;
    const int nob = a.Cout_pad / 16;
    const size_t lds = sizeof(float) * (fwd_lds_floats(a.Cin_pad, a.Ch_pad, a.Cout_pad) + (size_t)(FWD_WAVES / 4) * a.Cout_pad * LDP);
    constexpr int NW = FWD_WAVES;
    const dim3 grid(B * a.tiles_per_sample), block(NW * 64);
    const double pix = (double)B * P;
    dlwp_prof_scope prof(stream, 2.0 * pix * Ch * (Cin + Cout), 4.0 * pix * (Cin + Cout), "pwmlp_fwd_kernel<%d, %d>",
                         nob, NW);                        // the instantiation this call launches, as the live accounting reports it
#define LAUNCH(N)                                                             \
    if ((rc = set_lds(pwmlp_fwd_kernel<N, NW>, lds)) != DLWP_OK) return rc;   \
    hipLaunchKernelGGL((pwmlp_fwd_kernel<N, NW>), grid, block, lds, stream, a);
    switch (nob) {
        case 1: LAUNCH(1) break;
        case 2: LAUNCH(2) break;
        case 3: LAUNCH(3) break;
        default: LAUNCH(4) break;
    }
#undef LAUNCH
    DLWP_LAUNCH_CHECK();
    if (rows_after) return dlwp_fno_rows_dft(rows_plan, y->base, 0, 0, x1_out, B, stream);
    return DLWP_OK;
}

// Two forward MLPs on the same pixel tiles in ONE launch (projection of a net call -> lifting of the next one): the second
// MLP's input channels that ARE output channels of the first (matched by plane pointer and batch stride in the caller's
// channel table) are handed over in LDS.  Returns DLWP_E_UNSUPPORTED without touching the error string when the shapes do not
// allow the chain (the caller then issues the two launches separately).
int dlwp_pwmlp_fwd_chain_ex(const dlwp_chan_src* x1v, const float* w11, const float* b11, const float* w12, const float* b12,
                            const dlwp_chan_dst* y1, const dlwp_chan_src* res1, int Cin1, int Ch1, int Cout1,
                            const dlwp_chan_src* x2v, const float* w21, const float* b21, const float* w22, const float* b22,
                            const dlwp_chan_dst* y2, int Cin2, int Ch2, int Cout2, const signed char* next_ch, int B, int P,
                            const dlwp_fno_plan* rows_plan, float2* x1_out, hipStream_t stream) {
    ChainArgs c;
    size_t lds_floats;
    int rc = chain_make_args(c, lds_floats, x1v, w11, b11, w12, b12, y1, res1, Cin1, Ch1, Cout1, true, x2v, w21, b21, w22, b22, y2,
                             Cin2, Ch2, Cout2, next_ch, B, P, rows_plan, x1_out);
    if (rc) return rc;
    constexpr int NW = FWD_WAVES;
    const size_t lds = sizeof(float) * lds_floats;
    const int nob2 = c.l.Cout_pad / 16;
    const dim3 grid(B * c.p.tiles_per_sample), block(NW * 64);
    const double pix = (double)B * P;
    dlwp_prof_scope prof(stream, 2.0 * pix * (Ch1 * (Cin1 + Cout1) + Ch2 * (Cin2 + Cout2)), 4.0 * pix * (Cin1 + Cout1 + Cin2 + Cout2),
                         "pwmlp_fwd_chain_kernel<1, %d, %d>", nob2, NW);
    if (nob2 == 1) {
        if ((rc = set_lds(pwmlp_fwd_chain_kernel<1, 1, NW>, lds)) != DLWP_OK) return rc;
        hipLaunchKernelGGL((pwmlp_fwd_chain_kernel<1, 1, NW>), grid, block, lds, stream, c);
    } else {
        if ((rc = set_lds(pwmlp_fwd_chain_kernel<1, 2, NW>, lds)) != DLWP_OK) return rc;
        hipLaunchKernelGGL((pwmlp_fwd_chain_kernel<1, 2, NW>), grid, block, lds, stream, c);
    }
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

int dlwp_pwmlp_bwd_ex(const dlwp_chan_src* x, const float* w1, const float* b1, const float* w2,
                      const dlwp_chan_src* gy, const dlwp_chan_src* pred, const dlwp_chan_src* target,
                      float mse_scale, const dlwp_chan_dst* gx, int gx_accumulate, const dlwp_chan_dst* gres,
                      float* gw1, float* gb1, float* gw2, float* gb2, float* slab, int slab_accumulate, int B,
                      int Cin, int Ch, int Cout, int P, hipStream_t stream) {
    return dlwp_pwmlp_bwd_rows_ex(x, w1, b1, w2, gy, pred, target, mse_scale, gx, gx_accumulate, gres, gw1, gb1, gw2, gb2,
                                  slab, slab_accumulate, B, Cin, Ch, Cout, P, nullptr, nullptr, stream);
}

int dlwp_pwmlp_bwd_rows_ex(const dlwp_chan_src* x, const float* w1, const float* b1, const float* w2,
                           const dlwp_chan_src* gy, const dlwp_chan_src* pred, const dlwp_chan_src* target,
                           float mse_scale, const dlwp_chan_dst* gx, int gx_accumulate, const dlwp_chan_dst* gres,
                           float* gw1, float* gb1, float* gw2, float* gb2, float* slab, int slab_accumulate, int B,
                           int Cin, int Ch, int Cout, int P, const dlwp_fno_plan* rows_plan, float2* x1_out,
                           hipStream_t stream) {
    DLWP_REQUIRE(B > 0 && Cin > 0 && Ch > 0 && Cout > 0 && P > 0, DLWP_E_INVALID,
                 "pwmlp_bwd: non-positive dimension");
    BwdArgs a{};
    a.x = *x; a.w1 = w1; a.b1 = b1; a.w2 = w2;
    if (gy) a.gy = *gy;
    if (pred) { a.pred = *pred; a.target = *target; }
    a.mse_scale = mse_scale;
    if (gx) a.gx = *gx;
    a.gx_accumulate = gx_accumulate;
    if (gres) a.gres = *gres;
    a.gw1 = gw1; a.gb1 = gb1; a.gw2 = gw2; a.gb2 = gb2;
    a.B = B; a.Cin = Cin; a.Ch = Ch; a.Cout = Cout; a.P = P;
    a.tiles_per_sample = ceil_div(P, PT);
    a.Cin_pad = round_up(Cin, 16); a.Ch_pad = round_up(Ch, 16); a.Cout_pad = round_up(Cout, 16);
    a.slab = slab; a.slab_stride = dlwp_pwmlp_slab_stride(Cin, Ch, Cout); a.slab_accumulate = slab_accumulate;
    a.vec_w = aligned16(w1);
    a.dCin = make_fastdiv(Cin); a.dCh = make_fastdiv(Ch);
    a.vec_x = P % 4 == 0 && view_vec_ok(a.x) && view_vec_ok(a.gy);
    const int nib = a.Cin_pad / 16, nob = a.Cout_pad / 16;
    DLWP_REQUIRE(nib <= 4 && nob <= 4, DLWP_E_UNSUPPORTED,
                 "pwmlp_bwd: Cin<=64 and Cout<=64 supported (got %d, %d)", Cin, Cout);
    bool rows_after = false;
    if (x1_out) {
        DLWP_REQUIRE(rows_plan && gx && gx->base && !gx_accumulate, DLWP_E_INVALID,
                     "pwmlp_bwd: the rows DFT needs a plan and a dense, overwritten gx");
        const bool fuse = dlwp_pwmlp_rows_fusable(rows_plan, Cin, P) && a.vec_x && view_vec_ok(a.gx) &&
                          gx->bstride == (long long)Cin * P && gx->cstride == P &&
                          (size_t)BWD_WAVES * a.Cin_pad * LDP >= (size_t)4 * a.Cin_pad * 16 + (size_t)16 * LDP;
        if (fuse) { a.x1_out = x1_out; a.FT = rows_plan->FT_adj; a.rows_H = rows_plan->H; a.m2c = rows_plan->m2c; }
        else rows_after = true;       // shapes the epilogue cannot host: separate rows kernel, same result
    }
    const size_t red = (size_t)BWD_WAVES * a.Cin_pad * LDP;  // gx partial tiles (host the rows-DFT scratch afterwards)
    const size_t lds = sizeof(float) * ((size_t)a.Cin_pad * LDP + (size_t)a.Cout_pad * LDP + red);
    constexpr int NW = BWD_WAVES;
    const dim3 grid(B * a.tiles_per_sample), block(NW * 64);
    int rc;
    const bool scalar = Cout == 1;
    const double pix = (double)B * P;
    dlwp_prof_scope prof(stream, 2.0 * pix * Ch * (3 * Cin + 2 * Cout), 4.0 * pix * (2 * Cin + Cout), "pwmlp_bwd_kernel<%d, %d, %d>",
                         nib, scalar ? 0 : nob, NW);      // the instantiation this call launches, as the live accounting reports it
#define LAUNCH(I, O)                                                           \
    if ((rc = set_lds(pwmlp_bwd_kernel<I, O, NW>, lds)) != DLWP_OK) return rc; \
    hipLaunchKernelGGL((pwmlp_bwd_kernel<I, O, NW>), grid, block, lds, stream, a);
#define ROW(I)                       \
    switch (nob) {                   \
        case 1: LAUNCH(I, 1) break;  \
        case 2: LAUNCH(I, 2) break;  \
        case 3: LAUNCH(I, 3) break;  \
        default: LAUNCH(I, 4) break; \
    }
    if (scalar) {            // Cout == 1: the scalar-output instantiations (NOB = 0)
        switch (nib) {
            case 1: LAUNCH(1, 0) break;
            case 2: LAUNCH(2, 0) break;
            case 3: LAUNCH(3, 0) break;
            default: LAUNCH(4, 0) break;
        }
    } else switch (nib) {
        case 1: ROW(1) break;
        case 2: ROW(2) break;
        case 3: ROW(3) break;
        default: ROW(4) break;
    }
#undef ROW
#undef LAUNCH
    DLWP_LAUNCH_CHECK();
    if (rows_after) return dlwp_fno_rows_dft(rows_plan, gx->base, 0, 1, x1_out, B, stream);
    return DLWP_OK;
}

long long dlwp_pwmlp_slab_stride(int Cin, int Ch, int Cout) {
    const long long nhb = round_up(Ch, 16) / 16, nib = round_up(Cin, 16) / 16, nob = round_up(Cout, 16) / 16;
    return nhb * (nob + nib) * 256 + round_up(Ch, 16) + round_up(Cout, 16);
}

int dlwp_pwmlp_slab_count(int B, int P) { return B * ceil_div(P, PT); }

int dlwp_fold_slabs(const dlwp_fold_job* jobs, int njobs, hipStream_t stream) {
    DLWP_REQUIRE(jobs && njobs >= 1 && njobs <= FOLD_MAX_JOBS, DLWP_E_INVALID, "fold_slabs: 1..%d jobs", FOLD_MAX_JOBS);
    FoldArgs a{};
    a.njobs = njobs;
    int blocks = 0;
    for (int k = 0; k < njobs; ++k) {
        const dlwp_fold_job& q = jobs[k];
        FoldJobDev& J = a.j[k];
        DLWP_REQUIRE(q.slab && q.nslab > 0, DLWP_E_INVALID, "fold_slabs: job %d has no slab", k);
        J.slab = q.slab; J.nslab = q.nslab; J.kind = q.pwmlp ? 1 : 0;
        if (q.pwmlp) {
            J.stride = dlwp_pwmlp_slab_stride(q.Cin, q.Ch, q.Cout);
            J.Cin = q.Cin; J.Ch = q.Ch; J.Cout = q.Cout;
            J.nob = round_up(q.Cout, 16) / 16; J.nib = round_up(q.Cin, 16) / 16;
            J.Ch_pad = round_up(q.Ch, 16); J.Cout_pad = round_up(q.Cout, 16);
            J.d1 = q.d1; J.d2 = q.d2; J.d3 = q.d3; J.d4 = q.d4;
            DLWP_REQUIRE(q.d1 && q.d2 && q.d3 && q.d4, DLWP_E_INVALID, "fold_slabs: job %d needs gw1, gb1, gw2, gb2", k);
        } else {
            J.stride = q.stride; J.d1 = q.d1; J.d2 = q.d2; J.n1 = (int)q.n1; J.n2 = (int)q.n2;
            DLWP_REQUIRE(q.d1 && q.n1 + q.n2 <= q.stride, DLWP_E_INVALID, "fold_slabs: job %d segments exceed the stride", k);
        }
        J.blk0 = blocks;
        J.nblk = (int)((J.stride + 63) / 64);
        blocks += J.nblk;
    }
    hipLaunchKernelGGL(fold_slabs_kernel, dim3(blocks), dim3(256), 0, stream, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

int dlwp_pwmlp_slab_reduce(const float* slab, int nslab, int Cin, int Ch, int Cout, float* gw1, float* gb1,
                           float* gw2, float* gb2, hipStream_t stream) {
    dlwp_fold_job q{};
    q.slab = slab; q.nslab = nslab; q.pwmlp = 1; q.Cin = Cin; q.Ch = Ch; q.Cout = Cout;
    q.d1 = gw1; q.d2 = gb1; q.d3 = gw2; q.d4 = gb2;
    return dlwp_fold_slabs(&q, 1, stream);
}

#ifdef DLWP_STAMPS
extern "C" int dlwp_debug_stamps_pwmlp(unsigned long long* host_out) {
    DLWP_HIP(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_dlwp_stamps), sizeof(unsigned long long) * 32));
    return DLWP_OK;
}
#endif
