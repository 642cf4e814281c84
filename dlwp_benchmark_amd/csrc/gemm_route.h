// The token GEMM (token_ops.hip), host side: the ROUTE of a product -- the kernel family, its template parameters, the split-K plans,
// tile counts, grid and LDS bytes -- decided by dlwp_gemm_route for every entry (dlwp_gemm*, dlwp_gemm_batched*, dlwp_gemm_run, the
// members of dlwp_weight_grad_group).  Pure host arithmetic on the call, the two mode globals and the tuning knobs: standard headers
// only, no HIP call, nothing is dereferenced.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "tuning.h"

extern int g_gemm_bf16;       // dlwp_set_gemm_precision
extern int g_gemm_tile256;    // dlwp_set_gemm_tile256: 0 by shape (gemm_p8_applies), 1 wherever the kernel applies, -1 never

constexpr int BK = 32;         // K-step of gemm_kernel
constexpr int BKB = 32;        // K-step of the bf16-operand mode.  A 64-deep step (fewer barriers, twice the bytes in flight
                               // per workgroup) was measured: 136 instead of 104 registers drop the occupancy from 4 to 3
                               // waves per SIMD and the net effect is -13 % ... +10 % depending on the shape (8192x512x256:
                               // 14.1 -> 16.2 us, 8192x256x512: 15.1 -> 13.6 us), so the 32-deep step stays
// K-step of a bf16-operand kernel: 64 only for the 128 x 128 weight-gradient product of two bf16 arrays (both operands
// row-contiguous, K = tokens, split-K): 16200-deep 3072 x 768: 300 -> 410 TFLOP/s.  Everywhere else the doubled LDS image
// halves the workgroups per CU and loses (16200 x 3072 x 768 forward: 479 -> 392; profiles/r02_gemm_bench.txt).
constexpr int gemm_bf_kstep(int s16m, int T, bool akc, bool bkc) { return s16m == 3 && T == 2 && !akc && !bkc ? 64 : BKB; }
constexpr int GT = 128, GK = 64;      // gemm_glds_kernel / gemm_glds_tn_kernel: tile edge, deep K-step
constexpr int P8T = 256;              // gemm_p8_kernel / gemm_p8_tn_kernel: tile edge
constexpr int DT_A = 1, DT_B = 2, DT_C = 4, DT_R = 8;
constexpr int gr_ceil_div(int a, int b) { return (a + b - 1) / b; }
// dynamic LDS of gemm_kernel and the two group kernels: 4 operand images (two stages of A and B), bf16 [row][k + 8] / [k][row + 8] or
// fp32 [row][BK + 4] / [k][row + 4], whichever layout is larger
constexpr size_t gemm_generic_lds(bool bf, int T, int kstep) {
    return sizeof(float) * 4 * (bf ? std::max(64 * T * (kstep + 8), kstep * (64 * T + 8)) / 2 : std::max(64 * T * (BK + 4), BK * (64 * T + 4)));
}

enum GemmEntry { GEMM_PLAIN, GEMM_BATCHED, GEMM_RUN, GEMM_WGRAD_MEMBER };      // dlwp_gemm / _mixed / _rowscale, dlwp_gemm_batched*, dlwp_gemm_run,
                                                                               // a member of dlwp_weight_grad_group
struct GemmCall {
    int M, N, K, lda, ldb, ldc, transA, transB;
    long long nbatch, sA1, sA2, sB1, sB2, sC1, sC2, sR1, sR2, sBi1, sBi2;      // batches (nb1 * nb2) and their strides
    int dt;                                           // DT_* mask of the bf16 arrays
    uintptr_t A, B, C, bias, preact, residual;        // addresses: only their alignment is read, 0 = absent
    bool act, act_b, bias_row, rowsum, row_scale, accumulate;
    bool shared_out;                                  // dlwp_gemm_run: the batches add into one output
    GemmEntry entry;
    int per_product;                                  // GEMM_WGRAD_MEMBER: the member's share of the group's workgroup slots
    bool queue_open;                                  // a dlwp_gemm_group_begin queue is open on this thread
    int ncu;                                          // compute units (the persistent 256 x 256 kernels run one workgroup on each)
    bool no_slab_p8tn, no_slab_tn;                    // the launcher found no slab for that family's route: route again without it
};
enum GemmFamily {
    GEMM_PARKED,       // waits in the group queue for gemm_group_any_kernel<BF> (parameters as GEMM_GENERIC, VEC 3, T 1)
    GEMM_P8,           // gemm_p8_kernel<DIRECT, BKC, WIDE>
    GEMM_GLDS,         // gemm_glds_kernel<BKC, KD, GN>
    GEMM_GLDS_TN,      // gemm_glds_tn_kernel<KD> (+ gemm_slab_reduce_kernel)
    GEMM_P8_TN,        // gemm_p8_tn_kernel + gemm_slab_reduce_kernel
    GEMM_GENERIC,      // gemm_kernel<AKC, BKC, VEC, T, BF, S16M>; a GEMM_WGRAD_MEMBER runs it inside gemm_group_kernel
};
struct GemmSplit { int splits, kchunk, xcd_splitk; };
struct GemmRoute {
    GemmFamily family;
    bool akc, bkc, bf, direct, wide;
    int vec, T, s16m, kd, gn;
    int vec_ab;                  // bit 0 / 1: operand A / B allows 16-byte loads (vec is 0 on the 128 tile unless both do)
    GemmSplit caller;            // the split the entry prepares C for (zero: C must be zeroed first)
    bool zero, atomic_out;
    GemmSplit kernel;            // what the kernel runs with: the caller's, or the plan of a TN family
    int ntm, ntn;
    unsigned grid_x, grid_z, block;
    size_t lds;
    bool vec_epi, wide_epi;
    bool slab;                   // the K slices go to a slab (slab_bytes) whose `slices` planes gemm_slab_reduce_kernel adds in order
    int slices;
    size_t slab_bytes;
};

// Tile edge selection.  The 128 x 128 instantiation (T = 2) needs ~200 VGPRs and 74 KB of LDS, i.e. two waves per SIMD,
// and measured 5-7 % SLOWER than 64 x 64 (T = 1: ~104 VGPRs, four waves per SIMD hide the LDS fragment reads behind the
// other waves' MFMAs) on the SFNO (M = 512-32768, N = K = 256-512) and FourCastNet-scale (16200 x 3072 x 768) products,
// so it is only used when DLWP_GEMM_TILE=128 asks for it (kept for re-measurement with bf16 operands).
// With both operands stored as bf16 (16-byte loads, 4 staging registers per operand) the picture changes for deep products:
// profiles/r02_gemm_bench.txt, 16200 x 3072 x 768: 395 -> 479 TFLOP/s, 16200 x 768 x 3072 (gx): 438 -> 656; at K = 256-512
// (SFNO) the 128 tile still loses (264 -> 176), so it is taken from K = 768 on.
// can_split: no epilogue, so a long K may be cut into slices (weight gradients: few output tiles, K = tokens) -- the slices
// fill the chip where the tiles alone would not.
inline int gemm_tile_for(int M, int N, long long nbatch, int K, int dt, bool can_split) {
    const int tile_env = dlwp_tune("GEMM_TILE"), forced = tile_env == DLWP_TUNE_UNSET ? 0 : (tile_env == 128 ? 2 : 1);
    if (M < 128 || N < dlwp_tune_or("GEMM_TILE128_MINN", 128)) return 1;      // (knob: 96-wide outputs on the 128 tile, measurement)
    const long long tiles = (long long)gr_ceil_div(M, 128) * gr_ceil_div(N, 128) * nbatch;
    const bool fills = tiles * (can_split ? std::max(1, K / (4 * BK)) : 1) >= 224;
    if (forced) return forced == 2 && fills ? 2 : 1;
    return g_gemm_bf16 && (dt & 3) == 3 && K >= 768 && fills ? 2 : 1;
}

// a slice count that is a multiple of 8 lets a kernel keep the tiles of a K slice on one XCD (round 5): the nearest such count at or
// above `splits` (down to just over half of it) that survives the rounding of a slice to whole K-steps
inline bool gemm_xcd_kchunk(int K, int kstep, int splits, int* kchunk) {
    for (int s8 = gr_ceil_div(splits, 8) * 8; s8 >= 8 && s8 > splits / 2; s8 -= 8) {
        const int kc = gr_ceil_div(gr_ceil_div(K, s8), kstep) * kstep;
        if (gr_ceil_div(K, kc) % 8 == 0) { *kchunk = kc; return true; }
    }
    return false;
}
// the entries' split-K plan: reductions over a long K with few output tiles (weight gradients) are cut along K into whole K-steps until
// `budget` workgroups exist (512 for a lone product; the members of a weight-gradient group share one resident round) and combined
// with float atomics into a zeroed C
inline GemmSplit gemm_split_plan(long long tiles, int K, int budget, bool can_split, bool xcd) {
    GemmSplit p{1, 0, 0};
    if (can_split && tiles < 256 && K >= 8 * BK) p.splits = std::min(gr_ceil_div(budget, (int)tiles), K / (4 * BK));
    p.kchunk = gr_ceil_div(gr_ceil_div(K, p.splits), BK) * BK;
    p.splits = gr_ceil_div(K, p.kchunk);
    if (xcd && p.splits >= 8 && (dlwp_tune_or("GEMM_XCD_SPLITK", 1) & 1) != 0 && gemm_xcd_kchunk(K, BK, p.splits, &p.kchunk)) {
        p.splits = gr_ceil_div(K, p.kchunk);
        p.xcd_splitk = 1;
    }
    return p;
}

// bf16 arrays in memory (dlwp_gemm_mixed): whole groups of 8 along the contiguous dimension and 16-byte aligned -> the 16-byte path
// (bit 0 / 1: operand A / B); otherwise TileIO::load widens them element-wise (correct, slower)
inline int gemm_s16m(const GemmCall& c, bool akc, bool bkc, int kchunk) {
    auto ok16 = [&](uintptr_t p, int ld, bool kc, int rows, long long s1, long long s2) {
        return p % 16 == 0 && ld % 8 == 0 && (kc ? c.K % 8 == 0 && kchunk % 8 == 0 : rows % 8 == 0) && (c.nbatch == 1 || (s1 % 8 == 0 && s2 % 8 == 0));
    };
    return (((c.dt & DT_A) && ok16(c.A, c.lda, akc, c.M, c.sA1, c.sA2)) ? 1 : 0) | (((c.dt & DT_B) && ok16(c.B, c.ldb, bkc, c.N, c.sB1, c.sB2)) ? 2 : 0);
}

// column-tile width of gemm_glds_kernel: 96 when N is a multiple of 96 and rounds x width (whole rounds of one workgroup per CU, work per
// tile ~ its width) comes out lower than with 128-wide tiles; ties go to 128 when N is a multiple of 128.  GEMM_GLDS_N96: 0 never, 1 by
// this rule (default), 2 wherever N % 96 == 0.  GEMM_GLDS_N96_TIE_K: ties go to 96 up to this K (default 192).
inline int gemm_glds_tile_n(const GemmCall& c) {
    const int mode = dlwp_tune_or("GEMM_GLDS_N96", 1);
    if (mode == 0 || c.N % 96 != 0) return GT;
    if (mode == 2) return 96;
    const long long ncu = 256, mt = gr_ceil_div(c.M, GT);
    const long long c128 = (mt * gr_ceil_div(c.N, GT) + ncu - 1) / ncu * 128, c96 = (mt * (c.N / 96) + ncu - 1) / ncu * 96;
    // ties: 96 where 128 would pad, and for short products (K <= 192: launch / epilogue bound, the finer tiles fill the last round better --
    // Swin C4 443 -> 449 samples/s with every tie at 96, AFNO 721 53.6 -> 52.3 with its K = 768 products there too)
    return c96 < c128 || (c96 == c128 && (c.N % GT != 0 || c.K <= dlwp_tune_or("GEMM_GLDS_N96_TIE_K", 192))) ? 96 : GT;
}
// shapes the LDS-DMA kernel takes: both operands bf16 arrays with k contiguous and 16-byte aligned rows, K a multiple of 32, one
// plain product (no split-K / batches / row sums / row bias), the aligned epilogue, enough tiles to be worth 128 x 128
inline bool gemm_glds_applies(const GemmCall& c, const GemmRoute& r) {
    const bool off = dlwp_tune_on("GEMM_NOGLDS");
    if (off || !g_gemm_bf16 || !r.akc || (c.dt & (DT_A | DT_B)) != (DT_A | DT_B)) return false;
    if (c.K % 32 || c.lda % 8 || c.ldb % 8 || c.A % 16 || c.B % 16) return false;
    if (!r.bkc && c.N % 8) return false;
    if (r.caller.splits != 1 || c.nbatch != 1 || r.atomic_out || c.rowsum || c.bias_row || c.act_b || !r.vec_epi) return false;
    const bool force = dlwp_tune_on("GEMM_GLDS_FORCE");          // measurement: skip the shape heuristic below
    if (force) return c.M >= GT && c.N >= 64;
    // at least one workgroup per CU: below that the 64 x 64 kernel's shorter prologue wins (measured, profiles/r03_gemm_bench.txt: Pangu
    // 8192 x 192 x 768 104 vs 120 TFLOP/s, 2048 x 1536 x 384 77 vs 93; round 6, in the step: 128 tiles instead of 256 costs Pangu C4 1.3 %).
    // K: rounds 3 - 5 asked for four 64-deep K-steps; with >= 256 tiles the kernel wins from K = 96 on (three 32-deep steps) -- back to back
    // 32768 x 768 x 192 36.2 -> 26.1 us, 65536 x 384 x 96 28.8 -> 21.7 us (profiles/r06_gemm_vs_vendor.txt), in the step Swin C4 390.5 -> 396.5,
    // Pangu C4 107.0 -> 107.9 samples/s (profiles/r06_gemm_glds_threshold_sweep.txt)
    const int mink = dlwp_tune_or("GEMM_GLDS_MINK", 96), mintiles = dlwp_tune_or("GEMM_GLDS_MINTILES", 256);
    return c.K >= mink && (long long)gr_ceil_div(c.M, GT) * gr_ceil_div(c.N, gemm_glds_tile_n(c)) >= mintiles;
}
// the 256 x 256 kernel runs one workgroup per CU: nothing covers its prologue (two K-tiles of DMAs) and epilogue, so it needs a long K
// to pay -- 8192^3: 1351 against 1017 TFLOP/s, 4096^3 1186 / 983, 16200 x 768 x 3072: 898 / 788, but 16200 x 3072 x 768: 686 / 693 and every
// K <= 512 shape loses (profiles/r03_gemm_p8.txt): taken from K = 2048 with at least 128 tiles, or when forced
inline bool gemm_p8_applies(const GemmCall& c, const GemmRoute& r) {
    const bool env_on = dlwp_tune_on("GEMM_P8");
    if (g_gemm_tile256 < 0 || !r.akc || c.K % 64 || c.M < P8T || c.N < P8T) return false;
    const long long tiles = (long long)gr_ceil_div(c.M, P8T) * gr_ceil_div(c.N, P8T);
    const int mink = dlwp_tune_or("GEMM_P8_MINK", 2048);
    // one workgroup per CU: the last round should be at least 70 % full.  Round 5 asked for 80 % (16200 x 768 x 3072: 192 tiles = 75 % of one
    // round, where the 128 x 128 LDS-DMA kernel was then 0.4 % of the C5 step faster); with the 128-byte-row epilogue (round 6) this kernel
    // wins there: C5 720 x 1440 step 16.25 -> 16.08 ms, 721 x 1440 / Pangu / Swin unchanged (profiles/r06_gemm_p8_dispatch_sweep.txt)
    const long long rounds = (tiles + 255) / 256;
    const int fill_pct = dlwp_tune_or("GEMM_P8_FILL", 70);
    const bool fills = tiles >= 128 && 100 * tiles >= (long long)fill_pct * rounds * 256;
    return env_on || g_gemm_tile256 > 0 || (c.K >= mink && fills);
}
// weight-gradient products the TN kernels take: both operands bf16 arrays [k][row], fp32 output, no epilogue, one batch, the
// caller already prepared for split-K (zeroed or accumulating output)
inline bool gemm_glds_tn_applies(const GemmCall& c, const GemmRoute& r) {
    const bool off = dlwp_tune_on("GEMM_NOGLDS") || dlwp_tune_on("GEMM_NOGLDS_TN");
    if (off || !g_gemm_bf16 || (c.dt & (DT_A | DT_B | DT_C | DT_R)) != (DT_A | DT_B)) return false;
    if (c.M % 8 || c.N % 8 || c.lda % 8 || c.ldb % 8 || c.A % 16 || c.B % 16) return false;
    if (c.nbatch != 1 || r.atomic_out || c.bias || c.residual || c.preact || c.act || c.act_b || c.bias_row) return false;
    return c.M >= GT && c.N >= GT && c.K >= 1024 && r.caller.splits > 1;
}
// weight gradients on the 256 x 256 two-group kernel.  Measured (profiles/r03_gemm_p8.txt): 4096^3 707 against 656 TFLOP/s for the
// 128 x 128 sliced kernel, 8192^3 764 / 762, FourCastNet 3072 x 768 x 16200 639 / 689, 768 x 3072 x 16200 652 / 640 -- with every fragment
// through two transposing reads the K loop does not reach the y = x W^T kernel's rate and the gain is within the noise: NOT taken by
// shape, only when forced (dlwp_set_gemm_tile256(1) / DLWP_GEMM_P8: tests, measurements).  Needs the slab.
inline bool gemm_p8_tn_applies(const GemmCall& c) {
    if (c.no_slab_p8tn || dlwp_tune_on("GEMM_NOP8_TN") || g_gemm_tile256 < 0 || c.M < P8T || c.N < P8T || c.N % 4 || c.ldc % 4 || c.C % 16) return false;
    return dlwp_tune_on("GEMM_P8") || g_gemm_tile256 > 0;
}

// ---- the families' own plans: r arrives with the call-level part filled in (dlwp_gemm_route below)
inline GemmRoute gemm_route_glds(const GemmCall& c, GemmRoute r) {
    r.family = GEMM_GLDS;
    r.gn = gemm_glds_tile_n(c);
    r.ntn = gr_ceil_div(c.N, r.gn);
    r.ntm = gr_ceil_div(c.M, GT);
    const int kd_env = dlwp_tune("GEMM_GLDS_KD");
    // depth of a K-step (profiles/r03_gemm_glds_kd.txt): 32 deep leaves room for three or four workgroups per CU, which wins for
    // y = x W^T up to K ~ 1000 (16200 x 3072 x 768: 122 -> 110 us) and for gx = g W with at least four column tiles (16200 x 768 x 3072:
    // 122 -> 96 us, 8192^3: 841 -> 945 TFLOP/s); the deep, long products stay at 64 (8192^3 y: 1001 TFLOP/s against 828)
    const bool shallow = c.K % GK != 0 || (kd_env != DLWP_TUNE_UNSET ? kd_env == 32 : (r.bkc ? c.K <= 1024 : c.N >= 512));
    r.kd = shallow ? 32 : 64;
    // 64 KB at KD = 64 (the epilogue's 64 x 132 fp32 half tile fits inside); 33 KB (that half tile) at KD = 32
    r.lds = shallow ? sizeof(float) * 64 * (GT + 4) : (size_t)2 * 2 * GT * GK * 2;
    r.grid_x = r.ntn * r.ntm;
    return r;
}
inline GemmRoute gemm_route_p8(const GemmCall& c, GemmRoute r) {
    r.family = GEMM_P8;
    r.ntn = gr_ceil_div(c.N, P8T);
    r.ntm = gr_ceil_div(c.M, P8T);
    r.lds = (size_t)2 * 4 * 128 * 64 * 2;      // 128 KB: two stages of four half-tile images (the epilogue's 64 x 260 fp32 tile fits inside)
    r.direct = !dlwp_tune_on("GEMM_P8_STAGED");
    // 128-byte-row register epilogue (round 6): every tensor the epilogue touches in whole, aligned 8-column pieces
    auto al = [](uintptr_t p, bool bf) { return p % (bf ? 16 : 32) == 0; };
    r.wide_epi = dlwp_tune_or("GEMM_P8_WIDE", 1) != 0 && c.N % 8 == 0 && c.ldc % 8 == 0 && al(c.C, c.dt & DT_C) && al(c.preact, c.dt & DT_C) &&
                 al(c.residual, c.dt & DT_R) && (!c.bias || c.bias_row || c.bias % 16 == 0);
    r.wide = r.direct && r.wide_epi;
    r.grid_x = std::min(r.ntn * r.ntm, c.ncu);
    r.block = 512;
    return r;
}
inline GemmRoute gemm_route_p8_tn(const GemmCall& c, GemmRoute r) {
    r.family = GEMM_P8_TN;
    r.ntn = gr_ceil_div(c.N, P8T);
    r.ntm = gr_ceil_div(c.M, P8T);
    const int tiles8 = r.ntn * r.ntm, splits = std::max(1, std::min(c.ncu / tiles8, c.K / (16 * 64)));
    r.kernel.kchunk = gr_ceil_div(gr_ceil_div(c.K, splits), 64) * 64;
    r.kernel.splits = gr_ceil_div(c.K, r.kernel.kchunk);
    r.slab = true;
    r.slices = r.kernel.splits;
    r.slab_bytes = sizeof(float) * r.slices * (size_t)c.M * c.N;
    r.lds = (size_t)2 * 4 * 128 * 64 * 2;
    r.grid_x = std::min(tiles8 * r.kernel.splits, c.ncu);
    r.block = 512;
    return r;
}
inline GemmRoute gemm_route_glds_tn(const GemmCall& c, GemmRoute r) {
    r.family = GEMM_GLDS_TN;
    r.ntn = gr_ceil_div(c.N, GT);
    r.ntm = gr_ceil_div(c.M, GT);
    const int tilesg = r.ntn * r.ntm;
    // K-step depth and slices from the sweep in profiles/r03_gemm_glds_tn.txt: the grid should fill the resident slots once (a second,
    // partial round costs as much as a full one): 64 deep = 64 KB of LDS, two workgroups per CU; 32 deep = 32 KB and 160 VGPRs, three
    // per CU, which pays once there are enough output tiles (FourCastNet's 3072 x 768: 120 us against 133)
    const int kd_env = dlwp_tune("GEMM_GLDS_TN_KD");
    const bool shallow = kd_env != DLWP_TUNE_UNSET ? kd_env == 32 : tilesg >= 96;
    r.kd = shallow ? 32 : 64;
    const int slots = dlwp_tune_or("GEMM_GLDS_TN_WGS", shallow ? 768 : 448);
    // at least eight K-steps per slice: shorter slices only add partial tiles to combine (8192 tokens x 512 x 256, graph timing,
    // tools/bench_gemm_graph.py: 32 slices 22.6 us, 16 slices 17.4 us)
    const int splits = std::max(1, std::min(slots / tilesg, c.K / (8 * r.kd)));
    r.kernel.kchunk = gr_ceil_div(gr_ceil_div(c.K, splits), r.kd) * r.kd;
    // few tiles, many slices: a slice count that is a multiple of 8 keeps the tiles of a slice on one XCD (round 5)
    r.kernel.xcd_splitk = splits >= 8 && tilesg < 64 && (dlwp_tune_or("GEMM_XCD_SPLITK", 1) & 2) != 0 && gemm_xcd_kchunk(c.K, r.kd, splits, &r.kernel.kchunk);
    r.grid_z = gr_ceil_div(c.K, r.kernel.kchunk);
    r.kernel.splits = std::max(2, (int)r.grid_z);      // > 1: the atomic epilogue (the caller zeroed C for its own split)
    r.lds = (size_t)2 * 2 * GT * r.kd * 2;
    r.grid_x = tilesg;
    // few output tiles cut into many slices (SFNO's 512 x 256: 8 tiles x 32) read more slab in the reduction than the atomics cost
    r.slab = !(c.no_slab_tn || dlwp_tune_on("GEMM_TN_ATOMIC") || tilesg < dlwp_tune_or("GEMM_TN_SLAB_MIN", 24) || c.N % 4 || c.ldc % 4 || c.C % 16);
    r.slices = (int)r.grid_z;
    r.slab_bytes = sizeof(float) * r.slices * (size_t)c.M * c.N;
    return r;
}

inline GemmRoute dlwp_gemm_route(const GemmCall& c) {
    GemmRoute r{};
    r.akc = !c.transA;      // A is k-contiguous when not transposed ([M][K]); B is k-contiguous when transposed ([N][K])
    r.bkc = c.transB != 0;
    r.bf = g_gemm_bf16 != 0;
    const bool epilogue = c.bias || c.act || c.preact || c.residual || c.row_scale || (c.dt & DT_C);      // a bf16 output takes no split-K atomics
    const bool by_shape = c.entry == GEMM_PLAIN || c.entry == GEMM_BATCHED;      // the other entries stay on the 64 x 64 tile
    r.T = by_shape ? gemm_tile_for(c.M, c.N, c.nbatch, c.K, c.dt, !epilogue) : 1;
    const long long tiles = (long long)gr_ceil_div(c.N, 64 * r.T) * gr_ceil_div(c.M, 64 * r.T) * c.nbatch;
    r.caller = gemm_split_plan(tiles, c.K, c.entry == GEMM_WGRAD_MEMBER ? c.per_product : 512, !epilogue, c.entry == GEMM_PLAIN);
    r.kernel = r.caller;
    r.atomic_out = c.shared_out;
    r.zero = (r.caller.splits > 1 || c.shared_out) && !c.accumulate;
    // 16-byte loads need every row start and every group of four along the contiguous dimension to be aligned and whole;
    // decided per operand (a weight matrix with an odd row length must not force scalar loads on the activations)
    bool vecA = c.A % ((c.dt & DT_A) ? 8 : 16) == 0 && c.lda % 4 == 0 && (c.transA ? c.M % 4 == 0 : c.K % 4 == 0);
    bool vecB = c.B % ((c.dt & DT_B) ? 8 : 16) == 0 && c.ldb % 4 == 0 && (c.transB ? c.K % 4 == 0 : c.N % 4 == 0);
    if (c.nbatch > 1) {
        vecA = vecA && c.sA1 % 4 == 0 && c.sA2 % 4 == 0;
        vecB = vecB && c.sB1 % 4 == 0 && c.sB2 % 4 == 0;
    }
    r.vec = r.vec_ab = (vecA ? 1 : 0) | (vecB ? 2 : 0);
    // the epilogue through an LDS tile with 16-byte global accesses
    r.vec_epi = r.caller.splits == 1 && !r.atomic_out && c.N % 4 == 0 && c.ldc % 4 == 0 && c.C % 16 == 0 && (!c.bias || c.bias_row || c.bias % 16 == 0) &&
                c.residual % 16 == 0 && c.preact % 16 == 0;
    if (c.nbatch > 1)
        r.vec_epi = r.vec_epi && c.sC1 % 4 == 0 && c.sC2 % 4 == 0 && c.sR1 % 4 == 0 && c.sR2 % 4 == 0 && (c.bias_row || (c.sBi1 % 4 == 0 && c.sBi2 % 4 == 0));
    r.block = 256;
    r.grid_z = 1;
    const bool lone = c.entry != GEMM_WGRAD_MEMBER;      // a group member stays on the generic kernel's body
    // the queue: small, latency-bound products of the generic 64 x 64 configuration only: at most 2.2 GFLOP (the SFNO block-tail
    // products are 2.1; Pangu's 8192 x 384 x 1152 input gradient at 7.2 GFLOP belongs on its own kernel: parked, the C4 step went
    // from 14.3 to 15.1 ms)
    if (lone && c.queue_open && r.vec == 3 && r.T == 1 && !c.act_b && 2.0 * c.M * c.N * (double)c.K * c.nbatch <= 2.2e9 && c.K <= 16384) {
        r.family = GEMM_PARKED;
    } else if (lone && gemm_glds_applies(c, r)) {
        return gemm_p8_applies(c, r) ? gemm_route_p8(c, r) : gemm_route_glds(c, r);
    } else if (lone && !r.akc && !r.bkc && gemm_glds_tn_applies(c, r)) {
        return gemm_p8_tn_applies(c) ? gemm_route_p8_tn(c, r) : gemm_route_glds_tn(c, r);
    } else {
        r.family = GEMM_GENERIC;
        if (r.T == 2 && r.vec != 3) r.vec = 0;      // the 128-wide tile exists for fully aligned operands only
    }
    r.ntn = gr_ceil_div(c.N, 64 * r.T);
    r.ntm = gr_ceil_div(c.M, 64 * r.T);
    if (r.bf && r.vec == 3 && (c.dt & (DT_A | DT_B)) && !c.act_b) r.s16m = gemm_s16m(c, r.akc, r.bkc, r.caller.kchunk);
    r.lds = gemm_generic_lds(r.bf, r.T, gemm_bf_kstep(r.s16m, r.T, r.akc, r.bkc));
    r.grid_x = r.ntn * r.ntm;
    r.grid_z = (unsigned)(c.nbatch * r.caller.splits);
    return r;
}
