// Long-rollout diagnostics of the weather benchmark in one read of outputs and targets, and the monthly climatology.
//
// Reference: the second half of compute_metrics (src/dlwpbench/scripts/evaluate.py:548-588: RMSE of zonally and temporally averaged
// fields globally and on latitude bands, RMSE of the month 11-12 time-mean fields) beside its first half (:514-546, per-lead RMSE and
// ACC), and scripts/build_baselines.py:23-67 (persistence and climatology forecasts; the monthly climatology :52-62).  The reference
// de-normalises outputs and targets on the host, writes them to NetCDF and reduces them with xarray; its climatology forecast is a
// [sample, time] loop that copies one of twelve monthly maps per frame.  Here every quantity is a sum over ONE read of the chunk:
//   moments [Bc][T][V][5]   the five sums of dlwp_error_moments per sample, lead time and variable, in physical units
//   zonal   [2][Bc][T][V][H] the longitude mean of the de-normalised output (0) and target (1)
//   wsum    [2][Bc][V][H][W] the running sum of the NORMALISED output / target over the frames inside the window [w0, w1)
// De-normalisation is x * scale[v] + shift[v].  All sums are taken of the normalised values (a z500 offset of 5e4 never sits inside
// an fp32 accumulation or difference): the climatology is brought into normalised units per pixel, c_n = (c - shift) * (1 / scale),
// the moments are multiplied by scale^2 (|scale| for the absolute error) after summing, the zonal mean is sum / W * scale + shift,
// and wsum stays normalised (the caller applies scale to the difference of the two window means, where the shift cancels).
//
// Decomposition.  A workgroup of four waves owns (sample b, variable v, a block of 4 RPW latitude rows) and walks the chunk's frames
// in order; a wave owns RPW whole rows, lane l the columns l, l + 64, ... (CP of them), so a row sum is CP in-lane additions and one
// xor butterfly of the wave, and lat-lon planes need no workgroup barrier.  RPW and CP depend on W and the mesh only (lat-lon 1 x 1 up
// to 64 columns, HPX 2 x 1; then 1 x 2, 1 x 4, 1 x 8) -- never on the batch, the chunk or the device -- so the summation order below is the same for every chunking.
// More parallelism for small batches comes from the row blocks (grid.x), not from splitting time: the window sum of a pixel stays in
// one register from the first frame to the last.  A wave alone on its SIMD (batch 8: one workgroup per CU) hides nothing by itself,
// so (a) lat-lon frames are loaded in register groups of PF frames (outputs, targets and the frame's climatology map), two groups
// alternating: while one is reduced the other's loads are in flight; (b) the reduction of a frame is branch-free (a lane without a
// point carries zeros, a frame outside the window adds +0) and its 2 RPW + 5 butterflies run side by side, six rounds of
// ds_bpermute per frame instead of one dependent chain per value.
// HPX planes ([12][n][n], scored on lat-lon through the 4-tap hpx2ll table): the workgroup copies the output and target planes of a
// GROUP of up to 8 frames to LDS (16-byte pieces, four loads issued before their four LDS stores, so the group's loads are in flight
// together), then every lane gathers its taps there frame by frame, as hpx_error_moments_kernel<STAGED>; the taps of a lane's
// RPW x CP points stay in registers over the frames and the climatology of the next frame is loaded before the current one is
// reduced.  Every row block stages the whole plane again (HPX8: four row blocks; the re-reads are served by L2).  Planes of which
// not even one frame fits LDS_BUDGET are gathered from global memory by the same code (the direct path; the knob DIAG_PATH forces
// one).  No lat-lon tensor is written.
//
// Summation order (fixed; no atomics; every output address has one writer, so two runs give the same bits):
//   row sum      : per lane the columns l + 64 j in ascending j, then the xor butterfly 32, 16, 8, 4, 2, 1 over the wave
//   moments      : per lane the wave's rows in ascending order (columns as above, row weight applied per term), the butterfly, one
//                  partial per wave in the workspace; moments_fold_kernel adds the partials in ascending row order and scales
//   window sum   : wsum = wsum + x_frame in ascending frame order, starting from the value in memory -- a rollout scored in time
//                  chunks (and in batch chunks: samples are independent) gives the bits of one call
//
// group_mean (the monthly climatology: frames [N][P], group [N] -> mean [G][P], count [G]): a thread owns a pixel and walks the N
// frames in order, adding each to its own column of a [G][256] LDS table (no barrier: nobody else touches the column); an empty
// group gives count 0 and a zero row.
#include "common.hip.h"
#include "dlwpmi_internal.h"
#include "diag_stage.hip.h"      // tap4, stage_group (shared with csrc/spectra.hip)
#include <algorithm>

namespace {

constexpr int LDS_BUDGET = 72 * 1024;      // bytes of LDS the staged path may use (both planes of a frame group), as csrc/hpx_remap.hip
constexpr int MAX_CP = 8;                  // columns per lane: W <= 512
constexpr int GM_MAX_GROUPS = 64;          // group_mean: [G][256] floats of LDS

enum { MODE_LL = 0, MODE_HPX_LDS = 1, MODE_HPX_DIRECT = 2 };

struct DiagArgs {
    const float *out, *target, *scale, *shift, *roww, *clim;
    const int* month;
    const int* idx;
    const float* w;
    long long bs, ts;          // element strides of `out` along batch and time
    int M, npix, Bc, Tc, V, H, W, t_begin, T, w0, w1, vec, nslot, pf;
    float *part, *zonal, *wsum;
};

template <int RPW, int CP, int MODE>
__global__ __launch_bounds__(256) void rollout_diag_kernel(const DiagArgs a) {
    extern __shared__ __align__(16) float lds[];             // MODE_HPX_LDS: [pf][2][npix], the out and target planes of a frame group
    constexpr bool HPX = MODE != MODE_LL;
    constexpr int PF = RPW * CP <= 2 ? 4 : 2;                          // lat-lon: frames per register group, their loads in flight together
    const int v = blockIdx.y, b = blockIdx.z, lane = lane_id();
    const int slot = blockIdx.x * 4 + wave_id(), row0 = slot * RPW, hw = a.H * a.W;
    const float sc = a.scale ? a.scale[v] : 1.f, sh = a.shift ? a.shift[v] : 0.f, inv = 1.f / sc;
    const bool has_out = a.out != nullptr, has_clim = a.clim != nullptr;
    const bool any_win = a.t_begin < a.w1 && a.t_begin + a.Tc > a.w0;

    int pix[RPW][CP];
    float wr[RPW], so_w[RPW][CP], st_w[RPW][CP];
    int4 i4[HPX ? RPW : 1][HPX ? CP : 1];
    float4 w4[HPX ? RPW : 1][HPX ? CP : 1];
    float* ws_o = a.wsum + ((long long)b * a.V + v) * hw;
    float* ws_t = ws_o + (long long)a.Bc * a.V * hw;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int r = row0 + i;
        wr[i] = r < a.H ? (a.roww ? a.roww[r] : 1.f) : 0.f;
#pragma unroll
        for (int j = 0; j < CP; ++j) {
            const int c = lane + 64 * j;
            pix[i][j] = r < a.H && c < a.W ? r * a.W + c : -1;      // -1: no point (a row past H, a column past W)
            so_w[i][j] = any_win && pix[i][j] >= 0 ? ws_o[pix[i][j]] : 0.f;
            st_w[i][j] = any_win && pix[i][j] >= 0 ? ws_t[pix[i][j]] : 0.f;
            if constexpr (HPX) {
                i4[i][j] = pix[i][j] >= 0 ? reinterpret_cast<const int4*>(a.idx)[pix[i][j]] : make_int4(0, 0, 0, 0);
                w4[i][j] = pix[i][j] >= 0 ? reinterpret_cast<const float4*>(a.w)[pix[i][j]] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    const float* ob = has_out ? a.out + b * a.bs + (long long)v * a.npix : nullptr;
    const float* tb = a.target + ((long long)b * a.Tc * a.V + v) * a.npix;
    const long long tts = (long long)a.V * a.npix;
    const int* mrow = has_clim ? a.month + (long long)b * a.Tc : nullptr;

    // the climatology maps (physical units) of frame tc at this lane's points; zeros without a climatology or past the chunk
    auto load_clim = [&](int tc, float(&c)[RPW][CP]) {
        const float* cp = nullptr;
        if (has_clim && tc < a.Tc) {
            const int m = min(max(mrow[tc], 0), a.M - 1);          // (0 <= month < M is the caller's precondition; never an address outside clim)
            cp = a.clim + ((long long)m * a.V + v) * hw;
        }
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
            for (int j = 0; j < CP; ++j) c[i][j] = cp && pix[i][j] >= 0 ? cp[pix[i][j]] : 0.f;
    };
    struct Group {
        float o[PF][RPW][CP], t[PF][RPW][CP], c[PF][RPW][CP];
    };
    // lat-lon: outputs, targets and climatology of the frames t0 .. t0 + PF - 1 at this lane's points
    auto load_group = [&](int t0, Group& g) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int tc = t0 + k;
            const bool live = tc < a.Tc;
            load_clim(tc, g.c[k]);
            const float* op = has_out && live ? ob + tc * a.ts : nullptr;
            const float* tp = live ? tb + tc * tts : nullptr;
#pragma unroll
            for (int i = 0; i < RPW; ++i)
#pragma unroll
                for (int j = 0; j < CP; ++j) {
                    const bool ok = pix[i][j] >= 0;
                    g.o[k][i][j] = op && ok ? op[pix[i][j]] : 0.f;
                    g.t[k][i][j] = tp && ok ? tp[pix[i][j]] : 0.f;
                }
        }
    };
    // one frame: o / t the normalised values at this lane's points (o unused when the forecast is the climatology), c the climatology
    auto frame = [&](int tc, const float(&o_)[RPW][CP], const float(&t_)[RPW][CP], const float(&c_)[RPW][CP]) {
        const int g = a.t_begin + tc;
        const bool inwin = g >= a.w0 && g < a.w1;
        // branch-free: a lane without a point carries zeros (o_, t_, c_ are 0 there), a frame outside the window adds +0, and without
        // a climatology c_n = 0 and the three anomaly sums are dropped at the write -- so the NR reductions below run side by side
        constexpr int NR = 2 * RPW + 5;
        float red[NR];
#pragma unroll
        for (int q = 0; q < NR; ++q) red[q] = 0.f;
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
#pragma unroll
            for (int j = 0; j < CP; ++j) {
                const float cn = has_clim && pix[i][j] >= 0 ? (c_[i][j] - sh) * inv : 0.f;
                const float t = t_[i][j], o = has_out ? o_[i][j] : cn, d = o - t, oc = o - cn, tc_ = t - cn;
                red[2 * RPW + 0] += wr[i] * d * d;
                red[2 * RPW + 1] += wr[i] * fabsf(d);
                red[2 * RPW + 2] += wr[i] * oc * tc_;
                red[2 * RPW + 3] += wr[i] * oc * oc;
                red[2 * RPW + 4] += wr[i] * tc_ * tc_;
                red[2 * i] += o;
                red[2 * i + 1] += t;
                so_w[i][j] += inwin ? o : 0.f;
                st_w[i][j] += inwin ? t : 0.f;
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {                   // the xor butterfly 32, 16, ..., 1 on all NR values at once
            float other[NR];
#pragma unroll
            for (int q = 0; q < NR; ++q) other[q] = __shfl_xor(red[q], s);
#pragma unroll
            for (int q = 0; q < NR; ++q) red[q] += other[q];
        }
        float zo[RPW], zt[RPW];
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            zo[i] = fmaf(red[2 * i] / (float)a.W, sc, sh);
            zt[i] = fmaf(red[2 * i + 1] / (float)a.W, sc, sh);
        }
        const float a0 = red[2 * RPW], a1 = red[2 * RPW + 1], a2 = has_clim ? red[2 * RPW + 2] : 0.f,
                    a3 = has_clim ? red[2 * RPW + 3] : 0.f, a4 = has_clim ? red[2 * RPW + 4] : 0.f;
        if (lane < RPW && row0 + lane < a.H) {               // zonal [2][Bc][T][V][H]: lane i writes row row0 + i
            float yo = zo[0], yt = zt[0];
#pragma unroll
            for (int i = 1; i < RPW; ++i)
                if (lane == i) {
                    yo = zo[i];
                    yt = zt[i];
                }
            const long long z = (((long long)b * a.T + g) * a.V + v) * a.H + row0 + lane;
            a.zonal[z] = yo;
            a.zonal[z + (long long)a.Bc * a.T * a.V * a.H] = yt;
        }
        if (lane < 5) {                                      // part [Bc][Tc][V][nslot][5]
            const float m = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : lane == 3 ? a3 : a4;
            a.part[((((long long)b * a.Tc + tc) * a.V + v) * a.nslot + slot) * 5 + lane] = m;
        }
    };

    if constexpr (!HPX) {
        // two register groups: while one is reduced the loads of the other are in flight
        Group A, B;
        auto reduce = [&](int t0, const Group& g) {
#pragma unroll
            for (int k = 0; k < PF; ++k)
                if (t0 + k < a.Tc) frame(t0 + k, g.o[k], g.t[k], g.c[k]);
        };
        load_group(0, A);
        for (int t0 = 0; t0 < a.Tc; t0 += 2 * PF) {
            load_group(t0 + PF, B);
            reduce(t0, A);
            load_group(t0 + 2 * PF, A);
            reduce(t0 + PF, B);
        }
    } else {
        // a group of pf frames is staged at once (their loads in flight together); the climatology of the next frame is loaded
        // before the current one is reduced
        const int pf = MODE == MODE_HPX_LDS ? a.pf : 1;
        float cnext[RPW][CP];
        load_clim(0, cnext);
        for (int t0 = 0; t0 < a.Tc; t0 += pf) {
            const int nf = min(pf, a.Tc - t0);
            if constexpr (MODE == MODE_HPX_LDS) {
                stage_group(lds, has_out ? ob + t0 * a.ts : nullptr, a.ts, tb + t0 * tts, tts, nf, a.npix, a.vec);
                __syncthreads();
            }
#pragma unroll 1
            for (int k = 0; k < nf; ++k) {
                const int tc = t0 + k;
                float c_[RPW][CP], o_[RPW][CP], t_[RPW][CP];
#pragma unroll
                for (int i = 0; i < RPW; ++i)
#pragma unroll
                    for (int j = 0; j < CP; ++j) c_[i][j] = cnext[i][j];
                load_clim(tc + 1, cnext);
                const float* so = MODE == MODE_HPX_LDS ? lds + 2 * k * a.npix : (has_out ? ob + tc * a.ts : nullptr);
                const float* st = MODE == MODE_HPX_LDS ? lds + (2 * k + 1) * a.npix : tb + tc * tts;
#pragma unroll
                for (int i = 0; i < RPW; ++i)
#pragma unroll
                    for (int j = 0; j < CP; ++j) {
                        const bool ok = pix[i][j] >= 0;
                        t_[i][j] = ok ? tap4(st, i4[i][j], w4[i][j]) : 0.f;
                        o_[i][j] = ok && has_out ? tap4(so, i4[i][j], w4[i][j]) : 0.f;
                    }
                frame(tc, o_, t_, c_);
            }
            if constexpr (MODE == MODE_HPX_LDS) __syncthreads();   // the next group's copy overwrites the planes
        }
    }
    if (any_win) {
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
            for (int j = 0; j < CP; ++j)
                if (pix[i][j] >= 0) {
                    ws_o[pix[i][j]] = so_w[i][j];
                    ws_t[pix[i][j]] = st_w[i][j];
                }
    }
}

// moments [Bc][T][V][5] <- the per-wave partials in ascending slot (= row) order, times scale^2 (|scale| for the absolute error)
__global__ __launch_bounds__(256) void moments_fold_kernel(const float* __restrict__ part, const float* __restrict__ scale, float* m,
                                                           long long n, int Tc, int V, int nslot, int t_begin, int T) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;      // e = ((b Tc + tc) V + v) 5 + k
    if (e >= n) return;
    const int k = (int)(e % 5);
    const long long q = e / 5;
    const int v = (int)(q % V);
    const long long bt = q / V;
    const int tc = (int)(bt % Tc);
    const long long b = bt / Tc;
    float s = 0.f;
    for (int i = 0; i < nslot; ++i) s += part[(q * nslot + i) * 5 + k];
    const float sc = scale ? scale[v] : 1.f;
    m[((b * T + t_begin + tc) * V + v) * 5 + k] = s * (k == 1 ? fabsf(sc) : sc * sc);
}

__global__ __launch_bounds__(256) void group_mean_kernel(const float* __restrict__ frames, const int* __restrict__ group, float* mean,
                                                         int* count, long long N, long long P, int G) {
    extern __shared__ __align__(16) float lds[];             // [G][256] sums, then [G] counts (thread 0's)
    int* cnt = reinterpret_cast<int*>(lds + G * 256);
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    for (int g = 0; g < G; ++g) lds[g * 256 + threadIdx.x] = 0.f;
    if (threadIdx.x == 0)
        for (int g = 0; g < G; ++g) cnt[g] = 0;
    const bool act = p < P;
#pragma unroll 4
    for (long long n = 0; n < N; ++n) {
        const int g = group[n];
        const float x = act ? frames[n * P + p] : 0.f;
        if ((unsigned)g < (unsigned)G) {                     // (0 <= group < G is the caller's precondition; never an LDS address outside the table)
            lds[g * 256 + threadIdx.x] += x;
            if (threadIdx.x == 0) ++cnt[g];
        }
    }
    __syncthreads();                                         // cnt is thread 0's; every thread reads it
    for (int g = 0; g < G; ++g) {
        const int c = cnt[g];
        if (act) mean[g * P + p] = c ? lds[g * 256 + threadIdx.x] / (float)c : 0.f;
        if (blockIdx.x == 0 && threadIdx.x == 0) count[g] = c;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// (rows per wave, columns per lane): a function of (W, mesh) ONLY, so that the summation order does not depend on the chunking.
// Lat-lon: one row per wave (32 x 64: eight workgroups per plane, two waves per SIMD already at batch 8); HPX: two rows per wave
// up to 64 columns (every row block stages the whole plane again)
void diag_shape(int W, bool hpx, int* rpw, int* cp) {
    int c = 1;
    while (c * 64 < W) c *= 2;
    *cp = c;
    *rpw = hpx ? std::max(1, 2 / c) : 1;
}
constexpr int HPX_GROUP = 8;               // frames staged per group at most (HPX8: 8 x 6 KiB)

template <int MODE>
int launch_diag(const DiagArgs& a, int rpw, int cp, size_t lds, hipStream_t stream) {
    const dim3 grid(a.nslot / 4, a.V, a.Bc);
#define DLWP_DIAG_LAUNCH(R_, C_)                                                                                            \
    do {                                                                                                                    \
        if (lds) {                                                                                                          \
            const int rc = dlwp_ensure_lds((const void*)rollout_diag_kernel<R_, C_, MODE>, lds, "rollout_diag");            \
            if (rc) return rc;                                                                                              \
        }                                                                                                                   \
        hipLaunchKernelGGL((rollout_diag_kernel<R_, C_, MODE>), grid, dim3(256), lds, stream, a);                           \
    } while (0)
    if (cp == 1 && rpw == 1) DLWP_DIAG_LAUNCH(1, 1);
    else if (cp == 1) DLWP_DIAG_LAUNCH(2, 1);
    else if (cp == 2) DLWP_DIAG_LAUNCH(1, 2);
    else if (cp == 4) DLWP_DIAG_LAUNCH(1, 4);
    else DLWP_DIAG_LAUNCH(1, 8);
#undef DLWP_DIAG_LAUNCH
    return DLWP_OK;
}

}  // namespace

extern "C" long long dlwp_rollout_diag_ws_floats(int Bc, int Tc, int V, int H, int W, int hpx) {
    if (Bc <= 0 || Tc <= 0 || V <= 0 || H <= 0 || W <= 0) {
        dlwp_set_error("rollout_diag_ws_floats: Bc %d, Tc %d, V %d, H %d, W %d must be positive", Bc, Tc, V, H, W);
        return DLWP_E_INVALID;
    }
    if (W > 64 * MAX_CP) {
        dlwp_set_error("rollout_diag_ws_floats: W %d above %d", W, 64 * MAX_CP);
        return DLWP_E_UNSUPPORTED;
    }
    int rpw, cp;
    diag_shape(W, hpx != 0, &rpw, &cp);
    return (long long)Bc * Tc * V * (4LL * ceil_div(H, 4 * rpw)) * 5;
}

extern "C" int dlwp_rollout_diag(const float* out, long long out_bstride, long long out_tstride, const float* target,
                                 const float* scale, const float* shift, const float* row_weights, const float* clim,
                                 const int* month, int M, const int* idx, const float* w, int n, int Bc, int Tc, int V, int H, int W,
                                 int t_begin, int T, int w0, int w1, float* moments, float* zonal, float* wsum, float* ws,
                                 void* stream) {
    DLWP_REQUIRE(target, DLWP_E_INVALID, "rollout_diag: target is NULL");
    DLWP_REQUIRE(moments, DLWP_E_INVALID, "rollout_diag: moments is NULL");
    DLWP_REQUIRE(zonal, DLWP_E_INVALID, "rollout_diag: zonal is NULL");
    DLWP_REQUIRE(wsum, DLWP_E_INVALID, "rollout_diag: wsum is NULL");
    DLWP_REQUIRE(ws, DLWP_E_INVALID, "rollout_diag: ws is NULL (dlwp_rollout_diag_ws_floats gives its size)");
    DLWP_REQUIRE((idx != nullptr) == (w != nullptr), DLWP_E_INVALID, "rollout_diag: the hpx2ll table needs both idx and w, not one (NULL idx %d, NULL w %d)",
                 idx == nullptr, w == nullptr);
    const bool hpx = idx != nullptr;
    DLWP_REQUIRE(Bc > 0 && Tc > 0 && V > 0 && H > 0 && W > 0 && T > 0, DLWP_E_INVALID,
                 "rollout_diag: Bc %d, Tc %d, V %d, H %d, W %d, T %d must be positive", Bc, Tc, V, H, W, T);
    DLWP_REQUIRE(!hpx || n > 0, DLWP_E_INVALID, "rollout_diag: nside n %d must be positive with an hpx2ll table", n);
    DLWP_REQUIRE(out_bstride >= 0 && out_tstride >= 0, DLWP_E_INVALID, "rollout_diag: negative stride of out (batch %lld, time %lld)",
                 out_bstride, out_tstride);
    DLWP_REQUIRE((clim != nullptr) == (month != nullptr), DLWP_E_INVALID, "rollout_diag: clim and month go together (NULL clim %d, NULL month %d)",
                 clim == nullptr, month == nullptr);
    DLWP_REQUIRE(!clim || M > 0, DLWP_E_INVALID, "rollout_diag: M %d climatology maps must be positive", M);
    DLWP_REQUIRE(out || clim, DLWP_E_INVALID, "rollout_diag: out is NULL (the forecast is the climatology) but no clim is given");
    DLWP_REQUIRE(t_begin >= 0 && (long long)t_begin + Tc <= T, DLWP_E_INVALID, "rollout_diag: chunk t_begin %d + Tc %d is outside the rollout T %d",
                 t_begin, Tc, T);
    DLWP_REQUIRE(0 <= w0 && w0 <= w1 && w1 <= T, DLWP_E_INVALID, "rollout_diag: window [%d, %d) is outside [0, T = %d]", w0, w1, T);
    DLWP_REQUIRE(!hpx || (aligned16(idx) && aligned16(w)), DLWP_E_INVALID, "rollout_diag: idx and w must be 16-byte aligned");
    DLWP_REQUIRE(W <= 64 * MAX_CP, DLWP_E_UNSUPPORTED, "rollout_diag: W %d above %d columns", W, 64 * MAX_CP);
    DLWP_REQUIRE(V <= 65535 && Bc <= 65535 && (long long)H * W <= INT_MAX / 4 && (!hpx || n <= 8192), DLWP_E_UNSUPPORTED,
                 "rollout_diag: grid limits (V %d, Bc %d above 65535, %d x %d points, or n %d above 8192)", V, Bc, H, W, n);
    const int path = dlwp_tune_or("DIAG_PATH", 0);
    DLWP_REQUIRE(path >= 0 && path <= 2, DLWP_E_INVALID, "rollout_diag: DIAG_PATH %d is not 0 (auto), 1 (LDS) or 2 (direct)", path);
    DiagArgs a;
    a.npix = hpx ? 12 * n * n : H * W;
    const bool fits = 8LL * a.npix <= LDS_BUDGET;      // both planes of at least one frame
    DLWP_REQUIRE(!hpx || path != 1 || fits, DLWP_E_UNSUPPORTED, "rollout_diag: DIAG_PATH=1 but two planes of %d floats do not fit %d bytes of LDS",
                 a.npix, LDS_BUDGET);
    int rpw, cp;
    diag_shape(W, hpx, &rpw, &cp);
    a.out = out, a.target = target, a.scale = scale, a.shift = shift, a.roww = row_weights, a.clim = clim, a.month = month;
    a.idx = idx, a.w = w, a.bs = out_bstride, a.ts = out_tstride, a.M = M, a.Bc = Bc, a.Tc = Tc, a.V = V, a.H = H, a.W = W;
    a.t_begin = t_begin, a.T = T, a.w0 = w0, a.w1 = w1, a.nslot = 4 * ceil_div(H, 4 * rpw);
    a.vec = (!out || (aligned16(out) && out_bstride % 4 == 0 && out_tstride % 4 == 0)) && aligned16(target) && a.npix % 4 == 0;
    a.part = ws, a.zonal = zonal, a.wsum = wsum;
    a.pf = fits ? (int)std::min<long long>(std::min(HPX_GROUP, Tc), LDS_BUDGET / (8LL * a.npix)) : 1;      // staged frames per group
    const double bytes = 4.0 * Bc * Tc * V * (double)a.npix * (out ? 2 : 1);      // algorithmic: one read of outputs and targets
    {
        const int mode = !hpx ? MODE_LL : path == 1 || (path == 0 && fits) ? MODE_HPX_LDS : MODE_HPX_DIRECT;
        dlwp_prof_scope prof((hipStream_t)stream, 0.0, bytes, "%s",
                             mode == MODE_LL ? "rollout_diag_ll" : mode == MODE_HPX_LDS ? "rollout_diag_hpx_lds" : "rollout_diag_hpx_direct");
        int rc;
        if (mode == MODE_LL) rc = launch_diag<MODE_LL>(a, rpw, cp, 0, (hipStream_t)stream);
        else if (mode == MODE_HPX_LDS) rc = launch_diag<MODE_HPX_LDS>(a, rpw, cp, 8 * (size_t)a.npix * a.pf, (hipStream_t)stream);
        else rc = launch_diag<MODE_HPX_DIRECT>(a, rpw, cp, 0, (hipStream_t)stream);
        if (rc) return rc;
        DLWP_LAUNCH_CHECK();
    }
    const long long nm = (long long)Bc * Tc * V * 5;
    DLWP_REQUIRE((nm + 255) / 256 <= INT_MAX, DLWP_E_UNSUPPORTED, "rollout_diag: %lld moments are too many", nm);
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 4.0 * nm * (a.nslot + 1), "rollout_diag_fold");
    hipLaunchKernelGGL(moments_fold_kernel, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, scale, moments, nm,
                       Tc, V, a.nslot, t_begin, T);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_group_mean(const float* frames, const int* group, float* mean, int* count, long long N, long long P, int G,
                               void* stream) {
    DLWP_REQUIRE(frames, DLWP_E_INVALID, "group_mean: frames is NULL");
    DLWP_REQUIRE(group, DLWP_E_INVALID, "group_mean: group is NULL");
    DLWP_REQUIRE(mean, DLWP_E_INVALID, "group_mean: mean is NULL");
    DLWP_REQUIRE(count, DLWP_E_INVALID, "group_mean: count is NULL");
    DLWP_REQUIRE(N > 0 && P > 0 && G > 0, DLWP_E_INVALID, "group_mean: N %lld, P %lld, G %d must be positive", N, P, G);
    DLWP_REQUIRE(G <= GM_MAX_GROUPS, DLWP_E_UNSUPPORTED, "group_mean: G %d above %d groups", G, GM_MAX_GROUPS);
    DLWP_REQUIRE((P + 255) / 256 <= INT_MAX, DLWP_E_UNSUPPORTED, "group_mean: P %lld is too large", P);
    const size_t lds = ((size_t)G * 256 + G) * sizeof(float);
    const int rc = dlwp_ensure_lds((const void*)group_mean_kernel, lds, "group_mean");
    if (rc) return rc;
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 4.0 * ((double)N * P + (double)G * P), "group_mean");
    hipLaunchKernelGGL(group_mean_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), lds, (hipStream_t)stream, frames, group, mean,
                       count, N, P, G);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}
