// HEALPix <-> lat-lon remap: a 4-tap gather, its adjoint as a CSR gather, and the evaluation moments with the HEALPix -> lat-lon
// interpolation folded in.
//
// Reference: HEALPixRemap.ll2hpx / hpx2ll (src/dlwpbench/data/processing/healpix_mapping.py:328-399) remap one [lat, lon] or
// [12, n, n] map at a time on the CPU through reproject / astropy / healpy, in a five-process pool, and scripts/evaluate.py:71-109,
// 215-220 projects initial conditions, outputs and targets back to lat-lon before compute_metrics.  Here both directions are ONE
// table (dlwp_benchmark_amd/hpx_geometry.py: 4 source indices and 4 weights per output point, built once in float64 on the host)
// applied to `planes` = B T C maps per launch:
//   gather4 : dst[p][o] = sum_{k<4} w[4o+k] src[p stride + idx[4o+k]]
//   csr     : dst[p][r] (+)= sum_{rowptr[r] <= e < rowptr[r+1]} val[e] src[p][col[e]], e ascending, no atomics -- the gather's adjoint
//             with the transposed table (hpx_geometry.transpose_csr)
//   moments : dlwp_error_moments of hpx2ll(out), hpx2ll(target) without writing either lat-lon tensor
// The kernels cannot validate the device tables: 0 <= idx < n_in, rowptr monotone with rowptr[0] = 0, 0 <= col < n_in are the
// caller's precondition (hpx_remap.py checks them in numpy before the upload).
//
// gather4, LDS-staged path (a plane fits LDS_BUDGET).  A workgroup owns a tile of PT consecutive planes: each wave copies whole
// planes to LDS with 16-byte loads (a wave-load is 1 KB of one plane: coalesced; ds_write_b128 of consecutive 16-byte slots is
// conflict-free), then every thread loads the 4 indices and 4 weights of its output points ONCE (one 16-byte load each) and runs
// over the PT planes: per plane the 64 lanes of a wave read the same LDS image at the taps of 64 neighbouring output points, which
// are neighbouring source points (bilinear taps), so a ds_read_b32 sees mostly distinct banks (bank = dword % 32 per 32-lane half;
// the image is unpadded: lanes never stride by the plane size), and the store of dst[p][o .. o + 63] is one 256-byte run.  The
// tables cost 32 bytes per output point and workgroup, against 4 PT bytes of output.  With few plane tiles the output points are
// split over blockIdx.y as well so that more than `tiles` CUs work (each part stages the planes again: only when planes are few).
// Direct path (HPX64: 192 KB per plane): a thread keeps the taps of one output point in registers over a plane loop and gathers
// from global memory; neighbouring lanes hit neighbouring addresses, so the 4-byte gathers share cache lines.
//
// csr.  Row lengths are very uneven (HPX8 from 32 x 64: 96 entries for a polar pixel, 4 at the equator), so a row is not one lane's
// work: LG consecutive lanes share a row, lane j taking entries e0 + j, e0 + j + LG, ... in ascending order (their col / val loads
// are one contiguous run), each entry applied to the PT planes of the workgroup's tile from registers (one table load serves PT
// planes); the LG partial sums of a plane are then combined by a fixed xor butterfly -- the same order in every run, no atomics, so
// results are bit-reproducible.  LG = 8 where rows are long on average (the adjoint of hpx2ll: 10.7 entries), 2 where they are short
// (the adjoint of ll2hpx: 1.5; measured at HPX8 <-> 32 x 64 with 7296 planes: 115 us with 8 lanes per row).  The staged variant keeps the PT source planes in LDS (lanes of a row group read neighbouring
// columns of one plane); the results pass through a [PT][256 / LG + 1] LDS tile so that the store to dst runs along the row index
// in runs of at least 128 bytes.  Planes that do not fit LDS are read from global memory by the same code.  With few plane tiles the rows are split over
// blockIdx.y in multiples of the 256 / LG rows of one pass.
//
// moments.  One workgroup = one group g, 1024 lat-lon points (4 per thread, their taps and row weight in registers) and a range of
// the batch: per sample the two HEALPix planes are copied to LDS (16-byte loads) and every thread gathers its 4 x 2 x 4 taps there --
// the taps of a wave are 64 neighbouring points, but as global gathers they cost a texture-address cycle per distinct cache line
// and lane group (the first form of this kernel, one point per thread with global gathers, ran at 1.1 x the two-launch baseline);
// the climatology is read coalesced.  One atomic per moment and workgroup, as dlwp_error_moments.  Faces too large for LDS are
// gathered from global memory by the same code.
#include "common.hip.h"
#include "dlwpmi_internal.h"
#include <algorithm>

namespace {

constexpr int LDS_BUDGET = 72 * 1024;      // bytes of LDS a workgroup of the staged paths may use (two workgroups per CU; HPX8 <-> 32 x 64: 9 / 8 planes of 8 KB)
constexpr int MAX_PT = 16;                 // planes per workgroup tile
constexpr int WANT_WGS = 512;              // workgroups below which the output points are split over blockIdx.y as well

__device__ __forceinline__ float tap4(const float* __restrict__ s, const int4 i, const float4 w) {
    return fmaf(w.w, s[i.w], fmaf(w.z, s[i.z], fmaf(w.y, s[i.y], w.x * s[i.x])));
}

// wave wv of a 4-wave workgroup copies planes wv, wv + 4, ... of the tile to LDS (plane stride ldp floats; vec: 16-byte pieces)
__device__ __forceinline__ void stage_planes(float* lds, int ldp, const float* __restrict__ src, long long stride, int np, int n_in,
                                             int vec) {
    const int lane = lane_id();
    for (int p = wave_id(); p < np; p += 4) {
        const float* s = src + (long long)p * stride;
        float* d = lds + (long long)p * ldp;
        if (vec) {
            const int n4 = n_in >> 2;
#pragma unroll 4
            for (int u = lane; u < n4; u += WAVE) {
                const float4 v = reinterpret_cast<const float4*>(s)[u];
                reinterpret_cast<float4*>(d)[u] = v;
            }
        } else {
#pragma unroll 4
            for (int u = lane; u < n_in; u += WAVE) d[u] = s[u];
        }
    }
}

__global__ __launch_bounds__(256) void remap_gather4_lds_kernel(const float* __restrict__ src, long long stride,
                                                                const int* __restrict__ idx, const float* __restrict__ w,
                                                                float* __restrict__ dst, long long planes, int n_in, int n_out, int PT,
                                                                int ochunk, int vec) {
    extern __shared__ __align__(16) float lds[];             // [PT][n_in]
    const long long p0 = (long long)blockIdx.x * PT;
    const int np = planes - p0 < PT ? (int)(planes - p0) : PT;
    stage_planes(lds, n_in, src + p0 * stride, stride, np, n_in, vec);
    __syncthreads();
    const int o_begin = blockIdx.y * ochunk, o_end = min(n_out, o_begin + ochunk);
    for (int o = o_begin + threadIdx.x; o < o_end; o += 256) {
        const int4 i4 = reinterpret_cast<const int4*>(idx)[o];
        const float4 w4 = reinterpret_cast<const float4*>(w)[o];
        float* d = dst + p0 * n_out + o;
#pragma unroll 4
        for (int p = 0; p < np; ++p) d[(long long)p * n_out] = tap4(lds + p * n_in, i4, w4);
    }
}

__global__ __launch_bounds__(256) void remap_gather4_direct_kernel(const float* __restrict__ src, long long stride,
                                                                   const int* __restrict__ idx, const float* __restrict__ w,
                                                                   float* __restrict__ dst, long long planes, int n_out, int ppb) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= n_out) return;
    const int4 i4 = reinterpret_cast<const int4*>(idx)[o];
    const float4 w4 = reinterpret_cast<const float4*>(w)[o];
    const long long p_begin = (long long)blockIdx.y * ppb, p_end = p_begin + ppb < planes ? p_begin + ppb : planes;
#pragma unroll 4
    for (long long p = p_begin; p < p_end; ++p) dst[p * n_out + o] = tap4(src + p * stride, i4, w4);
}

// LG lanes share a row (8: long rows, the adjoint of hpx2ll; 2: short rows, the adjoint of ll2hpx); 256 / LG rows per pass
template <int PT, int LG, bool STAGED>
__global__ __launch_bounds__(256) void remap_csr_kernel(const float* __restrict__ src, const int* __restrict__ rowptr,
                                                        const int* __restrict__ col, const float* __restrict__ val, float* dst,
                                                        long long planes, int n_in, int n_out, int accumulate, int rchunk, int vec) {
    constexpr int RPP = 256 / LG;
    extern __shared__ __align__(16) float lds[];             // STAGED: [PT][n_in] source planes, then the [PT][RPP + 1] result tile
    const long long p0 = (long long)blockIdx.x * PT;
    const int np = planes - p0 < PT ? (int)(planes - p0) : PT;
    float* otile = lds + (STAGED ? PT * n_in : 0);
    if (STAGED) {
        stage_planes(lds, n_in, src + p0 * n_in, n_in, np, n_in, vec);
        __syncthreads();
    }
    const float* s = STAGED ? lds : src + p0 * n_in;
    const int j = threadIdx.x & (LG - 1), rl = threadIdx.x / LG;            // compute: LG lanes per row
    const int r_begin = blockIdx.y * rchunk, r_end = min(n_out, r_begin + rchunk);
    for (int r0 = r_begin; r0 < r_end; r0 += RPP) {
        float acc[PT];
#pragma unroll
        for (int p = 0; p < PT; ++p) acc[p] = 0.f;
        const int r = r0 + rl;
        if (r < r_end) {
            const int e1 = rowptr[r + 1];
#pragma unroll 4
            for (int e = rowptr[r] + j; e < e1; e += LG) {
                const int c = col[e];
                const float v = val[e];
#pragma unroll
                for (int p = 0; p < PT; ++p)
                    if (STAGED || p < np) acc[p] = fmaf(v, s[(size_t)p * n_in + c], acc[p]);      // (staged planes >= np: unused LDS)
            }
        }
#pragma unroll
        for (int p = 0; p < PT; ++p) {                                       // the LG partial sums of a row, combined in a fixed order
#pragma unroll
            for (int o = 1; o < LG; o <<= 1) acc[p] += __shfl_xor(acc[p], o);
            if (j == (PT <= LG ? p : 0)) otile[p * (RPP + 1) + rl] = acc[p];      // (every lane of the group holds the sum)
        }
        __syncthreads();
        for (int q = threadIdx.x; q < np * RPP; q += 256) {                  // store: the row runs fastest
            const int pp = q / RPP, rr = q - pp * RPP;
            if (r0 + rr < r_end) {
                float* d = dst + (p0 + pp) * n_out + r0 + rr;
                const float v = otile[pp * (RPP + 1) + rr];
                *d = accumulate ? *d + v : v;
            }
        }
        __syncthreads();
    }
}

// (the block reduction of csrc/train_ops.hip's error_moments_kernel)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ void block_atomic_sum(float v, float* out) {
    __shared__ float part[4];
    v = wave_sum(v);
    if (lane_id() == 0) part[wave_id()] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomic_add_f32(out, part[0] + part[1] + part[2] + part[3]);
}

constexpr int KP = 4;                      // lat-lon points per thread of the moments kernel (8: 185 VGPRs, two waves per SIMD)

template <bool STAGED>
__global__ __launch_bounds__(256) void hpx_error_moments_kernel(const float* __restrict__ o, const float* __restrict__ t,
                                                                const float* __restrict__ c, const float* __restrict__ roww,
                                                                const int* __restrict__ idx, const float* __restrict__ w, int B, int G,
                                                                int npix, int H, int W, int bchunk, int vec, float* m) {
    extern __shared__ __align__(16) float lds[];             // STAGED: the out plane, then the target plane of one sample
    const int g = blockIdx.x, hw = H * W, rbase = blockIdx.y * (KP * 256) + threadIdx.x;
    int4 i4[KP];
    float4 w4[KP];
    float wr[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        const int r = rbase + k * 256;
        if (r < hw) {
            i4[k] = reinterpret_cast<const int4*>(idx)[r];
            w4[k] = reinterpret_cast<const float4*>(w)[r];
            wr[k] = roww ? roww[r / W] : 1.f;
        } else {
            i4[k] = make_int4(0, 0, 0, 0);
            w4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            wr[k] = 0.f;
        }
    }
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
    const int b_begin = blockIdx.z * bchunk, b_end = min(B, b_begin + bchunk);
    for (int b = b_begin; b < b_end; ++b) {
        const long long plane = (long long)b * G + g;
        const float *go = o + plane * npix, *gt = t + plane * npix;
        const float *so = STAGED ? lds : go, *st = STAGED ? lds + npix : gt;
        if (STAGED) {
            if (vec) {
                const int n4 = npix >> 2;
                for (int u = threadIdx.x; u < n4; u += 256) {
                    reinterpret_cast<float4*>(lds)[u] = reinterpret_cast<const float4*>(go)[u];
                    reinterpret_cast<float4*>(lds + npix)[u] = reinterpret_cast<const float4*>(gt)[u];
                }
            } else {
                for (int u = threadIdx.x; u < npix; u += 256) {
                    lds[u] = go[u];
                    lds[npix + u] = gt[u];
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const int r = rbase + k * 256;
            if (r < hw) {
                const float ov = tap4(so, i4[k], w4[k]), tv = tap4(st, i4[k], w4[k]), d = ov - tv;
                a0 += wr[k] * d * d;
                a1 += wr[k] * fabsf(d);
                if (c) {
                    const float cv = c[plane * hw + r], oc = ov - cv, tc = tv - cv;
                    a2 += wr[k] * oc * tc;
                    a3 += wr[k] * oc * oc;
                    a4 += wr[k] * tc * tc;
                }
            }
        }
        if (STAGED) __syncthreads();       // the next sample's copy overwrites the planes
    }
    block_atomic_sum(a0, m + g);
    __syncthreads();                       // block_atomic_sum reuses one LDS scratch
    block_atomic_sum(a1, m + G + g);
    if (c) {
        __syncthreads();
        block_atomic_sum(a2, m + 2 * G + g);
        __syncthreads();
        block_atomic_sum(a3, m + 3 * G + g);
        __syncthreads();
        block_atomic_sum(a4, m + 4 * G + g);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// blockIdx.y parts of `n` items for `tiles` plane tiles: 1 when the tiles alone fill the device, never parts below 256 items
int split_parts(long long tiles, int n) {
    if (tiles >= WANT_WGS) return 1;
    return (int)std::max<long long>(1, std::min<long long>((WANT_WGS + tiles - 1) / tiles, (n + 255) / 256));
}

}  // namespace

extern "C" int dlwp_remap_gather4(const float* src, long long src_plane_stride, const int* idx, const float* w, float* dst,
                                  long long planes, int n_in, int n_out, void* stream) {
    DLWP_REQUIRE(src && idx && w && dst, DLWP_E_INVALID, "remap_gather4: NULL argument");
    DLWP_REQUIRE(planes > 0 && n_in > 0 && n_out > 0, DLWP_E_INVALID, "remap_gather4: planes %lld, n_in %d, n_out %d must be positive",
                 planes, n_in, n_out);
    DLWP_REQUIRE(src_plane_stride >= n_in, DLWP_E_INVALID, "remap_gather4: plane stride %lld < n_in %d", src_plane_stride, n_in);
    DLWP_REQUIRE(aligned16(idx) && aligned16(w), DLWP_E_INVALID, "remap_gather4: idx and w must be 16-byte aligned");
    const int path = dlwp_tune_or("REMAP_PATH", 0);
    DLWP_REQUIRE(path >= 0 && path <= 2, DLWP_E_INVALID, "remap_gather4: REMAP_PATH %d is not 0 (auto), 1 (LDS) or 2 (direct)", path);
    const bool fits = (long long)n_in * 4 <= LDS_BUDGET;
    DLWP_REQUIRE(path != 1 || fits, DLWP_E_UNSUPPORTED, "remap_gather4: REMAP_PATH=1 but a plane of %d floats does not fit %d bytes of LDS",
                 n_in, LDS_BUDGET);
    const double bytes = 4.0 * (double)planes * ((double)n_in + n_out);
    if (path == 1 || (path == 0 && fits)) {
        const int PT = (int)std::min<long long>(std::min(MAX_PT, LDS_BUDGET / (4 * n_in)), planes);
        const long long tiles = (planes + PT - 1) / PT;
        DLWP_REQUIRE(tiles <= INT_MAX, DLWP_E_UNSUPPORTED, "remap_gather4: %lld planes are too many", planes);
        const int parts = split_parts(tiles, n_out), ochunk = ceil_div(n_out, parts);
        const int vec = aligned16(src) && src_plane_stride % 4 == 0 && n_in % 4 == 0;
        const size_t lds = (size_t)PT * n_in * sizeof(float);
        const int rc = dlwp_ensure_lds((const void*)remap_gather4_lds_kernel, lds, "remap_gather4");
        if (rc) return rc;
        dlwp_prof_scope prof((hipStream_t)stream, 8.0 * planes * n_out, bytes, "remap_gather4_lds");
        hipLaunchKernelGGL(remap_gather4_lds_kernel, dim3((unsigned)tiles, ceil_div(n_out, ochunk)), dim3(256), lds,
                           (hipStream_t)stream, src, src_plane_stride, idx, w, dst, planes, n_in,
                           n_out, PT, ochunk, vec);
    } else {
        const int gx = ceil_div(n_out, 256);
        long long ppb = std::max<long long>(1, planes / std::max(1, 2048 / gx));
        ppb = std::max(ppb, (planes + 65534) / 65535);
        dlwp_prof_scope prof((hipStream_t)stream, 8.0 * planes * n_out, bytes, "remap_gather4_direct");
        hipLaunchKernelGGL(remap_gather4_direct_kernel, dim3(gx, (unsigned)((planes + ppb - 1) / ppb)), dim3(256), 0,
                           (hipStream_t)stream, src, src_plane_stride, idx, w, dst, planes, n_out, (int)std::min<long long>(ppb, INT_MAX));
    }
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_remap_csr(const float* src, const int* rowptr, const int* col, const float* val, float* dst, long long planes,
                              int n_in, int n_out, int accumulate, void* stream) {
    DLWP_REQUIRE(src && rowptr && col && val && dst, DLWP_E_INVALID, "remap_csr: NULL argument");
    DLWP_REQUIRE(planes > 0 && n_in > 0 && n_out > 0, DLWP_E_INVALID, "remap_csr: planes %lld, n_in %d, n_out %d must be positive", planes,
                 n_in, n_out);
    // the table is a transposed 4-tap gather: 4 n_in entries over n_out rows.  Long rows (HPX8 pixels read by 32 x 64: 10.7 on average,
    // 96 at the poles) take 8 lanes each, short ones (32 x 64 cells read by HPX8: 1.5) two
    const int LG = n_in >= n_out ? 8 : 2, RPP = 256 / LG;
    auto lds_bytes = [&](int pt, bool staged) { return ((staged ? (long long)pt * n_in : 0) + pt * (RPP + 1)) * (long long)sizeof(float); };
    // planes per tile: 2 with 8 lanes per row, 4 with 2.  Measured at HPX8 <-> 32 x 64 with 7296 planes (us at 8 / 4 / 2 planes per
    // tile): 8 lanes per row 112 / 91.5 / 82.4, 2 lanes per row 32.1 / 28.0 / 36.0 -- the long-row form waits on its 12-step polar
    // rows and gains from more resident workgroups (less LDS each) more than it loses on table reads per plane
    int PT = LG == 8 ? 2 : 4;
    while (PT > 1 && PT / 2 >= planes) PT /= 2;
    while (PT > 1 && lds_bytes(PT, true) > LDS_BUDGET) PT /= 2;
    const bool staged = lds_bytes(PT, true) <= LDS_BUDGET;
    if (!staged) PT = 8;                                                   // (global reads: no LDS to share, one table read per 8 planes)
    const long long tiles = (planes + PT - 1) / PT;
    DLWP_REQUIRE(tiles <= INT_MAX, DLWP_E_UNSUPPORTED, "remap_csr: %lld planes are too many", planes);
    const int passes = ceil_div(n_out, RPP);
    const int parts = tiles >= WANT_WGS ? 1 : (int)std::min<long long>((WANT_WGS + tiles - 1) / tiles, passes);
    const int rchunk = ceil_div(passes, parts) * RPP;
    DLWP_REQUIRE(ceil_div(n_out, rchunk) <= 65535, DLWP_E_UNSUPPORTED, "remap_csr: n_out %d is too large", n_out);
    const int vec = aligned16(src) && n_in % 4 == 0;
    const dim3 grid((unsigned)tiles, ceil_div(n_out, rchunk));
    const size_t lds = (size_t)lds_bytes(PT, staged);
    const double bytes = 4.0 * (double)planes * ((double)n_in + (accumulate ? 2.0 : 1.0) * n_out);
#define DLWP_CSR_LAUNCH(PT_, LG_, ST_)                                                                                                \
    do {                                                                                                                              \
        const int rc = ST_ ? dlwp_ensure_lds((const void*)remap_csr_kernel<PT_, LG_, ST_>, lds, "remap_csr") : DLWP_OK;               \
        if (rc) return rc;                                                                                                            \
        dlwp_prof_scope prof((hipStream_t)stream, 0.0, bytes, "remap_csr");                                                           \
        hipLaunchKernelGGL((remap_csr_kernel<PT_, LG_, ST_>), grid, dim3(256), lds, (hipStream_t)stream, src, rowptr, col, val, dst,  \
                           planes, n_in, n_out, accumulate, rchunk, vec);                                                             \
    } while (0)
    if (LG == 8) {
        if (!staged) DLWP_CSR_LAUNCH(8, 8, false);
        else if (PT == 2) DLWP_CSR_LAUNCH(2, 8, true);
        else DLWP_CSR_LAUNCH(1, 8, true);
    } else {
        if (!staged) DLWP_CSR_LAUNCH(8, 2, false);
        else if (PT == 4) DLWP_CSR_LAUNCH(4, 2, true);
        else if (PT == 2) DLWP_CSR_LAUNCH(2, 2, true);
        else DLWP_CSR_LAUNCH(1, 2, true);
    }
#undef DLWP_CSR_LAUNCH
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_hpx_error_moments(const float* out_hpx, const float* target_hpx, const float* climatology_ll,
                                      const float* row_weights, const int* idx, const float* w, int B, int G, int n, int H, int W,
                                      float* moments, void* stream) {
    DLWP_REQUIRE(out_hpx && target_hpx && idx && w && moments, DLWP_E_INVALID, "hpx_error_moments: NULL argument");
    DLWP_REQUIRE(B > 0 && G > 0 && n > 0 && H > 0 && W > 0, DLWP_E_INVALID, "hpx_error_moments: B %d, G %d, n %d, H %d, W %d must be positive",
                 B, G, n, H, W);
    DLWP_REQUIRE(n <= 8192 && (long long)H * W <= 65535LL * 256, DLWP_E_UNSUPPORTED,
                 "hpx_error_moments: n %d above 8192 or %d x %d above 65535 x 256 points", n, H, W);
    DLWP_REQUIRE(aligned16(idx) && aligned16(w), DLWP_E_INVALID, "hpx_error_moments: idx and w must be 16-byte aligned");
    const int npix = 12 * n * n, hw = H * W;
    const bool staged = 8LL * npix <= LDS_BUDGET;                          // both planes of a sample in LDS
    const int ny = ceil_div(hw, KP * 256);
    const int bsplit = (int)std::max<long long>(1, std::min<long long>(B, 1024 / ((long long)G * ny)));
    const int bchunk = ceil_div(B, bsplit);
    DLWP_REQUIRE(ceil_div(B, bchunk) <= 65535, DLWP_E_UNSUPPORTED, "hpx_error_moments: B %d is too large", B);
    const int vec = aligned16(out_hpx) && aligned16(target_hpx);          // (12 n^2 is a multiple of 4)
    const dim3 grid(G, ny, ceil_div(B, bchunk));
    const size_t lds = 8 * (size_t)npix;
    if (staged) {
        const int rc = dlwp_ensure_lds((const void*)hpx_error_moments_kernel<true>, lds, "hpx_error_moments");
        if (rc) return rc;
    }
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 4.0 * (double)B * G * (2.0 * npix + (climatology_ll ? hw : 0)), "hpx_error_moments");
    if (staged) {
        hipLaunchKernelGGL(hpx_error_moments_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, out_hpx, target_hpx, climatology_ll,
                           row_weights, idx, w, B, G, npix, H, W, bchunk, vec, moments);
    } else {
        hipLaunchKernelGGL(hpx_error_moments_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, out_hpx, target_hpx, climatology_ll,
                           row_weights, idx, w, B, G, npix, H, W, bchunk, vec, moments);
    }
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}
