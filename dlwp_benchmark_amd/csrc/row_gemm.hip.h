// The two loops over the exact-fp32 MFMA (common.hip.h mfma16 / mfma16_chunk) that the row kernels share (unet_ops.hip: 1 x 1 and
// 2 x 2 up-convolution; graph_bwd.hip: the first Linear's backward; graph_wide.hip: one Linear), one workgroup of 4 waves each:
//   row_gemm_chunks   Y[64 rows][NS*16] = A[64][K] . Wm[K][N], K in chunks of 16
//   row_wgrad_tiles   gW = A^T . dZ with K = rows, split over S workgroups that each walk the 64-row tiles s, s + S, ...; the
//                     partial sums are folded in the fixed order s = 0..S-1 (row_wgrad_fold_kernel), so no atomics: two launches
//                     on the same operands are bit-identical
// A caller says where an element comes from (its loaders) and where a result goes (its epilogue); nothing here knows a mode.
// conv3x3.hip (haloed tiles, nine taps, packed weight images) has loops of its own and takes the constants and the split rule.
#pragma once
#include "common.hip.h"
#include "dlwpmi_internal.h"

namespace rowgemm {

constexpr int TM = 64;        // rows (pixels) per workgroup tile
constexpr int KC = 16;        // K values per chunk
constexpr int AP = 20;        // LDS floats per row of an operand tile (16 + 4: conflict-free 16-byte reads)
constexpr int ZP = 80;        // LDS floats per row of the dz tile of a weight-gradient kernel (64 + 16)

// Split-K geometry of a weight gradient [kw][ncols] (kw: the operand width INCLUDING the bias column) over ntiles row tiles:
// workgroups own 16 x 64 blocks of the padded result, and S of them share a block so that about 512 are in flight
inline void split_k_geometry(int ntiles, int kw, int ncols, int* k_pad, int* n_pad, int* S) {
    *k_pad = round_up(kw, KC);
    *n_pad = round_up(ncols, 64);
    const int blocks = (*k_pad / KC) * (*n_pad / 64);
    int s = ceil_div(512, blocks);
    if (s > 32) s = 32;
    if (s > ntiles) s = ntiles;
    *S = s;
}

inline int row_tiles(long long rows) { return (int)((rows + TM - 1) / TM); }

// floats of the partial-sum scratch [S][k_pad][n_pad] of launch_row_wgrad(rows, K, N)
inline long long row_wgrad_ws_floats(long long rows, int K, int N) {
    int k_pad, n_pad, S;
    split_k_geometry(row_tiles(rows), K + 1, N, &k_pad, &n_pad, &S);
    return (long long)S * k_pad * n_pad;
}

// acc[ns] = sum_k A[row][k] Wm[k][16 ns + r] for the 64 rows x NS*16 columns of one workgroup (256 threads); on return lane
// (r, g) of wave w holds in acc[ns][j] row 16w + 4g + j, column 16 ns + r.
//   loadA(k, ok, v)      v[i] = element k of staged row (tid >> 4) + 16 i, i = 0..3 (all four at once: what depends on k alone,
//                        such as a division, is then formed once), 0 for a row beyond the caller's extent
//   loadW(kk, col, ok)   Wm[kk][col] of the workgroup's column block, 0 for a column beyond it
// ok is this function's zero fill up to the chunk (k < K; nothing in memory is padded).  A loader joins it to its own bound in ONE
// condition, `(ok && row in range) ? load : 0.f`: a test here around a test there compiles to nested branches with the address
// arithmetic repeated (up to + 12 VGPRs, profiles/r10_experiments.md).  Per chunk the operand tile [64][16] and the weight tile
// [g][column][4 K values] are staged in LDS through registers, one chunk ahead.
template <int NS, class LoadA, class LoadW>
__device__ __forceinline__ void row_gemm_chunks(int K, f32x4 (&acc)[NS], LoadA loadA, LoadW loadW) {
    constexpr int NC = NS * 16;
    static_assert(KC * NC == 256 * NS, "the weight tile is NS elements per thread");
    __shared__ float As[TM * AP];
    __shared__ float Ws[KC * NC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) acc[ns] = f32x4{0.f, 0.f, 0.f, 0.f};

    float v[4], wv[NS];
    // chunk kc's operand and weight tiles, global -> registers (issued one chunk ahead: in flight during the MFMAs)
    auto fetch = [&](int kc) {
        const int k = kc * KC + (tid & 15);
        loadA(k, k < K, v);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int u = tid + 256 * i;                   // Ws index: ((g * NC + column) * 4 + s)
            const int s = u & 3, col = (u >> 2) % NC, gg = (u >> 2) / NC;
            const int kk = kc * KC + 4 * gg + s;
            wv[i] = loadW(kk, col, kk < K);
        }
    };
    const int nchunks = (K + KC - 1) / KC;
    fetch(0);
    for (int kc = 0; kc < nchunks; ++kc) {
        if (kc) __syncthreads();                  // the previous chunk's fragments have been read
#pragma unroll
        for (int i = 0; i < 4; ++i) As[((tid >> 4) + 16 * i) * AP + (tid & 15)] = v[i];
#pragma unroll
        for (int i = 0; i < NS; ++i) Ws[tid + 256 * i] = wv[i];
        __syncthreads();
        if (kc + 1 < nchunks) fetch(kc + 1);      // after the barrier: __syncthreads() waits for loads in flight
        const f32x4 af = *reinterpret_cast<const f32x4*>(&As[(16 * w + r) * AP + 4 * g]);
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) {
            const f32x4 bf = *reinterpret_cast<const f32x4*>(&Ws[(g * NC + ns * 16 + r) * 4]);
            acc[ns] = mfma16_chunk(af, bf, acc[ns]);
        }
    }
}

// Workgroup (operand block blockIdx.x of 16, dz column block blockIdx.y of 64, split blockIdx.z) of a weight-gradient kernel:
// walks the row tiles blockIdx.z, blockIdx.z + S, ... and stores its partial sums to ws [S][k_pad][n_pad].
//   loadA(m)  operand column blockIdx.x * 16 + (tid & 15) of row m: the constant 1 for the bias column, 0 beyond it
//   loadZ(m)  dz column blockIdx.y * 64 + (tid & 63) of row m, 0 beyond the last column
// Both return 0 for a row beyond the caller's extent.  Tiles are staged in LDS through registers, one tile ahead.
template <class LoadA, class LoadZ>
__device__ __forceinline__ void row_wgrad_tiles(float* ws, int ntiles, int S, int k_pad, int n_pad, LoadA loadA, LoadZ loadZ) {
    __shared__ float As[TM * KC];
    __shared__ float Zs[TM * ZP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    float v[4], zv[16];
    auto fetch = [&](int t) {
        const int m0 = t * TM;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = loadA(m0 + (tid >> 4) + 16 * i);
#pragma unroll
        for (int i = 0; i < 16; ++i) zv[i] = loadZ(m0 + (tid >> 6) + 4 * i);
    };
    if ((int)blockIdx.z < ntiles) fetch(blockIdx.z);
    for (int t = blockIdx.z; t < ntiles; t += S) {
        __syncthreads();                          // the previous tile has been consumed
#pragma unroll
        for (int i = 0; i < 4; ++i) As[((tid >> 4) + 16 * i) * KC + (tid & 15)] = v[i];
#pragma unroll
        for (int i = 0; i < 16; ++i) Zs[((tid >> 6) + 4 * i) * ZP + (tid & 63)] = zv[i];
        __syncthreads();
        if (t + S < ntiles) fetch(t + S);
#pragma unroll 4
        for (int i = 0; i < TM / 4; ++i) {
            const int m = 4 * i + g;
            acc = mfma16(As[m * KC + r], Zs[m * ZP + 16 * w + r], acc);
        }
    }
    // lane (r, g) register j: operand column 4g + j of the block, dz column 16w + r of the block
    float* dst = ws + (long long)blockIdx.z * k_pad * n_pad;
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[(long long)(blockIdx.x * KC + 4 * g + j) * n_pad + blockIdx.y * 64 + 16 * w + r] = acc[j];
}

// gw[col][k] += sum_s ws[s][k][col],  gb[col] += sum_s ws[s][K][col]      (gw: a Linear's / 1 x 1 convolution's own [N][K]).
// NT threads per workgroup; a template so that only the translation units that launch it carry a copy.
template <int NT = 256>
__global__ __launch_bounds__(NT) void row_wgrad_fold_kernel(const float* __restrict__ ws, float* gw, float* gb, int K, int N, int S,
                                                            int k_pad, int n_pad) {
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;       // (k <= K, column), column fastest
    if (e >= (long long)(K + 1) * N) return;
    const int col = (int)(e % N), k = (int)(e / N);
    const long long stride = (long long)k_pad * n_pad;
    const float* p = ws + (long long)k * n_pad + col;
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += p[i * stride];
    if (k < K) gw[(long long)col * K + k] += s;
    else if (gb) gb[col] += s;
}

using fold_kernel_t = void (*)(const float*, float*, float*, int, int, int, int, int);

// Weight gradient + fold of an operand [rows][K] and a dz [rows][N]: fills the geometry fields of the kernel's argument struct
// (ntiles, S, k_pad, n_pad; ws is the caller's) and launches `wgrad`, a kernel built on row_wgrad_tiles, then `fold`.
template <class Args>
int launch_row_wgrad(void (*wgrad)(Args), Args& a, long long rows, int K, int N, float* gw, float* gb, hipStream_t s, const char* name,
                     const char* fold_name, fold_kernel_t fold = row_wgrad_fold_kernel<>) {
    a.ntiles = row_tiles(rows);
    split_k_geometry(a.ntiles, K + 1, N, &a.k_pad, &a.n_pad, &a.S);
    {
        dlwp_prof_scope ps(s, 2.0 * rows * (K + 1.0) * N, 4.0 * ((double)rows * (K + N) + (double)a.S * a.k_pad * a.n_pad), "%s", name);
        hipLaunchKernelGGL(wgrad, dim3(a.k_pad / KC, a.n_pad / 64, a.S), dim3(256), 0, s, a);
        DLWP_LAUNCH_CHECK();
    }
    {
        const long long n = (long long)(K + 1) * N;
        dlwp_prof_scope ps(s, (double)a.S * n, 4.0 * (a.S + 2.0) * n, "%s", fold_name);
        hipLaunchKernelGGL(fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.ws, gw, gb, K, N, a.S, a.k_pad, a.n_pad);
        DLWP_LAUNCH_CHECK();
    }
    return DLWP_OK;
}

}  // namespace rowgemm
