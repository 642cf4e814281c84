// The wide, bipartite graph kernels of the dlwpbench GraphCastNet (hidden_dim 512, grid-to-mesh and mesh-to-grid graphs): the row
// MLPs of graph_ops.hip at widths 1..512, taken apart into (row tile x column block) launches.  This file is the forward pass; the
// backward pass is graph_bwd.hip's, on the kernels the 1..128 family uses.  Reference call sites
// (src/dlwpbench/models/graphcast/gnn_layers/): MeshGraphMLP.forward (mesh_graph_mlp.py), MeshGraphEdgeMLPConcat.forward over
// concat_efeat(e, (v_src, v_dst)) (utils.py), aggregate_and_concat (utils.py) in MeshGraphEncoder / MeshGraphDecoder /
// MeshNodeBlock.
//
// Layout as in graph_ops.hip: fp32 row-major [rows][width]; src, dst and the CSR arrays are int32 arrays of ONE sample's graph
// with Ns source nodes, Nd destination nodes and E edges (the mesh graph: Ns == Nd and the two node tensors are one); sample b's
// source node i is row b Ns + i, its destination node i row b Nd + i, its edge k row b E + k.  No atomics; every launch is
// bit-reproducible.  graph_ops.hip keeps a whole MLP's rows in LDS, which ends at 128 columns; here a hidden row is up to 512
// floats and a first operand row up to 1536, so one launch is ONE Linear:
//   wide_linear_kernel    Y[64 rows][64 | 128 columns] = act(A . W^T + b) [+ res] on row_gemm.hip.h's chunk loop, the operand rows
//                         assembled through the index while they are staged,
//                           ROWS  A[r] = x[r]
//                           EDGE  A[r] = e[r] | vs[b Ns + src[k]] | vd[b Nd + dst[k]]
//                           NODE  A[r] = agg[r] | v[r]     (agg: dlwp_graph_wide_gather_sum over the in-edges, mean or sum)
//                         so no concatenation exists in memory.  The epilogue stores the post-activation rows and, SiLU, the
//                         derivative rows d = s (1 + v (1 - s));
//   wide_ln_fwd_kernel    one wave per row (512 floats = 8 registers per lane): two-pass biased variance, affine, + residual;
//                         stores the normalised rows and 1 / sigma when a backward follows.
#include "graph_common.hip.h"

namespace {

using namespace rowgemm;
using namespace graphc;

// ---------------------------------------------------------------- one Linear, forward
struct LinArgs {
    Operand p;
    const float *w, *b, *res;     // w [N][K]; b, res [R][N] nullable
    float *y, *der;               // der nullable
    int N, act;
};

template <int MODE, int NS>
__global__ __launch_bounds__(256) void wide_linear_kernel(const LinArgs a) {
    constexpr int NC = NS * 16;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * NC;
    const long long K = a.p.K;
    RowSrc rs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) rs[i] = row_src<MODE>(a.p, m0 + (tid >> 4) + 16 * i);
    f32x4 acc[NS];
    row_gemm_chunks<NS>(
        a.p.K, acc,
        [&](int k, bool ok, float (&v)[4]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (ok && rs[i].o0 >= 0) ? operand_at<MODE>(a.p, rs[i], k) : 0.f;
        },
        [&](int kk, int col, bool ok) -> float {
            const int n = n0 + col;
            return (ok && n < a.N) ? a.w[n * K + kk] : 0.f;
        });
    // lane (r, g) register j holds row 16w + 4g + j, column 16 ns + r of the block
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long m = m0 + 16 * w + 4 * g + j;
        if (m >= a.p.R) continue;
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) {
            const int n = n0 + ns * 16 + r;
            if (n >= a.N) continue;
            const long long o = m * a.N + n;
            float val = acc[ns][j] + (a.b ? a.b[n] : 0.f);
            if (a.act == RELU) {
                val = fmaxf(val, 0.f);
            } else if (a.act == SILU) {
                float d;
                val = silu(val, d);
                if (a.der) a.der[o] = d;
            }
            if (a.res) val += a.res[o];
            a.y[o] = val;
        }
    }
}

template <int MODE>
void launch_linear(const LinArgs& a, hipStream_t s) {
    const int tiles = ceil_div(a.p.R, TM);
    if (a.N <= 64) hipLaunchKernelGGL((wide_linear_kernel<MODE, 4>), dim3(tiles, ceil_div(a.N, 64)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((wide_linear_kernel<MODE, 8>), dim3(tiles, ceil_div(a.N, 128)), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------- LayerNorm, one wave per row
__global__ __launch_bounds__(256) void wide_ln_fwd_kernel(const float* __restrict__ z, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const float* __restrict__ res,
                                                          float* __restrict__ y, float* __restrict__ xhat, float* __restrict__ rstd,
                                                          int R, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= R) return;
    float v[LN_REGS];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_REGS; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < C ? z[m * C + c] : 0.f;
        s += v[i];
    }
    const float mean = wave_sum(s) / (float)C;
    float vs = 0.f;
#pragma unroll
    for (int i = 0; i < LN_REGS; ++i)
        if (lane + 64 * i < C) vs += (v[i] - mean) * (v[i] - mean);
    const float rs = 1.0f / sqrtf(wave_sum(vs) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < LN_REGS; ++i) {
        const int c = lane + 64 * i;
        if (c >= C) continue;
        const long long o = m * C + c;
        float h = (v[i] - mean) * rs;
        if (xhat) xhat[o] = h;
        h = h * gamma[c] + beta[c];
        if (res) h += res[o];
        y[o] = h;
    }
    if (rstd && lane == 0) rstd[m] = rs;
}

}  // namespace

extern "C" int dlwp_graph_wide_linear_fwd(const dlwp_graph_wide_operand* op, const float* w, const float* b, const float* res, float* y,
                                          float* der, int N, int act, void* stream_) {
    LinArgs a{};
    long long rows;
    int rc = wide_operand("graph_wide_linear_fwd", op, &a.p, &rows);
    if (rc) return rc;
    DLWP_REQUIRE(width_ok(N, WIDE_MAXW), DLWP_E_UNSUPPORTED, "graph_wide_linear_fwd: output width %d outside 1..%d", N, WIDE_MAXW);
    DLWP_REQUIRE(act == NONE || act == RELU || act == SILU, DLWP_E_INVALID,
                 "graph_wide_linear_fwd: act %d is none of none (-1), relu (0), silu (1)", act);
    rc = operand_pointers("graph_wide_linear_fwd", op->mode, a.p);
    if (rc) return rc;
    DLWP_REQUIRE(w && y, DLWP_E_INVALID, "graph_wide_linear_fwd: NULL argument (w or y)");
    DLWP_REQUIRE(!der || act == SILU, DLWP_E_INVALID, "graph_wide_linear_fwd: derivative rows are stored for silu only");
    a.w = w; a.b = b; a.res = res; a.y = y; a.der = der; a.N = N; a.act = act;
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, 2.0 * rows * a.p.K * N, 4.0 * ((double)rows * (a.p.K + (der ? 2.0 : 1.0) * N) + (double)a.p.K * N),
                       "graph_wide_linear_%s", mode_name(op->mode));
    if (op->mode == ROWS) launch_linear<ROWS>(a, s);
    else if (op->mode == EDGE) launch_linear<EDGE>(a, s);
    else launch_linear<NODE>(a, s);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_graph_wide_ln_fwd(const float* z, const float* gamma, const float* beta, const float* res, float* y, float* xhat,
                                      float* rstd, long long rows, int C, float eps, void* stream_) {
    DLWP_REQUIRE(z && gamma && beta && y, DLWP_E_INVALID, "graph_wide_ln_fwd: NULL argument");
    DLWP_REQUIRE((xhat == nullptr) == (rstd == nullptr), DLWP_E_INVALID, "graph_wide_ln_fwd: xhat and rstd go together");
    const int rc = check_rows_c("graph_wide_ln_fwd", rows, C, WIDE_MAXW);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, 8.0 * rows * C, 4.0 * rows * C * (2.0 + (res ? 1.0 : 0.0) + (xhat ? 1.0 : 0.0)), "graph_wide_ln_fwd");
    hipLaunchKernelGGL(wide_ln_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, z, gamma, beta, res, y, xhat, rstd,
                       (int)rows, C, eps);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}
