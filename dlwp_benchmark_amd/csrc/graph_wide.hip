// The wide, bipartite graph kernels of the dlwpbench GraphCastNet (hidden_dim 512, grid-to-mesh and mesh-to-grid graphs): the row
// MLPs of graph_ops.hip at widths 1..512, taken apart into (row tile x column block) launches.  Reference call sites
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
//                           NODE  A[r] = agg[r] | v[r]     (agg: wide_gather_sum_kernel over the in-edges, mean or sum)
//                         so no concatenation exists in memory.  The epilogue stores the post-activation rows and, SiLU, the
//                         derivative rows d = s (1 + v (1 - s));
//   wide_ln_fwd_kernel    one wave per row (512 floats = 8 registers per lane): two-pass biased variance, affine, + residual;
//                         stores the normalised rows and 1 / sigma when a backward follows;
//   wide_ln_bwd_kernel    one wave per row from the stored rows; gamma / beta gradients are per-lane column sums over a workgroup's
//                         rows, folded over the four waves and then over the workgroups in a fixed order;
//   wide_dgrad_kernel     dA = dz . W, written in parts (EDGE: de, per-edge d_src, per-edge d_dst; NODE: d_agg, dv; ROWS: dx,
//                         times the stored derivative rows or ReLU's mask: the backward of a LATER Linear in one launch);
//   wide_wgrad0_kernel    gW0 = dz^T . A with A gathered again, on row_wgrad_tiles' split-K walk and fold (later Linears read stored
//                         rows: dlwp_conv1x1_wgrad takes them at any width);
//   wide_gather_sum_kernel / wide_edge_gather_kernel   the CSR sums onto ONE node set (out-edges onto sources, in-edges onto
//                         destinations are two launches: the sets differ) and the gather back along dst.
#include "row_gemm.hip.h"

namespace {

using namespace rowgemm;
constexpr int MAXW = DLWP_GRAPH_WIDE_MAX_WIDTH;
constexpr int LN_REGS = MAXW / 64;                     // floats of a row per lane
constexpr long long ROW_LIMIT = (1ll << 31) - 64;      // the kernels form row indices of a whole last 64-row tile in int

enum { ROWS = DLWP_GRAPH_ROWS, EDGE = DLWP_GRAPH_EDGE, NODE = DLWP_GRAPH_NODE };
enum { NONE = DLWP_GRAPH_WIDE_ACT_NONE, RELU = DLWP_GRAPH_ACT_RELU, SILU = DLWP_GRAPH_ACT_SILU };

// the operand of a first Linear: ROWS x; EDGE x = e, vs, vd; NODE x = agg, vs = v.  Part widths D0 | D1 | D2, K their sum
struct Operand {
    const float *x, *vs, *vd;
    const int *src, *dst;
    int R, Ns, Nd, E, D0, D1, D2, K;
};

struct RowSrc {
    long long o0, o1, o2;     // float offsets of the row's parts; o0 < 0: row beyond R
};

template <int MODE>
__device__ __forceinline__ RowSrc row_src(const Operand& p, int m) {
    RowSrc s{-1, 0, 0};
    if (m >= p.R) return s;
    s.o0 = (long long)m * p.D0;
    if constexpr (MODE == EDGE) {
        const int b = m / p.E, k = m - b * p.E;
        s.o1 = ((long long)b * p.Ns + p.src[k]) * p.D1;
        s.o2 = ((long long)b * p.Nd + p.dst[k]) * p.D2;
    } else if constexpr (MODE == NODE) {
        s.o1 = (long long)m * p.D1;
    }
    return s;
}

// operand element k (< K) of a row
template <int MODE>
__device__ __forceinline__ float operand_at(const Operand& p, const RowSrc& s, int k) {
    if constexpr (MODE == ROWS) {
        return p.x[s.o0 + k];
    } else if constexpr (MODE == EDGE) {
        return k < p.D0 ? p.x[s.o0 + k] : (k < p.D0 + p.D1 ? p.vs[s.o1 + (k - p.D0)] : p.vd[s.o2 + (k - p.D0 - p.D1)]);
    } else {
        return k < p.D0 ? p.x[s.o0 + k] : p.vs[s.o1 + (k - p.D0)];
    }
}

// as graph_ops.hip's: far out s is exactly 0 or 1 and the pair is (-0, -0) or (v, 1)
__device__ __forceinline__ float silu(float v, float& d) {
    const float s = 1.0f / (1.0f + __expf(-v));
    d = s * (1.0f + v * (1.0f - s));
    return v * s;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

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

// dz = rstd (dy gamma - mean_c(dy gamma) - xhat mean_c(dy gamma xhat));  ws[blk][0][c] = sum_rows dy xhat,  ws[blk][1][c] = sum_rows dy
__global__ __launch_bounds__(256) void wide_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                          const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                          float* __restrict__ dz, float* __restrict__ ws, int R, int C) {
    __shared__ float P[3][2][MAXW];               // the column sums of waves 1..3
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float gm[LN_REGS], pg[LN_REGS], pb[LN_REGS];
#pragma unroll
    for (int i = 0; i < LN_REGS; ++i) {
        gm[i] = lane + 64 * i < C ? gamma[lane + 64 * i] : 0.f;
        pg[i] = pb[i] = 0.f;
    }
    for (long long m = (long long)blockIdx.x * 4 + w; m < R; m += (long long)gridDim.x * 4) {
        float gy[LN_REGS], xh[LN_REGS];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < LN_REGS; ++i) {
            const int c = lane + 64 * i;
            gy[i] = c < C ? dy[m * C + c] : 0.f;
            xh[i] = c < C ? xhat[m * C + c] : 0.f;
            const float d = __fmul_rn(gy[i], gm[i]);      // the product as it is formed below: at C = 1 they cancel exactly
            s1 += d;
            s2 += d * xh[i];
        }
        s1 = wave_sum(s1) / (float)C;
        s2 = wave_sum(s2) / (float)C;
        const float rs = rstd[m];
#pragma unroll
        for (int i = 0; i < LN_REGS; ++i) {
            const int c = lane + 64 * i;
            if (c >= C) continue;
            dz[m * C + c] = rs * (__fmul_rn(gy[i], gm[i]) - s1 - xh[i] * s2);
            pg[i] += gy[i] * xh[i];
            pb[i] += gy[i];
        }
    }
    if (w > 0) {
#pragma unroll
        for (int i = 0; i < LN_REGS; ++i) {
            P[w - 1][0][lane + 64 * i] = pg[i];
            P[w - 1][1][lane + 64 * i] = pb[i];
        }
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int i = 0; i < LN_REGS; ++i) {
            const int c = lane + 64 * i;
            if (c >= C) continue;
            ws[((long long)blockIdx.x * 2 + 0) * C + c] = ((pg[i] + P[0][0][c]) + P[1][0][c]) + P[2][0][c];
            ws[((long long)blockIdx.x * 2 + 1) * C + c] = ((pb[i] + P[0][1][c]) + P[1][1][c]) + P[2][1][c];
        }
    }
}

__global__ __launch_bounds__(256) void wide_ln_bwd_fold_kernel(const float* __restrict__ ws, float* ggamma, float* gbeta, int C, int nblk) {
    const int e = blockIdx.x * 256 + threadIdx.x;           // (which, column)
    if (e >= 2 * C) return;
    const int which = e / C, c = e - which * C;
    float s = 0.f;
    for (int i = 0; i < nblk; ++i) s += ws[((long long)i * 2 + which) * C + c];
    float* dst = which ? gbeta : ggamma;
    if (dst) dst[c] += s;
}

inline int ln_bwd_blocks(long long rows) {
    const long long n = (rows + 3) / 4;
    return n < 256 ? (int)n : 256;
}

// ---------------------------------------------------------------- backward of a Linear
struct GradArgs {
    Operand p;                // dgrad reads the shapes only
    const float* dz;          // [R][N]
    const float* w;           // dgrad: [N][K]
    const float* res;         // dgrad: the gradient arriving along the residual (nullable): + ROWS dx, EDGE de, NODE dv
    const float* mul;         // dgrad, ROWS: [R][K] (nullable); mask == 0: dx *= mul, mask != 0: dx = mul > 0 ? dx : 0
    float *o0, *o1, *o2;      // dgrad outputs (each nullable): EDGE de, d_src, d_dst; NODE d_agg, dv; ROWS dx
    float* ws;                // wgrad: [S][k_pad][n_pad]
    int N, mask, ntiles, S, k_pad, n_pad;
};

// gW0 = A^T . dz: this thread stages operand column c (column K: the constant 1 of the bias, beyond it zero) and dz column col
template <int MODE>
__global__ __launch_bounds__(256) void wide_wgrad0_kernel(const GradArgs a) {
    const int tid = threadIdx.x;
    const int c = blockIdx.x * KC + (tid & 15);
    const int col = blockIdx.y * 64 + (tid & 63);
    const long long ldz = a.N;
    row_wgrad_tiles(
        a.ws, a.ntiles, a.S, a.k_pad, a.n_pad,
        [&](int m) -> float {
            if (m >= a.p.R || c > a.p.K) return 0.f;
            if (c == a.p.K) return 1.f;
            return operand_at<MODE>(a.p, row_src<MODE>(a.p, m), c);
        },
        [&](int m) -> float { return (m < a.p.R && col < a.N) ? a.dz[m * ldz + col] : 0.f; });
}

// dA[R][K] = dz[R][N] . W[N][K], one workgroup per (64 rows, 128 columns), stored in parts
template <int MODE>
__global__ __launch_bounds__(256) void wide_dgrad_kernel(const GradArgs a) {
    constexpr int NS = 8, NC = 128;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * NC;
    const long long ldz = a.N, K = a.p.K;
    const int D0 = a.p.D0, D1 = a.p.D1, D2 = a.p.D2;
    f32x4 acc[NS];
    row_gemm_chunks<NS>(
        a.N, acc,
        [&](int k, bool ok, float (&v)[4]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + (tid >> 4) + 16 * i;
                v[i] = (ok && m < a.p.R) ? a.dz[m * ldz + k] : 0.f;
            }
        },
        [&](int kk, int col, bool ok) -> float {
            const int n = n0 + col;
            return (ok && n < a.p.K) ? a.w[kk * K + n] : 0.f;
        });
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long m = m0 + 16 * w + 4 * g + j;
        if (m >= a.p.R) continue;
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) {
            const int n = n0 + ns * 16 + r;
            if (n >= a.p.K) continue;
            float val = acc[ns][j];
            if constexpr (MODE == ROWS) {
                const long long o = m * K + n;
                if (a.mul) val = a.mask ? (a.mul[o] > 0.f ? val : 0.f) : val * a.mul[o];
                if (a.res) val += a.res[o];
                a.o0[o] = val;
            } else if constexpr (MODE == EDGE) {
                if (n < D0) {
                    if (a.o0) a.o0[m * D0 + n] = val + (a.res ? a.res[m * D0 + n] : 0.f);
                } else if (n < D0 + D1) {
                    if (a.o1) a.o1[m * D1 + (n - D0)] = val;
                } else {
                    if (a.o2) a.o2[m * D2 + (n - D0 - D1)] = val;
                }
            } else {
                if (n < D0) {
                    if (a.o0) a.o0[m * D0 + n] = val;
                } else {
                    if (a.o1) a.o1[m * D1 + (n - D0)] = val + (a.res ? a.res[m * D1 + (n - D0)] : 0.f);
                }
            }
        }
    }
}

// ---------------------------------------------------------------- sums and gathers between the edges and ONE node set
// out[b N + i] = [add] + sum over the CSR list of node i of in rows [/ count]; thread = (node row, column), column fastest
__global__ __launch_bounds__(256) void wide_gather_sum_kernel(const float* __restrict__ in, const int* __restrict__ ptr,
                                                              const int* __restrict__ eid, int mean, const float* __restrict__ add,
                                                              float* __restrict__ out, long long total, int N, int E, int C) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    const long long row = e / C;
    const int b = (int)(row / N), i = (int)(row - (long long)b * N);
    const long long eb = (long long)b * E;
    const int p0 = ptr[i], p1 = ptr[i + 1];
    float s = 0.f;
    for (int j = p0; j < p1; ++j) s += in[(eb + eid[j]) * C + c];
    if (mean && p1 > p0) s = s / (float)(p1 - p0);
    out[e] = add ? add[e] + s : s;
}

// out[b E + k] = [add] + in[b N + dst[k]] [/ in-degree]; thread = (edge row, column)
__global__ __launch_bounds__(256) void wide_edge_gather_kernel(const float* __restrict__ in, const int* __restrict__ dst,
                                                               const int* __restrict__ in_ptr, const float* __restrict__ add,
                                                               float* __restrict__ out, long long total, int N, int E, int C) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    const long long row = e / C;
    const int b = (int)(row / E), k = (int)(row - (long long)b * E);
    const int i = dst[k];
    float s = in[((long long)b * N + i) * C + c];
    if (in_ptr) s = s / (float)(in_ptr[i + 1] - in_ptr[i]);      // the edge itself is one of them: never zero
    out[e] = add ? add[e] + s : s;
}

bool width_ok(int v) { return v >= 1 && v <= MAXW; }

const char* mode_name(int mode) { return mode == ROWS ? "rows" : mode == EDGE ? "edge" : "node"; }

// checks a dlwp_graph_wide_operand's shape and fills the kernels' view of it (pointers included)
int wide_operand(const char* name, const dlwp_graph_wide_operand* q, Operand* p, long long* rows) {
    DLWP_REQUIRE(q, DLWP_E_INVALID, "%s: NULL argument (operand)", name);
    const int mode = q->mode;
    DLWP_REQUIRE(mode == ROWS || mode == EDGE || mode == NODE, DLWP_E_INVALID, "%s: mode %d is none of rows (0), edge (1), node (2)", name, mode);
    DLWP_REQUIRE(width_ok(q->D0), DLWP_E_UNSUPPORTED, "%s: width %d outside 1..%d", name, q->D0, MAXW);
    *p = Operand{};
    p->x = q->x; p->vs = q->vs; p->vd = q->vd; p->src = q->src; p->dst = q->dst;
    p->D0 = q->D0;
    if (mode == ROWS) {
        DLWP_REQUIRE(q->rows > 0, DLWP_E_INVALID, "%s: bad shape (%lld rows)", name, q->rows);
        *rows = q->rows;
    } else if (mode == EDGE) {
        DLWP_REQUIRE(q->B > 0 && q->Ns > 0 && q->Nd > 0 && q->E > 0, DLWP_E_INVALID,
                     "%s: bad shape (B %d, %d source nodes, %d destination nodes, E %d edges)", name, q->B, q->Ns, q->Nd, q->E);
        DLWP_REQUIRE(width_ok(q->D1) && width_ok(q->D2), DLWP_E_UNSUPPORTED, "%s: node width (source %d, destination %d) outside 1..%d",
                     name, q->D1, q->D2, MAXW);
        DLWP_REQUIRE((long long)q->B * q->Ns < ROW_LIMIT && (long long)q->B * q->Nd < ROW_LIMIT, DLWP_E_UNSUPPORTED,
                     "%s: more than 2^31 - 64 rows", name);
        *rows = (long long)q->B * q->E;
        p->Ns = q->Ns; p->Nd = q->Nd; p->E = q->E; p->D1 = q->D1; p->D2 = q->D2;
    } else {
        DLWP_REQUIRE(q->B > 0 && q->Nd > 0, DLWP_E_INVALID, "%s: bad shape (B %d, %d destination nodes)", name, q->B, q->Nd);
        DLWP_REQUIRE(width_ok(q->D1), DLWP_E_UNSUPPORTED, "%s: node width %d outside 1..%d", name, q->D1, MAXW);
        *rows = (long long)q->B * q->Nd;
        p->Nd = q->Nd; p->D1 = q->D1;
    }
    DLWP_REQUIRE(*rows < ROW_LIMIT, DLWP_E_UNSUPPORTED, "%s: more than 2^31 - 64 rows", name);
    p->R = (int)*rows;
    p->K = p->D0 + p->D1 + p->D2;
    return DLWP_OK;
}

int operand_pointers(const char* name, int mode, const Operand& p) {
    DLWP_REQUIRE(p.x, DLWP_E_INVALID, "%s: NULL argument (x)", name);
    DLWP_REQUIRE(mode == ROWS || p.vs, DLWP_E_INVALID, "%s: NULL argument (vs)", name);
    DLWP_REQUIRE(mode != EDGE || (p.vd && p.src && p.dst), DLWP_E_INVALID, "%s: NULL argument (vd, src or dst)", name);
    return DLWP_OK;
}

}  // namespace

extern "C" int dlwp_graph_wide_linear_fwd(const dlwp_graph_wide_operand* op, const float* w, const float* b, const float* res, float* y,
                                          float* der, int N, int act, void* stream_) {
    LinArgs a{};
    long long rows;
    int rc = wide_operand("graph_wide_linear_fwd", op, &a.p, &rows);
    if (rc) return rc;
    DLWP_REQUIRE(width_ok(N), DLWP_E_UNSUPPORTED, "graph_wide_linear_fwd: output width %d outside 1..%d", N, MAXW);
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

#define WIDE_ROWS_C(name)                                                                                                          \
    DLWP_REQUIRE(rows > 0, DLWP_E_INVALID, name ": bad shape (%lld rows)", rows);                                                  \
    DLWP_REQUIRE(rows < ROW_LIMIT, DLWP_E_UNSUPPORTED, name ": more than 2^31 - 64 rows");                                         \
    DLWP_REQUIRE(width_ok(C), DLWP_E_UNSUPPORTED, name ": width %d outside 1..%d", C, MAXW)

extern "C" int dlwp_graph_wide_ln_fwd(const float* z, const float* gamma, const float* beta, const float* res, float* y, float* xhat,
                                      float* rstd, long long rows, int C, float eps, void* stream_) {
    DLWP_REQUIRE(z && gamma && beta && y, DLWP_E_INVALID, "graph_wide_ln_fwd: NULL argument");
    DLWP_REQUIRE((xhat == nullptr) == (rstd == nullptr), DLWP_E_INVALID, "graph_wide_ln_fwd: xhat and rstd go together");
    WIDE_ROWS_C("graph_wide_ln_fwd");
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, 8.0 * rows * C, 4.0 * rows * C * (2.0 + (res ? 1.0 : 0.0) + (xhat ? 1.0 : 0.0)), "graph_wide_ln_fwd");
    hipLaunchKernelGGL(wide_ln_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, z, gamma, beta, res, y, xhat, rstd,
                       (int)rows, C, eps);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" long long dlwp_graph_wide_ln_bwd_ws_floats(long long rows, int C) {
    if (rows <= 0 || rows >= ROW_LIMIT || !width_ok(C)) {
        dlwp_set_error("graph_wide_ln_bwd_ws_floats: bad shape (%lld rows, width %d; widths are 1..%d)", rows, C, MAXW);
        return DLWP_E_INVALID;
    }
    return 2ll * ln_bwd_blocks(rows) * C;
}

extern "C" int dlwp_graph_wide_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dz, float* ws,
                                      float* ggamma, float* gbeta, long long rows, int C, void* stream_) {
    DLWP_REQUIRE(dy && xhat && rstd && gamma && dz && ws, DLWP_E_INVALID, "graph_wide_ln_bwd: NULL argument");
    WIDE_ROWS_C("graph_wide_ln_bwd");
    hipStream_t s = (hipStream_t)stream_;
    const int nblk = ln_bwd_blocks(rows);
    {
        dlwp_prof_scope ps(s, 10.0 * rows * C, 4.0 * 3.0 * rows * C, "graph_wide_ln_bwd");
        hipLaunchKernelGGL(wide_ln_bwd_kernel, dim3(nblk), dim3(256), 0, s, dy, xhat, rstd, gamma, dz, ws, (int)rows, C);
        DLWP_LAUNCH_CHECK();
    }
    {
        dlwp_prof_scope ps(s, 2.0 * nblk * C, 4.0 * 2.0 * (nblk + 2.0) * C, "graph_wide_ln_bwd_fold");
        hipLaunchKernelGGL(wide_ln_bwd_fold_kernel, dim3(ceil_div(2 * C, 256)), dim3(256), 0, s, ws, ggamma, gbeta, C, nblk);
        DLWP_LAUNCH_CHECK();
    }
    return DLWP_OK;
}

extern "C" long long dlwp_graph_wide_wgrad0_ws_floats(const dlwp_graph_wide_operand* op, int N) {
    Operand p;
    long long rows;
    const int rc = wide_operand("graph_wide_wgrad0_ws_floats", op, &p, &rows);
    if (rc) return rc;
    if (!width_ok(N)) {
        dlwp_set_error("graph_wide_wgrad0_ws_floats: output width %d outside 1..%d", N, MAXW);
        return DLWP_E_UNSUPPORTED;
    }
    return row_wgrad_ws_floats(rows, p.K, N);
}

extern "C" int dlwp_graph_wide_wgrad0(const dlwp_graph_wide_operand* op, const float* dz, float* ws, float* gw, float* gb, int N,
                                      void* stream_) {
    GradArgs a{};
    long long rows;
    int rc = wide_operand("graph_wide_wgrad0", op, &a.p, &rows);
    if (rc) return rc;
    DLWP_REQUIRE(width_ok(N), DLWP_E_UNSUPPORTED, "graph_wide_wgrad0: output width %d outside 1..%d", N, MAXW);
    rc = operand_pointers("graph_wide_wgrad0", op->mode, a.p);
    if (rc) return rc;
    DLWP_REQUIRE(dz && ws && gw, DLWP_E_INVALID, "graph_wide_wgrad0: NULL argument (dz, ws or gw)");
    a.dz = dz; a.ws = ws; a.N = N;
    hipStream_t s = (hipStream_t)stream_;
    if (op->mode == ROWS)
        return launch_row_wgrad(wide_wgrad0_kernel<ROWS>, a, rows, a.p.K, N, gw, gb, s, "graph_wide_wgrad0_rows", "graph_wide_wgrad0_fold");
    if (op->mode == EDGE)
        return launch_row_wgrad(wide_wgrad0_kernel<EDGE>, a, rows, a.p.K, N, gw, gb, s, "graph_wide_wgrad0_edge", "graph_wide_wgrad0_fold");
    return launch_row_wgrad(wide_wgrad0_kernel<NODE>, a, rows, a.p.K, N, gw, gb, s, "graph_wide_wgrad0_node", "graph_wide_wgrad0_fold");
}

extern "C" int dlwp_graph_wide_dgrad(const dlwp_graph_wide_operand* op, const float* dz, const float* w, const float* res,
                                     const float* mul, int mask, float* out0, float* out1, float* out2, int N, void* stream_) {
    GradArgs a{};
    long long rows;
    const int rc = wide_operand("graph_wide_dgrad", op, &a.p, &rows);
    if (rc) return rc;
    DLWP_REQUIRE(width_ok(N), DLWP_E_UNSUPPORTED, "graph_wide_dgrad: output width %d outside 1..%d", N, MAXW);
    DLWP_REQUIRE(dz && w, DLWP_E_INVALID, "graph_wide_dgrad: NULL argument (dz or w)");
    DLWP_REQUIRE(op->mode == ROWS ? out0 != nullptr : (out0 || out1 || out2), DLWP_E_INVALID, "graph_wide_dgrad: NULL argument (no output)");
    DLWP_REQUIRE(!mul || op->mode == ROWS, DLWP_E_INVALID, "graph_wide_dgrad: the multiplier goes with the rows mode");
    a.dz = dz; a.w = w; a.res = res; a.mul = mul; a.mask = mask; a.o0 = out0; a.o1 = out1; a.o2 = out2; a.N = N;
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, 2.0 * rows * a.p.K * N, 4.0 * ((double)rows * ((mul ? 2.0 : 1.0) * a.p.K + N) + (double)a.p.K * N),
                       "graph_wide_dgrad_%s", mode_name(op->mode));
    const dim3 grid(ceil_div(a.p.R, TM), ceil_div(a.p.K, 128)), block(256);
    if (op->mode == ROWS) hipLaunchKernelGGL(wide_dgrad_kernel<ROWS>, grid, block, 0, s, a);
    else if (op->mode == EDGE) hipLaunchKernelGGL(wide_dgrad_kernel<EDGE>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(wide_dgrad_kernel<NODE>, grid, block, 0, s, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

#define WIDE_BNEC(name)                                                                                                            \
    DLWP_REQUIRE(B > 0 && N > 0 && E > 0, DLWP_E_INVALID, name ": bad shape (B %d, N %d nodes, E %d edges)", B, N, E);             \
    DLWP_REQUIRE(width_ok(C), DLWP_E_UNSUPPORTED, name ": width %d outside 1..%d", C, MAXW);                                       \
    DLWP_REQUIRE((long long)B * E < ROW_LIMIT && (long long)B * N < ROW_LIMIT, DLWP_E_UNSUPPORTED, name ": more than 2^31 - 64 rows")

extern "C" int dlwp_graph_wide_gather_sum(const float* in, const int* ptr, const int* eid, int mean, const float* add, float* out, int B,
                                          int N, int E, int C, void* stream_) {
    DLWP_REQUIRE(in && ptr && eid && out, DLWP_E_INVALID, "graph_wide_gather_sum: NULL argument");
    WIDE_BNEC("graph_wide_gather_sum");
    const long long total = (long long)B * N * C;
    hipStream_t s = (hipStream_t)stream_;
    const double moved = (double)B * E * C;
    dlwp_prof_scope ps(s, moved, 4.0 * (moved + (add ? 2.0 : 1.0) * total), "graph_wide_gather_sum");
    hipLaunchKernelGGL(wide_gather_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, ptr, eid, mean, add, out, total,
                       N, E, C);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_graph_wide_edge_gather(const float* in, const int* dst, const int* in_ptr, const float* add, float* out, int B, int N,
                                           int E, int C, void* stream_) {
    DLWP_REQUIRE(in && dst && out, DLWP_E_INVALID, "graph_wide_edge_gather: NULL argument");
    WIDE_BNEC("graph_wide_edge_gather");
    const long long total = (long long)B * E * C;
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, (double)total, 4.0 * (add ? 3.0 : 2.0) * total, "graph_wide_edge_gather");
    hipLaunchKernelGGL(wide_edge_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, dst, in_ptr, add, out, total,
                       N, E, C);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}
