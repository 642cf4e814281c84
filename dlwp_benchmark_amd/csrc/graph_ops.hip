// The graph kernels of the MeshGraphNet baselines: row MLPs whose operand rows are assembled through an index while they are
// staged, and the fixed-order reductions / gathers between edges and nodes.  Reference call sites (the three blocks in
// src/{nsbench,dlwpbench}/models/graphcast/gnn_layers/): MeshGraphMLP.forward (mesh_graph_mlp.py:171-194), MeshEdgeBlock.forward
// (mesh_edge_block.py:86-94: MLP over cat(e, v[src], v[dst]) + e, the concatenation built by concat_efeat_dgl, utils.py:115-150)
// and MeshNodeBlock.forward (mesh_node_block.py:83-93: MLP over cat(sum of incoming e, v) + v, built by agg_concat_dgl,
// utils.py:340-380).
//
// Layout: every activation is fp32 row-major [rows][width].  src, dst and the CSR arrays are int32 arrays of ONE sample's graph
// (N nodes, E edges); sample b's node i is row b N + i, its edge k row b E + k, formed here.  No kernel uses atomics; every launch
// is bit-reproducible.
//
// Forward (graph_mlp_kernel): one workgroup (4 waves) owns 64 rows, wave w the rows 16w..16w+15, and runs the whole chain
// L x (Linear + bias + ReLU), Linear + bias [, LayerNorm] [, + residual] on them.  The first Linear's operand tile [64][16] is
// staged per chunk of 16 K-values in one of three modes,
//   ROWS  A[r] = x[r]
//   EDGE  A[r] = e[r] | v[b N + src[k]] | v[b N + dst[k]]
//   NODE  A[r] = agg[r] | v[r],  agg[r] = sum (or mean) of e[b E + eid] over the in-edges of node r in CSR order
// so cat(...) never exists in memory.  Hidden rows stay in LDS ([64][NS*16 + 4], rewritten in place: a wave reads and writes only
// its own 16 rows); the weight tile [16][NS*16] of each chunk is staged straight from nn.Linear's [out][in] layout, zero-filled
// beyond K and N (nothing in memory is padded).  The chunk loop is row_gemm.hip.h's (row_gemm_chunks) in a copy of this kernel's
// own: its barrier at the top of a chunk also hands Hs from one layer to the next, and from the second layer on the A fragment
// comes from Hs.
// When a backward pass follows the launch also stores the post-activation hidden rows, the normalised rows, 1/sigma and (NODE) agg.
// The activation is a template parameter: ReLU, or SiLU (GraphCast: activation_fn of MeshGraphMLP, graph_cast_net_ns.py:208-246),
// v s with s = 1 / (1 + exp(-v)).  SiLU is not monotone, so its derivative cannot be taken from the stored v s as ReLU's mask is:
// the launch stores d = s (1 + v (1 - s)) as well, and the backward of a later Linear is ONE launch,
// dz_{l-1} = (dz_l . W_l) * d_{l-1} (graph_dgrad0_kernel<ROWS, true>, dlwp_graph_dgrad_mul).
//
// Backward of the FIRST Linear (the others are Linears on stored rows: dlwp_conv1x1_dgrad / _wgrad, ReLU; dlwp_graph_dgrad_mul, SiLU):
// * graph_wgrad0_kernel: gW0 = dz0^T . A with A gathered again exactly as in the forward (NODE reads the stored agg), on
//   row_gemm.hip.h's split-K tile walk and fold (row_wgrad_tiles: INTO gw [hidden][K0] and gb; the bias rides along as operand
//   column K0 = 1);
// * graph_dgrad0_kernel: dA = dz0 . W0 (row_gemm_chunks), split while it is stored: EDGE -> de (+ the residual's dy), per-edge d_src, per-edge d_dst;
//   NODE -> d_agg, dv (+ the residual's dy); ROWS -> dx;
// * graph_gather_sum_kernel: out[b N + i] = [add] + sum over CSR list 1 of in1 rows [/ degree] + sum over CSR list 2 of in2 rows, in
//   list order (dv of an edge block: out-edges of d_src, in-edges of d_dst; also the forward aggregation on its own);
// * graph_edge_gather_kernel: out[b E + k] = [add] + d_agg[b N + dst[k]] [/ in-degree] (de of a node block).
// LayerNorm backward (graph_ln_bwd_kernel) works from the stored normalised rows and 1/sigma; the gamma / beta gradients are
// per-workgroup column sums folded in workgroup order INTO the gradient buffers.
#include "row_gemm.hip.h"

namespace {

using namespace rowgemm;      // TM rows per workgroup, KC K values per chunk, AP
constexpr int MAXW = DLWP_GRAPH_MAX_WIDTH;
constexpr int MAXL = DLWP_GRAPH_MAX_HIDDEN_LAYERS;
constexpr long long ROW_LIMIT = (1ll << 31) - 64;      // the kernels form row indices of a whole last 64-row tile in int

enum { ROWS = DLWP_GRAPH_ROWS, EDGE = DLWP_GRAPH_EDGE, NODE = DLWP_GRAPH_NODE };
enum { RELU = DLWP_GRAPH_ACT_RELU, SILU = DLWP_GRAPH_ACT_SILU };

struct MlpArgs {
    const float *x, *v;
    const int *src, *dst, *in_ptr, *in_eid;
    const float* w[MAXL + 1];
    const float* b[MAXL + 1];
    const float *gamma, *beta;
    float* y;
    float* hid[MAXL];
    float *xhat, *rstd, *agg;
    int R, N, E, De, Dv, K0, hidden, out, L, residual, mean;
    float eps;
    float* der[MAXL];         // SiLU: the derivative rows (behind the fields the ReLU kernels read: their offsets stay)
};

// where the operand row of row m comes from (one per staged row and thread)
struct RowSrc {
    long long o0, o1, o2;     // ROWS: x row.  EDGE: e row, v[src] row, v[dst] row.  NODE: first edge row of the sample, v row (float offsets,
    int p0, p1;               // except NODE o0: a ROW index); NODE: the in-edge range.  o0 < 0: row beyond R
};

template <int MODE>
__device__ __forceinline__ RowSrc row_src(int m, int R, int N, int E, int De, int Dv, int K0, const int* src, const int* dst,
                                          const int* in_ptr) {
    RowSrc s{-1, 0, 0, 0, 0};
    if (m >= R) return s;
    if constexpr (MODE == ROWS) {
        s.o0 = (long long)m * K0;
    } else if constexpr (MODE == EDGE) {
        const int b = m / E, k = m - b * E;
        s.o0 = (long long)m * De;
        s.o1 = ((long long)b * N + src[k]) * Dv;
        s.o2 = ((long long)b * N + dst[k]) * Dv;
    } else {
        const int b = m / N, n = m - b * N;
        s.o0 = (long long)b * E;
        s.o1 = (long long)m * Dv;
        s.p0 = in_ptr[n];
        s.p1 = in_ptr[n + 1];
    }
    return s;
}

// operand element k (< K0) of a row in the forward: NODE forms the aggregate
template <int MODE>
__device__ __forceinline__ float operand_fwd(const RowSrc& s, int k, const float* __restrict__ x, const float* __restrict__ v,
                                             const int* __restrict__ in_eid, int De, int Dv, int mean) {
    if constexpr (MODE == ROWS) {
        return x[s.o0 + k];
    } else if constexpr (MODE == EDGE) {
        return k < De ? x[s.o0 + k] : (k < De + Dv ? v[s.o1 + (k - De)] : v[s.o2 + (k - De - Dv)]);
    } else {
        if (k >= De) return v[s.o1 + (k - De)];
        float sum = 0.f;
        for (int j = s.p0; j < s.p1; ++j) sum += x[(s.o0 + in_eid[j]) * De + k];
        if (mean && s.p1 > s.p0) sum = sum / (float)(s.p1 - s.p0);
        return sum;
    }
}

// SiLU v s and its derivative s (1 + v (1 - s)), s = 1 / (1 + exp(-v)).  Far out exp(-v) is inf or 0, so s is exactly 0 or 1 and the
// pair is (-0, -0) or (v, 1): the division is IEEE's (1 / inf = 0), and no inf meets an inf or a zero
__device__ __forceinline__ float silu(float v, float& d) {
    const float s = 1.0f / (1.0f + __expf(-v));
    d = s * (1.0f + v * (1.0f - s));
    return v * s;
}

template <int MODE, int NS, int ACT>
__global__ __launch_bounds__(256) void graph_mlp_kernel(const MlpArgs a) {
    constexpr int NC = NS * 16;
    constexpr int HP = NC + 4;
    __shared__ float Hs[TM * HP];                 // the rows between two layers
    __shared__ float As[TM * AP];                 // first layer: operand chunk
    __shared__ float Ws[KC * NC];                 // [g][column][4 K values]
    __shared__ float Rs[TM];                      // 1 / sigma
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * TM;
    const int kq = tid & 15, rq = tid >> 4;       // this thread stages K value kq of the rows rq + 16 i

    RowSrc rs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) rs[i] = row_src<MODE>(m0 + rq + 16 * i, a.R, a.N, a.E, a.De, a.Dv, a.K0, a.src, a.dst, a.in_ptr);

    f32x4 acc[NS];
    float av[4], wv[NS];
    for (int l = 0; l <= a.L; ++l) {
        const int K = l == 0 ? a.K0 : a.hidden;
        const int Nl = l == a.L ? a.out : a.hidden;
        const float* __restrict__ wl = a.w[l];
        const float* __restrict__ bl = a.b[l];
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) acc[ns] = f32x4{0.f, 0.f, 0.f, 0.f};
        // chunk kc's tiles, global -> registers (issued one chunk ahead: in flight during the MFMAs)
        auto fetch = [&](int kc) {
            if (l == 0) {
                const int k = kc * KC + kq;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float val = 0.f;
                    if (rs[i].o0 >= 0 && k < a.K0) {
                        val = operand_fwd<MODE>(rs[i], k, a.x, a.v, a.in_eid, a.De, a.Dv, a.mean);
                        if (MODE == NODE && a.agg && k < a.De) a.agg[(long long)(m0 + rq + 16 * i) * a.De + k] = val;
                    }
                    av[i] = val;
                }
            }
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int u = tid + 256 * i;               // Ws index: ((g * NC + column) * 4 + s)
                const int s = u & 3, col = (u >> 2) % NC, gg = (u >> 2) / NC;
                const int kk = kc * KC + 4 * gg + s;
                wv[i] = (kk < K && col < Nl) ? wl[(long long)col * K + kk] : 0.f;
            }
        };
        const int nchunks = (K + KC - 1) / KC;
        fetch(0);
        for (int kc = 0; kc < nchunks; ++kc) {
            __syncthreads();                      // the previous chunk's (and layer's) fragments have been read, Hs is written
            if (l == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) As[(rq + 16 * i) * AP + kq] = av[i];
            }
#pragma unroll
            for (int i = 0; i < NS; ++i) Ws[tid + 256 * i] = wv[i];
            __syncthreads();
            if (kc + 1 < nchunks) fetch(kc + 1);
            const f32x4 af = l == 0 ? *reinterpret_cast<const f32x4*>(&As[(16 * w + r) * AP + 4 * g])
                                    : *reinterpret_cast<const f32x4*>(&Hs[(16 * w + r) * HP + kc * KC + 4 * g]);
#pragma unroll
            for (int ns = 0; ns < NS; ++ns) {
                if (ns * 16 < Nl) {
                    const f32x4 bf = *reinterpret_cast<const f32x4*>(&Ws[(g * NC + ns * 16 + r) * 4]);
                    acc[ns] = mfma16_chunk(af, bf, acc[ns]);
                }
            }
        }
        // lane (r, g) register j holds row 16w + 4g + j, column 16 ns + r.  All NC columns are written (zeros beyond Nl): the next
        // layer's last K chunk reads them
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = 16 * w + 4 * g + j, m = m0 + row;
#pragma unroll
            for (int ns = 0; ns < NS; ++ns) {
                const int n = ns * 16 + r;
                float val = 0.f;
                if (n < Nl) {
                    val = acc[ns][j] + (bl ? bl[n] : 0.f);
                    if (l < a.L) {
                        if constexpr (ACT == RELU) {
                            val = fmaxf(val, 0.f);
                            if (a.hid[l] && m < a.R) a.hid[l][(long long)m * a.hidden + n] = val;
                        } else {
                            float d;
                            val = silu(val, d);
                            if (m < a.R) {
                                if (a.hid[l]) a.hid[l][(long long)m * a.hidden + n] = val;
                                if (a.der[l]) a.der[l][(long long)m * a.hidden + n] = d;
                            }
                        }
                    }
                }
                Hs[row * HP + n] = val;
            }
        }
    }
    __syncthreads();
    const int C = a.out;
    if (a.gamma) {                                // four lanes per row: biased variance, two passes
        const int row = 16 * w + (lane >> 2), q = lane & 3;
        float* h = &Hs[row * HP];
        float s = 0.f;
        for (int c = q; c < C; c += 4) s += h[c];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        const float mean = s / (float)C;
        float vs = 0.f;
        for (int c = q; c < C; c += 4) vs += (h[c] - mean) * (h[c] - mean);
        vs += __shfl_xor(vs, 1);
        vs += __shfl_xor(vs, 2);
        const float rstd = 1.0f / sqrtf(vs / (float)C + a.eps);
        for (int c = q; c < C; c += 4) h[c] = (h[c] - mean) * rstd;
        if (q == 0) Rs[row] = rstd;
        __syncthreads();
    }
    // the 16 rows of a wave are one contiguous block of y
    const float* __restrict__ res = a.residual ? (MODE == NODE ? a.v : a.x) : nullptr;
    for (int idx = lane; idx < 16 * C; idx += 64) {
        const int lr = idx / C, c = idx - lr * C, row = 16 * w + lr, m = m0 + row;
        if (m >= a.R) break;
        float h = Hs[row * HP + c];
        const long long o = (long long)m * C + c;
        if (a.gamma) {
            if (a.xhat) a.xhat[o] = h;
            h = h * a.gamma[c] + a.beta[c];
        }
        if (res) h += res[o];
        a.y[o] = h;
    }
    if (a.gamma && a.rstd && lane < 16 && m0 + 16 * w + lane < a.R) a.rstd[m0 + 16 * w + lane] = Rs[16 * w + lane];
}

template <int MODE, int ACT>
int launch_mlp(const MlpArgs& a, hipStream_t s) {
    const dim3 grid(ceil_div(a.R, TM)), block(256);
    const int wmax = a.hidden > a.out ? a.hidden : a.out;
    if (wmax <= 32) hipLaunchKernelGGL((graph_mlp_kernel<MODE, 2, ACT>), grid, block, 0, s, a);
    else if (wmax <= 64) hipLaunchKernelGGL((graph_mlp_kernel<MODE, 4, ACT>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((graph_mlp_kernel<MODE, 8, ACT>), grid, block, 0, s, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

// ---------------------------------------------------------------- first layer, backward
struct Grad0Args {
    const float *x, *v;       // as the forward's; NODE: x = the stored agg [B N][De]
    const int *src, *dst;
    const float* dz;          // [R][hidden]
    const float* w;           // dgrad: [hidden][K0]
    const float* res;         // dgrad: the residual's dy (nullable), added to the e part (EDGE) / the v part (NODE)
    float *o0, *o1, *o2;      // dgrad outputs (each nullable): EDGE de, d_src, d_dst; NODE d_agg, dv; ROWS dx
    float* ws;                // wgrad: [S][k_pad][n_pad]
    int R, N, E, De, Dv, K0, hidden, ntiles, S, k_pad, n_pad;
    const float* mul;         // dgrad, ROWS with MUL: [R][K0], multiplied into dx as it is stored (nullable)
};

// operand element c of row m as the weight gradient reads it: column K0 is the constant 1 (bias), beyond it zero
template <int MODE>
__device__ __forceinline__ float operand_bwd(const Grad0Args& a, int m, int c) {
    if (c >= a.K0) return c == a.K0 ? 1.f : 0.f;
    if constexpr (MODE == ROWS) {
        return a.x[(long long)m * a.K0 + c];
    } else if constexpr (MODE == EDGE) {
        if (c < a.De) return a.x[(long long)m * a.De + c];
        const int b = m / a.E, k = m - b * a.E;
        if (c < a.De + a.Dv) return a.v[((long long)b * a.N + a.src[k]) * a.Dv + (c - a.De)];
        return a.v[((long long)b * a.N + a.dst[k]) * a.Dv + (c - a.De - a.Dv)];
    } else {
        return c < a.De ? a.x[(long long)m * a.De + c] : a.v[(long long)m * a.Dv + (c - a.De)];
    }
}

// gW0 = A^T . dz: this thread stages operand column c and dz column col
template <int MODE>
__global__ __launch_bounds__(256) void graph_wgrad0_kernel(const Grad0Args a) {
    const int tid = threadIdx.x;
    const int c = blockIdx.x * KC + (tid & 15);
    const int col = blockIdx.y * 64 + (tid & 63);
    row_wgrad_tiles(
        a.ws, a.ntiles, a.S, a.k_pad, a.n_pad,
        [&](int m) -> float { return m < a.R ? operand_bwd<MODE>(a, m, c) : 0.f; },
        [&](int m) -> float { return (m < a.R && col < a.hidden) ? a.dz[(long long)m * a.hidden + col] : 0.f; });
}

// dA[R][K0] = dz[R][hidden] . W0[hidden][K0], one workgroup per (64 rows, 64 columns), stored in parts.  MUL (ROWS only): dx times
// a.mul element by element -- a later Linear's input gradient times the stored derivative of the activation in front of it
template <int MODE, bool MUL = false>
__global__ __launch_bounds__(256) void graph_dgrad0_kernel(const Grad0Args a) {
    static_assert(!MUL || MODE == ROWS, "the multiplier has the layout of dx");
    constexpr int NS = 4, NC = 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * NC;
    const long long ldz = a.hidden;               // 64-bit here, once: widened inside the loader's condition it costs 4 instructions per load
    f32x4 acc[NS];
    row_gemm_chunks<NS>(
        a.hidden, acc,
        [&](int k, bool ok, float (&v)[4]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + (tid >> 4) + 16 * i;
                v[i] = (ok && m < a.R) ? a.dz[m * ldz + k] : 0.f;
            }
        },
        [&](int kk, int col, bool ok) -> float {
            const int n = n0 + col;
            return (ok && n < a.K0) ? a.w[(long long)kk * a.K0 + n] : 0.f;
        });
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long m = m0 + 16 * w + 4 * g + j;
        if (m >= a.R) continue;
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) {
            const int n = n0 + ns * 16 + r;
            if (n >= a.K0) continue;
            const float val = acc[ns][j];
            if constexpr (MODE == ROWS && MUL) {
                a.o0[m * a.K0 + n] = a.mul ? val * a.mul[m * a.K0 + n] : val;
            } else if constexpr (MODE == ROWS) {
                if (a.o0) a.o0[m * a.K0 + n] = val;
            } else if constexpr (MODE == EDGE) {
                if (n < a.De) {
                    if (a.o0) a.o0[m * a.De + n] = val + (a.res ? a.res[m * a.De + n] : 0.f);
                } else if (n < a.De + a.Dv) {
                    if (a.o1) a.o1[m * a.Dv + (n - a.De)] = val;
                } else {
                    if (a.o2) a.o2[m * a.Dv + (n - a.De - a.Dv)] = val;
                }
            } else {
                if (n < a.De) {
                    if (a.o0) a.o0[m * a.De + n] = val;
                } else {
                    if (a.o1) a.o1[m * a.Dv + (n - a.De)] = val + (a.res ? a.res[m * a.Dv + (n - a.De)] : 0.f);
                }
            }
        }
    }
}

// ---------------------------------------------------------------- reductions and gathers between edges and nodes
// thread = (node row, column), column fastest
__global__ __launch_bounds__(256) void graph_gather_sum_kernel(const float* __restrict__ in1, const int* __restrict__ ptr1,
                                                               const int* __restrict__ eid1, int mean1, const float* __restrict__ in2,
                                                               const int* __restrict__ ptr2, const int* __restrict__ eid2,
                                                               const float* __restrict__ add, float* __restrict__ out, long long total,
                                                               int N, int E, int C) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    const long long row = e / C;
    const int b = (int)(row / N), i = (int)(row - (long long)b * N);
    const long long eb = (long long)b * E;
    float s = 0.f;
    const int p0 = ptr1[i], p1 = ptr1[i + 1];
    for (int j = p0; j < p1; ++j) s += in1[(eb + eid1[j]) * C + c];
    if (mean1 && p1 > p0) s = s / (float)(p1 - p0);
    if (in2) {
        float s2 = 0.f;
        for (int j = ptr2[i]; j < ptr2[i + 1]; ++j) s2 += in2[(eb + eid2[j]) * C + c];
        s += s2;
    }
    out[e] = add ? add[e] + s : s;
}

// thread = (edge row, column)
__global__ __launch_bounds__(256) void graph_edge_gather_kernel(const float* __restrict__ in, const int* __restrict__ dst,
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

// ---------------------------------------------------------------- LayerNorm backward from the stored normalised rows
// dz = rstd (dy gamma - mean_c(dy gamma) - xhat mean_c(dy gamma xhat));  ws[blk][0][c] = sum_rows dy xhat,  ws[blk][1][c] = sum_rows dy
__global__ __launch_bounds__(256) void graph_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                           const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                           float* __restrict__ dz, float* __restrict__ ws, int R, int C, int ntiles) {
    __shared__ float S1[TM], S2[TM];
    __shared__ float Pg[MAXW], Pb[MAXW];
    const int tid = threadIdx.x, c = tid & (MAXW - 1), half = tid >> 7;
    const float gc = c < C ? gamma[c] : 0.f;
    float pg = 0.f, pb = 0.f;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int m0 = t * TM;
        {                                         // four lanes per row
            const int row = tid >> 2, q = tid & 3;
            const long long m = m0 + row;
            float s1 = 0.f, s2 = 0.f;
            if (m < R) {
                for (int cc = q; cc < C; cc += 4) {
                    const float d = __fmul_rn(dy[m * C + cc], gamma[cc]);      // the product as phase 2 forms it: at C = 1 they cancel exactly
                    s1 += d;
                    s2 += d * xhat[m * C + cc];
                }
            }
            s1 += __shfl_xor(s1, 1); s1 += __shfl_xor(s1, 2);
            s2 += __shfl_xor(s2, 1); s2 += __shfl_xor(s2, 2);
            if (q == 0) { S1[row] = s1 / (float)C; S2[row] = s2 / (float)C; }
        }
        __syncthreads();
        if (c < C) {
            for (int rr = half * 32; rr < half * 32 + 32; ++rr) {
                const long long m = m0 + rr;
                if (m >= R) break;
                const float gy = dy[m * C + c], xh = xhat[m * C + c];
                dz[m * C + c] = rstd[m] * (__fmul_rn(gy, gc) - S1[rr] - xh * S2[rr]);
                pg += gy * xh;
                pb += gy;
            }
        }
        __syncthreads();
    }
    if (half == 1) { Pg[c] = pg; Pb[c] = pb; }
    __syncthreads();
    if (half == 0 && c < C) {
        ws[((long long)blockIdx.x * 2 + 0) * C + c] = pg + Pg[c];
        ws[((long long)blockIdx.x * 2 + 1) * C + c] = pb + Pb[c];
    }
}

__global__ __launch_bounds__(256) void graph_ln_bwd_fold_kernel(const float* __restrict__ ws, float* ggamma, float* gbeta, int C, int nblk) {
    const int e = blockIdx.x * 256 + threadIdx.x;           // (which, column)
    if (e >= 2 * C) return;
    const int which = e / C, c = e - which * C;
    float s = 0.f;
    for (int i = 0; i < nblk; ++i) s += ws[((long long)i * 2 + which) * C + c];
    float* dst = which ? gbeta : ggamma;
    if (dst) dst[c] += s;
}

inline int ln_bwd_blocks(long long rows) {
    const int ntiles = row_tiles(rows);
    return ntiles < 256 ? ntiles : 256;
}

bool width_ok(int v) { return v >= 1 && v <= MAXW; }

const char* mode_name(int mode) { return mode == ROWS ? "rows" : mode == EDGE ? "edge" : "node"; }

// shape checks shared by the entry points that take (mode, B, N, E, rows, De, Dv): fills rows and K0
int graph_shape(const char* name, int mode, int B, int N, int E, long long rows_in, int De, int Dv, long long* rows, int* K0) {
    DLWP_REQUIRE(mode == ROWS || mode == EDGE || mode == NODE, DLWP_E_INVALID, "%s: mode %d is none of rows (0), edge (1), node (2)", name, mode);
    DLWP_REQUIRE(width_ok(De), DLWP_E_UNSUPPORTED, "%s: width %d outside 1..%d", name, De, MAXW);
    if (mode == ROWS) {
        DLWP_REQUIRE(rows_in > 0, DLWP_E_INVALID, "%s: bad shape (%lld rows)", name, rows_in);
        *rows = rows_in;
        *K0 = De;
    } else {
        DLWP_REQUIRE(B > 0 && N > 0 && E > 0, DLWP_E_INVALID, "%s: bad shape (B %d, N %d nodes, E %d edges)", name, B, N, E);
        DLWP_REQUIRE(width_ok(Dv), DLWP_E_UNSUPPORTED, "%s: node width %d outside 1..%d", name, Dv, MAXW);
        *rows = (long long)B * (mode == EDGE ? E : N);
        *K0 = mode == EDGE ? De + 2 * Dv : De + Dv;
        DLWP_REQUIRE((long long)B * E < ROW_LIMIT && (long long)B * N < ROW_LIMIT, DLWP_E_UNSUPPORTED, "%s: more than 2^31 - 64 rows", name);
    }
    DLWP_REQUIRE(*rows < ROW_LIMIT, DLWP_E_UNSUPPORTED, "%s: more than 2^31 - 64 rows", name);
    return DLWP_OK;
}

}  // namespace

extern "C" int dlwp_graph_mlp_fwd(const dlwp_graph_mlp_args* p, void* stream_) {
    DLWP_REQUIRE(p, DLWP_E_INVALID, "graph_mlp_fwd: NULL argument");
    long long rows;
    int K0;
    const int rc = graph_shape("graph_mlp_fwd", p->mode, p->B, p->N, p->E, p->rows, p->De, p->Dv, &rows, &K0);
    if (rc) return rc;
    DLWP_REQUIRE(p->hidden_layers >= 1 && p->hidden_layers <= MAXL, DLWP_E_UNSUPPORTED,
                 "graph_mlp_fwd: %d hidden layers outside 1..%d", p->hidden_layers, MAXL);
    DLWP_REQUIRE(width_ok(p->hidden) && width_ok(p->out), DLWP_E_UNSUPPORTED, "graph_mlp_fwd: width (hidden %d, output %d) outside 1..%d",
                 p->hidden, p->out, MAXW);
    DLWP_REQUIRE(p->x && p->y, DLWP_E_INVALID, "graph_mlp_fwd: NULL argument (x or y)");
    DLWP_REQUIRE(p->mode == ROWS || p->v, DLWP_E_INVALID, "graph_mlp_fwd: NULL argument (v)");
    DLWP_REQUIRE(p->mode != EDGE || (p->src && p->dst), DLWP_E_INVALID, "graph_mlp_fwd: NULL argument (src or dst)");
    DLWP_REQUIRE(p->mode != NODE || (p->in_ptr && p->in_eid), DLWP_E_INVALID, "graph_mlp_fwd: NULL argument (in_ptr or in_eid)");
    for (int l = 0; l <= p->hidden_layers; ++l) DLWP_REQUIRE(p->w[l], DLWP_E_INVALID, "graph_mlp_fwd: NULL argument (weight %d)", l);
    DLWP_REQUIRE((p->gamma == nullptr) == (p->beta == nullptr), DLWP_E_INVALID, "graph_mlp_fwd: gamma and beta go together");
    DLWP_REQUIRE(p->act == RELU || p->act == SILU, DLWP_E_INVALID, "graph_mlp_fwd: act %d is neither relu (0) nor silu (1)", p->act);
    for (int l = 0; l < MAXL; ++l)
        DLWP_REQUIRE(!p->der[l] || (p->act == SILU && l < p->hidden_layers), DLWP_E_INVALID,
                     "graph_mlp_fwd: derivative rows %d given, but they are stored for the hidden layers of a silu chain only", l);
    if (p->residual) {
        DLWP_REQUIRE(p->mode != ROWS, DLWP_E_INVALID, "graph_mlp_fwd: a residual needs the edge or the node mode");
        DLWP_REQUIRE(p->out == (p->mode == EDGE ? p->De : p->Dv), DLWP_E_INVALID,
                     "graph_mlp_fwd: the residual has width %d, the output %d", p->mode == EDGE ? p->De : p->Dv, p->out);
    }
    MlpArgs a{};
    a.x = p->x; a.v = p->v; a.src = p->src; a.dst = p->dst; a.in_ptr = p->in_ptr; a.in_eid = p->in_eid;
    for (int l = 0; l <= p->hidden_layers; ++l) { a.w[l] = p->w[l]; a.b[l] = p->b[l]; }
    for (int l = 0; l < p->hidden_layers; ++l) { a.hid[l] = p->hid[l]; a.der[l] = p->der[l]; }
    a.gamma = p->gamma; a.beta = p->beta; a.eps = p->eps; a.y = p->y;
    a.xhat = p->xhat; a.rstd = p->rstd; a.agg = p->mode == NODE ? p->agg : nullptr;
    a.R = (int)rows; a.N = p->N; a.E = p->E; a.De = p->De; a.Dv = p->Dv; a.K0 = K0; a.hidden = p->hidden; a.out = p->out;
    a.L = p->hidden_layers; a.residual = p->residual; a.mean = p->mean;
    hipStream_t s = (hipStream_t)stream_;
    const double macs = (double)K0 * a.hidden + (a.L - 1.0) * a.hidden * a.hidden + (double)a.hidden * a.out;
    double bytes = 4.0 * rows * ((double)K0 + a.out + (a.residual ? a.out : 0)) + 4.0 * macs;
    if (a.hid[0]) bytes += 4.0 * rows * a.L * a.hidden;
    if (a.der[0]) bytes += 4.0 * rows * a.L * a.hidden;
    if (a.xhat) bytes += 4.0 * rows * a.out;
    dlwp_prof_scope ps(s, 2.0 * rows * macs, bytes, "graph_mlp_%s", mode_name(p->mode));
    if (p->act == SILU) {
        if (p->mode == ROWS) return launch_mlp<ROWS, SILU>(a, s);
        if (p->mode == EDGE) return launch_mlp<EDGE, SILU>(a, s);
        return launch_mlp<NODE, SILU>(a, s);
    }
    if (p->mode == ROWS) return launch_mlp<ROWS, RELU>(a, s);
    if (p->mode == EDGE) return launch_mlp<EDGE, RELU>(a, s);
    return launch_mlp<NODE, RELU>(a, s);
}

#define GRAD0_PROLOGUE(name)                                                                                                       \
    long long rows;                                                                                                                \
    int K0;                                                                                                                        \
    const int rc = graph_shape(name, mode, B, N, E, rows_in, De, Dv, &rows, &K0);                                                  \
    if (rc) return rc;                                                                                                             \
    DLWP_REQUIRE(width_ok(hidden), DLWP_E_UNSUPPORTED, name ": hidden width %d outside 1..%d", hidden, MAXW)

extern "C" long long dlwp_graph_wgrad0_ws_floats(long long rows, int K0, int hidden) {
    if (rows <= 0 || rows >= ROW_LIMIT || K0 < 1 || K0 > 3 * MAXW || !width_ok(hidden)) {
        dlwp_set_error("graph_wgrad0_ws_floats: bad shape (%lld rows, operand width %d, hidden %d)", rows, K0, hidden);
        return DLWP_E_INVALID;
    }
    return row_wgrad_ws_floats(rows, K0, hidden);
}

extern "C" int dlwp_graph_wgrad0(int mode, const float* x, const float* v, const int* src, const int* dst, const float* dz, float* ws,
                                 float* gw, float* gb, int B, int N, int E, long long rows_in, int De, int Dv, int hidden,
                                 void* stream_) {
    GRAD0_PROLOGUE("graph_wgrad0");
    DLWP_REQUIRE(x && dz && ws && gw, DLWP_E_INVALID, "graph_wgrad0: NULL argument");
    DLWP_REQUIRE(mode == ROWS || v, DLWP_E_INVALID, "graph_wgrad0: NULL argument (v)");
    DLWP_REQUIRE(mode != EDGE || (src && dst), DLWP_E_INVALID, "graph_wgrad0: NULL argument (src or dst)");
    Grad0Args a{};
    a.x = x; a.v = v; a.src = src; a.dst = dst; a.dz = dz; a.ws = ws;
    a.R = (int)rows; a.N = N; a.E = E; a.De = De; a.Dv = Dv; a.K0 = K0; a.hidden = hidden;
    hipStream_t s = (hipStream_t)stream_;
    if (mode == ROWS) return launch_row_wgrad(graph_wgrad0_kernel<ROWS>, a, rows, K0, hidden, gw, gb, s, "graph_wgrad0_rows", "graph_wgrad0_fold");
    if (mode == EDGE) return launch_row_wgrad(graph_wgrad0_kernel<EDGE>, a, rows, K0, hidden, gw, gb, s, "graph_wgrad0_edge", "graph_wgrad0_fold");
    return launch_row_wgrad(graph_wgrad0_kernel<NODE>, a, rows, K0, hidden, gw, gb, s, "graph_wgrad0_node", "graph_wgrad0_fold");
}

extern "C" int dlwp_graph_dgrad0(int mode, const float* dz, const float* w, const float* res, float* out0, float* out1, float* out2,
                                 int B, int N, int E, long long rows_in, int De, int Dv, int hidden, void* stream_) {
    GRAD0_PROLOGUE("graph_dgrad0");
    DLWP_REQUIRE(dz && w, DLWP_E_INVALID, "graph_dgrad0: NULL argument");
    DLWP_REQUIRE(out0 || out1 || out2, DLWP_E_INVALID, "graph_dgrad0: NULL argument (no output)");
    Grad0Args a{};
    a.dz = dz; a.w = w; a.res = res; a.o0 = out0; a.o1 = out1; a.o2 = out2;
    a.R = (int)rows; a.N = N; a.E = E; a.De = De; a.Dv = Dv; a.K0 = K0; a.hidden = hidden;
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, 2.0 * rows * K0 * hidden, 4.0 * ((double)rows * (K0 + hidden) + (double)K0 * hidden), "graph_dgrad0_%s",
                       mode_name(mode));
    const dim3 grid(ceil_div((int)rows, TM), ceil_div(K0, 64)), block(256);
    if (mode == ROWS) hipLaunchKernelGGL(graph_dgrad0_kernel<ROWS>, grid, block, 0, s, a);
    else if (mode == EDGE) hipLaunchKernelGGL(graph_dgrad0_kernel<EDGE>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(graph_dgrad0_kernel<NODE>, grid, block, 0, s, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_graph_dgrad_mul(const float* dz, const float* w, const float* mul, float* out, long long rows, int in, int out_width,
                                    void* stream_) {
    DLWP_REQUIRE(dz && w && out, DLWP_E_INVALID, "graph_dgrad_mul: NULL argument");
    DLWP_REQUIRE(rows > 0, DLWP_E_INVALID, "graph_dgrad_mul: bad shape (%lld rows)", rows);
    DLWP_REQUIRE(rows < ROW_LIMIT, DLWP_E_UNSUPPORTED, "graph_dgrad_mul: more than 2^31 - 64 rows");
    DLWP_REQUIRE(width_ok(in) && width_ok(out_width), DLWP_E_UNSUPPORTED, "graph_dgrad_mul: width (input %d, output %d) outside 1..%d", in,
                 out_width, MAXW);
    Grad0Args a{};
    a.dz = dz; a.w = w; a.mul = mul; a.o0 = out;
    a.R = (int)rows; a.K0 = in; a.hidden = out_width;
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, 2.0 * rows * in * out_width,
                       4.0 * ((double)rows * ((mul ? 2.0 : 1.0) * in + out_width) + (double)in * out_width), "graph_dgrad_mul");
    hipLaunchKernelGGL((graph_dgrad0_kernel<ROWS, true>), dim3(ceil_div((int)rows, TM), ceil_div(in, 64)), dim3(256), 0, s, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

#define GRAPH_BNEC(name)                                                                                                           \
    DLWP_REQUIRE(B > 0 && N > 0 && E > 0, DLWP_E_INVALID, name ": bad shape (B %d, N %d nodes, E %d edges)", B, N, E);             \
    DLWP_REQUIRE(width_ok(C), DLWP_E_UNSUPPORTED, name ": width %d outside 1..%d", C, MAXW);                                       \
    DLWP_REQUIRE((long long)B * E < ROW_LIMIT && (long long)B * N < ROW_LIMIT, DLWP_E_UNSUPPORTED, name ": more than 2^31 - 64 rows")

extern "C" int dlwp_graph_gather_sum(const float* in1, const int* ptr1, const int* eid1, int mean1, const float* in2, const int* ptr2,
                                     const int* eid2, const float* add, float* out, int B, int N, int E, int C, void* stream_) {
    DLWP_REQUIRE(in1 && ptr1 && eid1 && out, DLWP_E_INVALID, "graph_gather_sum: NULL argument");
    DLWP_REQUIRE(!in2 || (ptr2 && eid2), DLWP_E_INVALID, "graph_gather_sum: NULL argument (second list)");
    GRAPH_BNEC("graph_gather_sum");
    const long long total = (long long)B * N * C;
    hipStream_t s = (hipStream_t)stream_;
    const double moved = (double)B * E * C * (in2 ? 2.0 : 1.0);
    dlwp_prof_scope ps(s, moved, 4.0 * (moved + (add ? 2.0 : 1.0) * total), "graph_gather_sum");
    hipLaunchKernelGGL(graph_gather_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in1, ptr1, eid1, mean1, in2, ptr2,
                       eid2, add, out, total, N, E, C);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_graph_edge_gather(const float* in, const int* dst, const int* in_ptr, const float* add, float* out, int B, int N,
                                      int E, int C, void* stream_) {
    DLWP_REQUIRE(in && dst && out, DLWP_E_INVALID, "graph_edge_gather: NULL argument");
    GRAPH_BNEC("graph_edge_gather");
    const long long total = (long long)B * E * C;
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, (double)total, 4.0 * (add ? 3.0 : 2.0) * total, "graph_edge_gather");
    hipLaunchKernelGGL(graph_edge_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, dst, in_ptr, add, out, total,
                       N, E, C);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" long long dlwp_graph_ln_bwd_ws_floats(long long rows, int C) {
    if (rows <= 0 || rows >= ROW_LIMIT || !width_ok(C)) {
        dlwp_set_error("graph_ln_bwd_ws_floats: bad shape (%lld rows, width %d; widths are 1..%d)", rows, C, MAXW);
        return DLWP_E_INVALID;
    }
    return 2ll * ln_bwd_blocks(rows) * C;
}

extern "C" int dlwp_graph_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dz, float* ws,
                                 float* ggamma, float* gbeta, long long rows, int C, void* stream_) {
    DLWP_REQUIRE(dy && xhat && rstd && gamma && dz && ws, DLWP_E_INVALID, "graph_ln_bwd: NULL argument");
    DLWP_REQUIRE(rows > 0, DLWP_E_INVALID, "graph_ln_bwd: bad shape (%lld rows)", rows);
    DLWP_REQUIRE(rows < ROW_LIMIT, DLWP_E_UNSUPPORTED, "graph_ln_bwd: more than 2^31 - 64 rows");
    DLWP_REQUIRE(width_ok(C), DLWP_E_UNSUPPORTED, "graph_ln_bwd: width %d outside 1..%d", C, MAXW);
    hipStream_t s = (hipStream_t)stream_;
    const int nblk = ln_bwd_blocks(rows);
    {
        dlwp_prof_scope ps(s, 10.0 * rows * C, 4.0 * 3.0 * rows * C, "graph_ln_bwd");
        hipLaunchKernelGGL(graph_ln_bwd_kernel, dim3(nblk), dim3(256), 0, s, dy, xhat, rstd, gamma, dz, ws, (int)rows, C,
                           row_tiles(rows));
        DLWP_LAUNCH_CHECK();
    }
    {
        dlwp_prof_scope ps(s, 2.0 * nblk * C, 4.0 * 2.0 * (nblk + 2.0) * C, "graph_ln_bwd_fold");
        hipLaunchKernelGGL(graph_ln_bwd_fold_kernel, dim3(ceil_div(2 * C, 256)), dim3(256), 0, s, ws, ggamma, gbeta, C, nblk);
        DLWP_LAUNCH_CHECK();
    }
    return DLWP_OK;
}
