// The fused forward of the graph MLPs of the MeshGraphNet / GraphCastNS baselines (widths 1..128): row MLPs whose operand rows are
// assembled through an index while they are staged.  The backward pass is graph_bwd.hip's.  Reference call sites (the three blocks in
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
// dz_{l-1} = (dz_l . W_l) * d_{l-1} (dlwp_graph_dgrad_mul, graph_bwd.hip).
#include "graph_common.hip.h"

namespace {

using namespace rowgemm;      // TM rows per workgroup, KC K values per chunk, AP
using graphc::MAXW;
using graphc::ROWS; using graphc::EDGE; using graphc::NODE; using graphc::RELU; using graphc::SILU;
using graphc::silu; using graphc::width_ok; using graphc::mode_name; using graphc::graph_shape;
constexpr int MAXL = DLWP_GRAPH_MAX_HIDDEN_LAYERS;

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

}  // namespace

extern "C" int dlwp_graph_mlp_fwd(const dlwp_graph_mlp_args* p, void* stream_) {
    DLWP_REQUIRE(p, DLWP_E_INVALID, "graph_mlp_fwd: NULL argument");
    long long rows;
    int K0;
    const int rc = graph_shape("graph_mlp_fwd", p->mode, p->B, p->N, p->E, p->rows, p->De, p->Dv, &rows, &K0);
    if (rc) return rc;
    DLWP_REQUIRE(p->hidden_layers >= 1 && p->hidden_layers <= MAXL, DLWP_E_UNSUPPORTED,
                 "graph_mlp_fwd: %d hidden layers outside 1..%d", p->hidden_layers, MAXL);
    DLWP_REQUIRE(width_ok(p->hidden, MAXW) && width_ok(p->out, MAXW), DLWP_E_UNSUPPORTED, "graph_mlp_fwd: width (hidden %d, output %d) outside 1..%d",
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
