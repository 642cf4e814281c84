// The backward pass of the graph MLPs, ONE kernel set for both families: the fused 1..128 family of graph_ops.hip (dlwp_graph_*:
// one node set, widths to 128) and the wide, bipartite family of graph_wide.hip (dlwp_graph_wide_*: Ns sources, Nd destinations,
// widths to 512).  The fused family is the case Ns == Nd, vs == vd, D1 == D2 of the operand view (graph_common.hip.h: Operand).
// No kernel here has a width limit of its own: the limits, the error texts and the accounting names belong
// to the entry points below, which are thin adapters onto
// * graph_wgrad0_kernel<MODE>: gW0 = dz0^T . A of a FIRST Linear with A gathered again exactly as in the forward (NODE reads the
//   stored agg), on row_gemm.hip.h's split-K tile walk and fold (row_wgrad_tiles: INTO gw [N][K] and gb; the bias rides along as
//   operand column K = 1).  Later Linears read stored rows: dlwp_conv1x1_wgrad takes them at any width;
// * graph_dgrad_kernel<MODE, NS>: dA = dz . W (row_gemm_chunks<NS>: 64 rows x NS*16 columns per workgroup; NS 4 for the fused
//   family, 8 for the wide one), split while it is stored: EDGE -> de (+ the residual's dy), per-edge d_src, per-edge d_dst; NODE ->
//   d_agg, dv (+ the residual's dy); ROWS -> dx, times a multiplier (SiLU's stored derivative rows) or ReLU's mask of the stored
//   post-activation rows, + the residual's dy: the backward of a LATER Linear, (dz . W) * d, in one launch.  How much of that the
//   ROWS epilogue can do is a third template parameter (dlwp_graph_dgrad0: nothing, dlwp_graph_dgrad_mul: the multiplier,
//   dlwp_graph_wide_dgrad: all of it);
// * graph_gather_sum_kernel: out[b N + i] = [add] + sum over CSR list 1 of in1 rows [/ degree] [+ sum over CSR list 2 of in2 rows],
//   in list order (the forward aggregation on its own; dv of an edge block: out-edges of d_src and in-edges of d_dst, in one launch
//   on one node set, in two on two);
// * graph_edge_gather_kernel: out[b E + k] = [add] + d_agg[b N + dst[k]] [/ in-degree] (de of a node block);
// * LayerNorm backward from the stored normalised rows and 1/sigma, two main kernels with summation orders of their own --
//   graph_ln_bwd_kernel (fused family: 64-row tiles, four lanes per row) and wide_ln_bwd_kernel (one wave per row) -- and ONE
//   graph_ln_bwd_fold_kernel: the gamma / beta gradients are per-workgroup column sums folded in workgroup order INTO the buffers.
// No kernel uses atomics; every launch is bit-reproducible, and each output element is formed by the same additions in the same
// order whichever family's entry point launched the kernel.
#include "graph_common.hip.h"

namespace {

using namespace rowgemm;      // TM rows per workgroup, KC K values per chunk
using namespace graphc;

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

// operand element c (< K) of row m for a thread that keeps its column and walks the rows (row_src / operand_at keep the row and
// walk the columns).  Which part holds column c -- and with it the node rows, the index array and the widths -- does not change
// from row to row, so an EDGE element is ONE chain index -> node row whichever side it is on
template <int MODE>
__device__ __forceinline__ float operand_col(const Operand& p, int m, int c) {
    if (MODE == ROWS || c < p.D0) return p.x[(long long)m * p.D0 + c];
    if constexpr (MODE == EDGE) {
        const bool s = c < p.D0 + p.D1;           // the source side
        const float* v = s ? p.vs : p.vd;
        const int* idx = s ? p.src : p.dst;
        const int n = s ? p.Ns : p.Nd, d = s ? p.D1 : p.D2, off = s ? c - p.D0 : c - p.D0 - p.D1;
        const int b = m / p.E, k = m - b * p.E;
        return v[((long long)b * n + idx[k]) * d + off];
    } else {
        return p.vs[(long long)m * p.D1 + (c - p.D0)];
    }
}

// gW0 = A^T . dz: this thread stages operand column c (column K: the constant 1 of the bias, beyond it zero) and dz column col
template <int MODE>
__global__ __launch_bounds__(256) void graph_wgrad0_kernel(const GradArgs a) {
    const int tid = threadIdx.x;
    const int c = blockIdx.x * KC + (tid & 15);
    const int col = blockIdx.y * 64 + (tid & 63);
    const long long ldz = a.N;
    row_wgrad_tiles(
        a.ws, a.ntiles, a.S, a.k_pad, a.n_pad,
        [&](int m) -> float {
            if (m >= a.p.R || c > a.p.K) return 0.f;
            if (c == a.p.K) return 1.f;
            return operand_col<MODE>(a.p, m, c);
        },
        [&](int m) -> float { return (m < a.p.R && col < a.N) ? a.dz[m * ldz + col] : 0.f; });
}

// what the ROWS epilogue may be asked for.  A template parameter, not a run-time choice: on the small launches of the fused family
// the tests and loads of the full form cost 10 - 16 % of the kernel's time
enum { STORE = 0,             // dx = dA
       TIMES = 1,             // dx = dA * mul (mul nullable)
       FULL = 2 };            // dx = dA * mul or masked by mul > 0 (mul nullable), + res (nullable)

// dA[R][K] = dz[R][N] . W[N][K], one workgroup per (64 rows, NS*16 columns), stored in parts.  ROWS writes o0 unconditionally
template <int MODE, int NS, int EPI = STORE>
__global__ __launch_bounds__(256) void graph_dgrad_kernel(const GradArgs a) {
    static_assert(EPI == STORE || MODE == ROWS, "the multiplier and the mask have the layout of dx");
    constexpr int NC = NS * 16;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * NC;
    const long long ldz = a.N, K = a.p.K;         // 64-bit here, once: widened inside a loader's condition it costs 4 instructions per load
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
                if constexpr (EPI == TIMES) {
                    if (a.mul) val = val * a.mul[o];
                } else if constexpr (EPI == FULL) {
                    if (a.mul) val = a.mask ? (a.mul[o] > 0.f ? val : 0.f) : val * a.mul[o];
                    if (a.res) val += a.res[o];
                }
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

template <int NS, int EPI>
void launch_dgrad(int mode, const GradArgs& a, hipStream_t s) {
    const dim3 grid(ceil_div(a.p.R, TM), ceil_div(a.p.K, NS * 16)), block(256);
    if (mode == ROWS) hipLaunchKernelGGL((graph_dgrad_kernel<ROWS, NS, EPI>), grid, block, 0, s, a);
    else if (mode == EDGE) hipLaunchKernelGGL((graph_dgrad_kernel<EDGE, NS>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((graph_dgrad_kernel<NODE, NS>), grid, block, 0, s, a);
}

int launch_wgrad0(int mode, GradArgs& a, long long rows, float* gw, float* gb, hipStream_t s, const char* const names[3],
                  const char* fold_name) {
    if (mode == ROWS) return launch_row_wgrad(graph_wgrad0_kernel<ROWS>, a, rows, a.p.K, a.N, gw, gb, s, names[ROWS], fold_name);
    if (mode == EDGE) return launch_row_wgrad(graph_wgrad0_kernel<EDGE>, a, rows, a.p.K, a.N, gw, gb, s, names[EDGE], fold_name);
    return launch_row_wgrad(graph_wgrad0_kernel<NODE>, a, rows, a.p.K, a.N, gw, gb, s, names[NODE], fold_name);
}

// ---------------------------------------------------------------- reductions and gathers between the edges and one node set
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

int launch_gather_sum(const char* name, const float* in1, const int* ptr1, const int* eid1, int mean1, const float* in2,
                      const int* ptr2, const int* eid2, const float* add, float* out, int B, int N, int E, int C, int maxw,
                      hipStream_t s) {
    const int rc = check_bnec(name, B, N, E, C, maxw);
    if (rc) return rc;
    const long long total = (long long)B * N * C;
    const double moved = (double)B * E * C * (in2 ? 2.0 : 1.0);
    dlwp_prof_scope ps(s, moved, 4.0 * (moved + (add ? 2.0 : 1.0) * total), "%s", name);
    hipLaunchKernelGGL(graph_gather_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in1, ptr1, eid1, mean1, in2, ptr2,
                       eid2, add, out, total, N, E, C);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

int launch_edge_gather(const char* name, const float* in, const int* dst, const int* in_ptr, const float* add, float* out, int B, int N,
                       int E, int C, int maxw, hipStream_t s) {
    DLWP_REQUIRE(in && dst && out, DLWP_E_INVALID, "%s: NULL argument", name);
    const int rc = check_bnec(name, B, N, E, C, maxw);
    if (rc) return rc;
    const long long total = (long long)B * E * C;
    dlwp_prof_scope ps(s, (double)total, 4.0 * (add ? 3.0 : 2.0) * total, "%s", name);
    hipLaunchKernelGGL(graph_edge_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, dst, in_ptr, add, out, total,
                       N, E, C);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

// ---------------------------------------------------------------- LayerNorm backward from the stored normalised rows
// dz = rstd (dy gamma - mean_c(dy gamma) - xhat mean_c(dy gamma xhat));  ws[blk][0][c] = sum_rows dy xhat,  ws[blk][1][c] = sum_rows dy
// The fused family's: 64-row tiles, four lanes per row
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

// The wide family's: one wave per row; the column sums are per lane over a workgroup's rows, then folded over its four waves
__global__ __launch_bounds__(256) void wide_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                          const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                          float* __restrict__ dz, float* __restrict__ ws, int R, int C) {
    __shared__ float P[3][2][WIDE_MAXW];          // the column sums of waves 1..3
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

__global__ __launch_bounds__(256) void graph_ln_bwd_fold_kernel(const float* __restrict__ ws, float* ggamma, float* gbeta, int C, int nblk) {
    const int e = blockIdx.x * 256 + threadIdx.x;           // (which, column)
    if (e >= 2 * C) return;
    const int which = e / C, c = e - which * C;
    float s = 0.f;
    for (int i = 0; i < nblk; ++i) s += ws[((long long)i * 2 + which) * C + c];
    float* dst = which ? gbeta : ggamma;
    if (dst) dst[c] += s;
}

// workgroups of the main kernel = partial rows of the fold: at most 256, over 64-row tiles (fused) or 4 rows each (wide)
inline int ln_bwd_blocks(long long rows, bool wide) {
    const long long n = wide ? (rows + 3) / 4 : row_tiles(rows);
    return n < 256 ? (int)n : 256;
}

long long ln_bwd_ws_floats(const char* name, long long rows, int C, bool wide) {
    const int maxw = wide ? WIDE_MAXW : MAXW;
    if (rows <= 0 || rows >= ROW_LIMIT || !width_ok(C, maxw)) {
        dlwp_set_error("%s: bad shape (%lld rows, width %d; widths are 1..%d)", name, rows, C, maxw);
        return DLWP_E_INVALID;
    }
    return 2ll * ln_bwd_blocks(rows, wide) * C;
}

int launch_ln_bwd(const char* name, const char* fold_name, const float* dy, const float* xhat, const float* rstd, const float* gamma,
                  float* dz, float* ws, float* ggamma, float* gbeta, long long rows, int C, bool wide, hipStream_t s) {
    DLWP_REQUIRE(dy && xhat && rstd && gamma && dz && ws, DLWP_E_INVALID, "%s: NULL argument", name);
    const int rc = check_rows_c(name, rows, C, wide ? WIDE_MAXW : MAXW);
    if (rc) return rc;
    const int nblk = ln_bwd_blocks(rows, wide);
    {
        dlwp_prof_scope ps(s, 10.0 * rows * C, 4.0 * 3.0 * rows * C, "%s", name);
        if (wide) hipLaunchKernelGGL(wide_ln_bwd_kernel, dim3(nblk), dim3(256), 0, s, dy, xhat, rstd, gamma, dz, ws, (int)rows, C);
        else hipLaunchKernelGGL(graph_ln_bwd_kernel, dim3(nblk), dim3(256), 0, s, dy, xhat, rstd, gamma, dz, ws, (int)rows, C, row_tiles(rows));
        DLWP_LAUNCH_CHECK();
    }
    {
        dlwp_prof_scope ps(s, 2.0 * nblk * C, 4.0 * 2.0 * (nblk + 2.0) * C, "%s", fold_name);
        hipLaunchKernelGGL(graph_ln_bwd_fold_kernel, dim3(ceil_div(2 * C, 256)), dim3(256), 0, s, ws, ggamma, gbeta, C, nblk);
        DLWP_LAUNCH_CHECK();
    }
    return DLWP_OK;
}

const char* const WGRAD0_NAMES[3] = {"graph_wgrad0_rows", "graph_wgrad0_edge", "graph_wgrad0_node"};
const char* const WIDE_WGRAD0_NAMES[3] = {"graph_wide_wgrad0_rows", "graph_wide_wgrad0_edge", "graph_wide_wgrad0_node"};

// the fused family's (mode, B, N, E, rows, De, Dv, hidden) as the shared argument struct: one node set, so Ns = Nd = N, D1 = D2 = Dv
int grad0_args(const char* name, int mode, int B, int N, int E, long long rows_in, int De, int Dv, int hidden, GradArgs* a, long long* rows) {
    int K0;
    const int rc = graph_shape(name, mode, B, N, E, rows_in, De, Dv, rows, &K0);
    if (rc) return rc;
    DLWP_REQUIRE(width_ok(hidden, MAXW), DLWP_E_UNSUPPORTED, "%s: hidden width %d outside 1..%d", name, hidden, MAXW);
    *a = GradArgs{};
    a->p.R = (int)*rows; a->p.D0 = De; a->p.K = K0; a->N = hidden;
    if (mode != ROWS) { a->p.Ns = a->p.Nd = N; a->p.E = E; a->p.D1 = Dv; }
    if (mode == EDGE) a->p.D2 = Dv;
    return DLWP_OK;
}

}  // namespace

// ---------------------------------------------------------------- the fused family, widths 1..128
extern "C" long long dlwp_graph_wgrad0_ws_floats(long long rows, int K0, int hidden) {
    if (rows <= 0 || rows >= ROW_LIMIT || K0 < 1 || K0 > 3 * MAXW || !width_ok(hidden, MAXW)) {
        dlwp_set_error("graph_wgrad0_ws_floats: bad shape (%lld rows, operand width %d, hidden %d)", rows, K0, hidden);
        return DLWP_E_INVALID;
    }
    return row_wgrad_ws_floats(rows, K0, hidden);
}

extern "C" int dlwp_graph_wgrad0(int mode, const float* x, const float* v, const int* src, const int* dst, const float* dz, float* ws,
                                 float* gw, float* gb, int B, int N, int E, long long rows_in, int De, int Dv, int hidden,
                                 void* stream_) {
    GradArgs a;
    long long rows;
    const int rc = grad0_args("graph_wgrad0", mode, B, N, E, rows_in, De, Dv, hidden, &a, &rows);
    if (rc) return rc;
    DLWP_REQUIRE(x && dz && ws && gw, DLWP_E_INVALID, "graph_wgrad0: NULL argument");
    DLWP_REQUIRE(mode == ROWS || v, DLWP_E_INVALID, "graph_wgrad0: NULL argument (v)");
    DLWP_REQUIRE(mode != EDGE || (src && dst), DLWP_E_INVALID, "graph_wgrad0: NULL argument (src or dst)");
    a.p.x = x; a.p.vs = v; a.p.vd = v; a.p.src = src; a.p.dst = dst; a.dz = dz; a.ws = ws;
    return launch_wgrad0(mode, a, rows, gw, gb, (hipStream_t)stream_, WGRAD0_NAMES, "graph_wgrad0_fold");
}

extern "C" int dlwp_graph_dgrad0(int mode, const float* dz, const float* w, const float* res, float* out0, float* out1, float* out2,
                                 int B, int N, int E, long long rows_in, int De, int Dv, int hidden, void* stream_) {
    GradArgs a;
    long long rows;
    const int rc = grad0_args("graph_dgrad0", mode, B, N, E, rows_in, De, Dv, hidden, &a, &rows);
    if (rc) return rc;
    DLWP_REQUIRE(dz && w, DLWP_E_INVALID, "graph_dgrad0: NULL argument");
    DLWP_REQUIRE(out0 || out1 || out2, DLWP_E_INVALID, "graph_dgrad0: NULL argument (no output)");
    if (mode == ROWS && !out0) return DLWP_OK;    // every part is optional, and plain rows have only this one
    a.dz = dz; a.w = w; a.res = res; a.o0 = out0; a.o1 = out1; a.o2 = out2;      // on plain rows res is not read: STORE
    hipStream_t s = (hipStream_t)stream_;
    const int K0 = a.p.K;
    dlwp_prof_scope ps(s, 2.0 * rows * K0 * hidden, 4.0 * ((double)rows * (K0 + hidden) + (double)K0 * hidden), "graph_dgrad0_%s",
                       mode_name(mode));
    launch_dgrad<4, STORE>(mode, a, s);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_graph_dgrad_mul(const float* dz, const float* w, const float* mul, float* out, long long rows, int in, int out_width,
                                    void* stream_) {
    DLWP_REQUIRE(dz && w && out, DLWP_E_INVALID, "graph_dgrad_mul: NULL argument");
    DLWP_REQUIRE(rows > 0, DLWP_E_INVALID, "graph_dgrad_mul: bad shape (%lld rows)", rows);
    DLWP_REQUIRE(rows < ROW_LIMIT, DLWP_E_UNSUPPORTED, "graph_dgrad_mul: more than 2^31 - 64 rows");
    DLWP_REQUIRE(width_ok(in, MAXW) && width_ok(out_width, MAXW), DLWP_E_UNSUPPORTED,
                 "graph_dgrad_mul: width (input %d, output %d) outside 1..%d", in, out_width, MAXW);
    GradArgs a{};
    a.dz = dz; a.w = w; a.mul = mul; a.o0 = out;
    a.p.R = (int)rows; a.p.D0 = a.p.K = in; a.N = out_width;
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, 2.0 * rows * in * out_width,
                       4.0 * ((double)rows * ((mul ? 2.0 : 1.0) * in + out_width) + (double)in * out_width), "graph_dgrad_mul");
    launch_dgrad<4, TIMES>(ROWS, a, s);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_graph_gather_sum(const float* in1, const int* ptr1, const int* eid1, int mean1, const float* in2, const int* ptr2,
                                     const int* eid2, const float* add, float* out, int B, int N, int E, int C, void* stream_) {
    DLWP_REQUIRE(in1 && ptr1 && eid1 && out, DLWP_E_INVALID, "graph_gather_sum: NULL argument");
    DLWP_REQUIRE(!in2 || (ptr2 && eid2), DLWP_E_INVALID, "graph_gather_sum: NULL argument (second list)");
    return launch_gather_sum("graph_gather_sum", in1, ptr1, eid1, mean1, in2, ptr2, eid2, add, out, B, N, E, C, MAXW, (hipStream_t)stream_);
}

extern "C" int dlwp_graph_edge_gather(const float* in, const int* dst, const int* in_ptr, const float* add, float* out, int B, int N,
                                      int E, int C, void* stream_) {
    return launch_edge_gather("graph_edge_gather", in, dst, in_ptr, add, out, B, N, E, C, MAXW, (hipStream_t)stream_);
}

extern "C" long long dlwp_graph_ln_bwd_ws_floats(long long rows, int C) { return ln_bwd_ws_floats("graph_ln_bwd_ws_floats", rows, C, false); }

extern "C" int dlwp_graph_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dz, float* ws,
                                 float* ggamma, float* gbeta, long long rows, int C, void* stream_) {
    return launch_ln_bwd("graph_ln_bwd", "graph_ln_bwd_fold", dy, xhat, rstd, gamma, dz, ws, ggamma, gbeta, rows, C, false,
                         (hipStream_t)stream_);
}

// ---------------------------------------------------------------- the wide, bipartite family, widths 1..512
extern "C" long long dlwp_graph_wide_ln_bwd_ws_floats(long long rows, int C) {
    return ln_bwd_ws_floats("graph_wide_ln_bwd_ws_floats", rows, C, true);
}

extern "C" int dlwp_graph_wide_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dz, float* ws,
                                      float* ggamma, float* gbeta, long long rows, int C, void* stream_) {
    return launch_ln_bwd("graph_wide_ln_bwd", "graph_wide_ln_bwd_fold", dy, xhat, rstd, gamma, dz, ws, ggamma, gbeta, rows, C, true,
                         (hipStream_t)stream_);
}

extern "C" long long dlwp_graph_wide_wgrad0_ws_floats(const dlwp_graph_wide_operand* op, int N) {
    Operand p;
    long long rows;
    const int rc = wide_operand("graph_wide_wgrad0_ws_floats", op, &p, &rows);
    if (rc) return rc;
    if (!width_ok(N, WIDE_MAXW)) {
        dlwp_set_error("graph_wide_wgrad0_ws_floats: output width %d outside 1..%d", N, WIDE_MAXW);
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
    DLWP_REQUIRE(width_ok(N, WIDE_MAXW), DLWP_E_UNSUPPORTED, "graph_wide_wgrad0: output width %d outside 1..%d", N, WIDE_MAXW);
    rc = operand_pointers("graph_wide_wgrad0", op->mode, a.p);
    if (rc) return rc;
    DLWP_REQUIRE(dz && ws && gw, DLWP_E_INVALID, "graph_wide_wgrad0: NULL argument (dz, ws or gw)");
    a.dz = dz; a.ws = ws; a.N = N;
    return launch_wgrad0(op->mode, a, rows, gw, gb, (hipStream_t)stream_, WIDE_WGRAD0_NAMES, "graph_wide_wgrad0_fold");
}

extern "C" int dlwp_graph_wide_dgrad(const dlwp_graph_wide_operand* op, const float* dz, const float* w, const float* res,
                                     const float* mul, int mask, float* out0, float* out1, float* out2, int N, void* stream_) {
    GradArgs a{};
    long long rows;
    const int rc = wide_operand("graph_wide_dgrad", op, &a.p, &rows);
    if (rc) return rc;
    DLWP_REQUIRE(width_ok(N, WIDE_MAXW), DLWP_E_UNSUPPORTED, "graph_wide_dgrad: output width %d outside 1..%d", N, WIDE_MAXW);
    DLWP_REQUIRE(dz && w, DLWP_E_INVALID, "graph_wide_dgrad: NULL argument (dz or w)");
    DLWP_REQUIRE(op->mode == ROWS ? out0 != nullptr : (out0 || out1 || out2), DLWP_E_INVALID, "graph_wide_dgrad: NULL argument (no output)");
    DLWP_REQUIRE(!mul || op->mode == ROWS, DLWP_E_INVALID, "graph_wide_dgrad: the multiplier goes with the rows mode");
    a.dz = dz; a.w = w; a.res = res; a.mul = mul; a.mask = mask; a.o0 = out0; a.o1 = out1; a.o2 = out2; a.N = N;
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, 2.0 * rows * a.p.K * N, 4.0 * ((double)rows * ((mul ? 2.0 : 1.0) * a.p.K + N) + (double)a.p.K * N),
                       "graph_wide_dgrad_%s", mode_name(op->mode));
    launch_dgrad<8, FULL>(op->mode, a, s);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_graph_wide_gather_sum(const float* in, const int* ptr, const int* eid, int mean, const float* add, float* out, int B,
                                          int N, int E, int C, void* stream_) {
    DLWP_REQUIRE(in && ptr && eid && out, DLWP_E_INVALID, "graph_wide_gather_sum: NULL argument");
    return launch_gather_sum("graph_wide_gather_sum", in, ptr, eid, mean, nullptr, nullptr, nullptr, add, out, B, N, E, C, WIDE_MAXW,
                             (hipStream_t)stream_);
}

extern "C" int dlwp_graph_wide_edge_gather(const float* in, const int* dst, const int* in_ptr, const float* add, float* out, int B, int N,
                                           int E, int C, void* stream_) {
    return launch_edge_gather("graph_wide_edge_gather", in, dst, in_ptr, add, out, B, N, E, C, WIDE_MAXW, (hipStream_t)stream_);
}
