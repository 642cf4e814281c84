// What the three graph translation units share (graph_ops.hip: the fused forward at widths 1..128; graph_wide.hip: the wide
// forward at widths 1..512; graph_bwd.hip: the backward pass of both): the mode / activation codes, SiLU, the view of a first
// Linear's operand rows, and the host-side shape checks.  A check takes the caller's entry-point name and width limit, so every
// entry point keeps its own error text.  No __global__ kernel lives here.
#pragma once
#include "row_gemm.hip.h"

namespace graphc {

constexpr int MAXW = DLWP_GRAPH_MAX_WIDTH;             // the fused family's widths: 1..128
constexpr int WIDE_MAXW = DLWP_GRAPH_WIDE_MAX_WIDTH;   // the wide family's: 1..512
constexpr int LN_REGS = WIDE_MAXW / 64;                // floats of a row per lane in the one-wave-per-row LayerNorm kernels
constexpr long long ROW_LIMIT = (1ll << 31) - 64;      // the kernels form row indices of a whole last 64-row tile in int

enum { ROWS = DLWP_GRAPH_ROWS, EDGE = DLWP_GRAPH_EDGE, NODE = DLWP_GRAPH_NODE };
enum { NONE = DLWP_GRAPH_WIDE_ACT_NONE, RELU = DLWP_GRAPH_ACT_RELU, SILU = DLWP_GRAPH_ACT_SILU };

// SiLU v s and its derivative s (1 + v (1 - s)), s = 1 / (1 + exp(-v)).  Far out exp(-v) is inf or 0, so s is exactly 0 or 1 and the
// pair is (-0, -0) or (v, 1): the division is IEEE's (1 / inf = 0), and no inf meets an inf or a zero
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

// the operand of a first Linear: ROWS x; EDGE x = e, vs, vd; NODE x = agg, vs = v.  Part widths D0 | D1 | D2, K their sum.  A graph
// on one node set is Ns == Nd, vs == vd, D1 == D2
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

// ---------------------------------------------------------------- host: names and shape checks
inline bool width_ok(int v, int maxw) { return v >= 1 && v <= maxw; }

inline const char* mode_name(int mode) { return mode == ROWS ? "rows" : mode == EDGE ? "edge" : "node"; }

// (rows, C) of an entry point on plain rows
inline int check_rows_c(const char* name, long long rows, int C, int maxw) {
    DLWP_REQUIRE(rows > 0, DLWP_E_INVALID, "%s: bad shape (%lld rows)", name, rows);
    DLWP_REQUIRE(rows < ROW_LIMIT, DLWP_E_UNSUPPORTED, "%s: more than 2^31 - 64 rows", name);
    DLWP_REQUIRE(width_ok(C, maxw), DLWP_E_UNSUPPORTED, "%s: width %d outside 1..%d", name, C, maxw);
    return DLWP_OK;
}

// (B, N, E, C) of a sum or gather between the edges and one node set
inline int check_bnec(const char* name, int B, int N, int E, int C, int maxw) {
    DLWP_REQUIRE(B > 0 && N > 0 && E > 0, DLWP_E_INVALID, "%s: bad shape (B %d, N %d nodes, E %d edges)", name, B, N, E);
    DLWP_REQUIRE(width_ok(C, maxw), DLWP_E_UNSUPPORTED, "%s: width %d outside 1..%d", name, C, maxw);
    DLWP_REQUIRE((long long)B * E < ROW_LIMIT && (long long)B * N < ROW_LIMIT, DLWP_E_UNSUPPORTED, "%s: more than 2^31 - 64 rows", name);
    return DLWP_OK;
}

// the fused family's (mode, B, N, E, rows, De, Dv): fills rows and K0
inline int graph_shape(const char* name, int mode, int B, int N, int E, long long rows_in, int De, int Dv, long long* rows, int* K0) {
    DLWP_REQUIRE(mode == ROWS || mode == EDGE || mode == NODE, DLWP_E_INVALID, "%s: mode %d is none of rows (0), edge (1), node (2)", name, mode);
    DLWP_REQUIRE(width_ok(De, MAXW), DLWP_E_UNSUPPORTED, "%s: width %d outside 1..%d", name, De, MAXW);
    if (mode == ROWS) {
        DLWP_REQUIRE(rows_in > 0, DLWP_E_INVALID, "%s: bad shape (%lld rows)", name, rows_in);
        *rows = rows_in;
        *K0 = De;
    } else {
        DLWP_REQUIRE(B > 0 && N > 0 && E > 0, DLWP_E_INVALID, "%s: bad shape (B %d, N %d nodes, E %d edges)", name, B, N, E);
        DLWP_REQUIRE(width_ok(Dv, MAXW), DLWP_E_UNSUPPORTED, "%s: node width %d outside 1..%d", name, Dv, MAXW);
        *rows = (long long)B * (mode == EDGE ? E : N);
        *K0 = mode == EDGE ? De + 2 * Dv : De + Dv;
        DLWP_REQUIRE((long long)B * E < ROW_LIMIT && (long long)B * N < ROW_LIMIT, DLWP_E_UNSUPPORTED, "%s: more than 2^31 - 64 rows", name);
    }
    DLWP_REQUIRE(*rows < ROW_LIMIT, DLWP_E_UNSUPPORTED, "%s: more than 2^31 - 64 rows", name);
    return DLWP_OK;
}

// the wide family's dlwp_graph_wide_operand: checks its shape and fills the kernels' view of it (pointers included)
inline int wide_operand(const char* name, const dlwp_graph_wide_operand* q, Operand* p, long long* rows) {
    DLWP_REQUIRE(q, DLWP_E_INVALID, "%s: NULL argument (operand)", name);
    const int mode = q->mode;
    DLWP_REQUIRE(mode == ROWS || mode == EDGE || mode == NODE, DLWP_E_INVALID, "%s: mode %d is none of rows (0), edge (1), node (2)", name, mode);
    DLWP_REQUIRE(width_ok(q->D0, WIDE_MAXW), DLWP_E_UNSUPPORTED, "%s: width %d outside 1..%d", name, q->D0, WIDE_MAXW);
    *p = Operand{};
    p->x = q->x; p->vs = q->vs; p->vd = q->vd; p->src = q->src; p->dst = q->dst;
    p->D0 = q->D0;
    if (mode == ROWS) {
        DLWP_REQUIRE(q->rows > 0, DLWP_E_INVALID, "%s: bad shape (%lld rows)", name, q->rows);
        *rows = q->rows;
    } else if (mode == EDGE) {
        DLWP_REQUIRE(q->B > 0 && q->Ns > 0 && q->Nd > 0 && q->E > 0, DLWP_E_INVALID,
                     "%s: bad shape (B %d, %d source nodes, %d destination nodes, E %d edges)", name, q->B, q->Ns, q->Nd, q->E);
        DLWP_REQUIRE(width_ok(q->D1, WIDE_MAXW) && width_ok(q->D2, WIDE_MAXW), DLWP_E_UNSUPPORTED,
                     "%s: node width (source %d, destination %d) outside 1..%d", name, q->D1, q->D2, WIDE_MAXW);
        DLWP_REQUIRE((long long)q->B * q->Ns < ROW_LIMIT && (long long)q->B * q->Nd < ROW_LIMIT, DLWP_E_UNSUPPORTED,
                     "%s: more than 2^31 - 64 rows", name);
        *rows = (long long)q->B * q->E;
        p->Ns = q->Ns; p->Nd = q->Nd; p->E = q->E; p->D1 = q->D1; p->D2 = q->D2;
    } else {
        DLWP_REQUIRE(q->B > 0 && q->Nd > 0, DLWP_E_INVALID, "%s: bad shape (B %d, %d destination nodes)", name, q->B, q->Nd);
        DLWP_REQUIRE(width_ok(q->D1, WIDE_MAXW), DLWP_E_UNSUPPORTED, "%s: node width %d outside 1..%d", name, q->D1, WIDE_MAXW);
        *rows = (long long)q->B * q->Nd;
        p->Nd = q->Nd; p->D1 = q->D1;
    }
    DLWP_REQUIRE(*rows < ROW_LIMIT, DLWP_E_UNSUPPORTED, "%s: more than 2^31 - 64 rows", name);
    p->R = (int)*rows;
    p->K = p->D0 + p->D1 + p->D2;
    return DLWP_OK;
}

inline int operand_pointers(const char* name, int mode, const Operand& p) {
    DLWP_REQUIRE(p.x, DLWP_E_INVALID, "%s: NULL argument (x)", name);
    DLWP_REQUIRE(mode == ROWS || p.vs, DLWP_E_INVALID, "%s: NULL argument (vs)", name);
    DLWP_REQUIRE(mode != EDGE || (p.vd && p.src && p.dst), DLWP_E_INVALID, "%s: NULL argument (vd, src or dst)", name);
    return DLWP_OK;
}

}  // namespace graphc
