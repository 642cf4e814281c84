// Window attention (winattn.hip, winattn_small.hip), host side: the ROUTE of a call -- the kernel family and the instantiation a shape
// runs on, decided by dlwp_winattn_route_fwd / _bwd (winattn_small.hip) for every *_supported entry, refusal and launch of the two
// files.  A route becomes a launched instantiation through kernel_inst.h (ki_consts, KI_INST, ki_launch).
#pragma once
#include "kernel_inst.h"

enum WaFamily {
    WA_NONE,             // unsupported: WaRoute::why holds what the entry reports
    WA_TILED,            // winattn_fwd_kernel / winattn_bwd_q_kernel + winattn_bwd_kv_kernel <NDB, NBUF, BF>
    WA_WAVE_FWD,         // winattn_small_fwd_kernel<NC, NDB, VEC, BF, TOK, IOBF>
    WA_WAVE_BWD,         // winattn_small_bwd_kernel<NDB, VEC, BF>
    WA_LDS_BWD2,         // winattn_lds_bwd_kernel<NDB>                 (two passes)
    WA_LDS_BWD1P,        // winattn_lds_bwd1p_kernel<NDB, NW, IOBF>     (one pass)
    WA_LDS_FWD_TOK,      // winattn_lds_fwd_tok_kernel<NC, NDB, IOBF>
};
// layout bits of a call (0: fp32 arrays in the window layout): the *_tokens entries (gradients / outputs in the unpartitioned token
// layout through position maps), their operands too (fill != NULL), bf16 tensors
enum { WA_TOKENS = 1, WA_FILL = 2, WA_IO_BF16 = 4 };
struct WaCall {
    int layout, N, d, TB;
    long long pairs;     // (window, head) pairs = B_ * heads
    int q_lo, q_hi;      // the caller's query range (no rule reads it today: which chunks to skip is the launcher's business)
};
struct WaRoute {
    WaFamily family;
    int n2, ndb;         // n2: NBUF (tiled), NC (forward families), NW (one-pass backward); ndb: NDB
    bool vec, bf, tok, io;
    const char* why;     // WA_NONE: the refusal's text, a format of (N, d, why_arg); nothing is formatted until an entry reports it
    long long why_arg;
};
WaRoute dlwp_winattn_route_fwd(const WaCall& c);
WaRoute dlwp_winattn_route_bwd(const WaCall& c);
inline int wa_refuse(const WaRoute& r, int N, int d) { dlwp_set_error(r.why, N, d, r.why_arg); return DLWP_E_UNSUPPORTED; }
