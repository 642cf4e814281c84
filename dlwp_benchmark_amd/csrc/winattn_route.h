// Window attention (winattn.hip, winattn_small.hip), host side: the ROUTE of a call -- the kernel family and the instantiation a shape
// runs on, decided by dlwp_winattn_route_fwd / _bwd (winattn_small.hip) for every *_supported entry, refusal and launch of the two
// files -- and the one helper every launch of the family goes through.
#pragma once
#include <cstdio>
#include <type_traits>
#include "common.hip.h"
#include "dlwpmi_internal.h"

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
inline int wa_not_built() { dlwp_set_error("window attention: the route names an instantiation that is not built"); return DLWP_E_UNSUPPORTED; }

// ---- a route's run-time integers -> compile-time constants: wa_consts(f, WaOneOf<1, 2>{ndb}, WaBool{bf}, ...) calls
// f(std::integral_constant<int, ndb>{}, std::integral_constant<int, bf>{}, ...); WA_C / WA_B read such a constant inside f
template <int... Vs> struct WaOneOf { int v; };
using WaBool = WaOneOf<0, 1>;
#define WA_C(c) decltype(c)::value
#define WA_B(c) (decltype(c)::value != 0)
template <class F> int wa_consts(F&& f) { return f(); }
template <class F, int... Vs, class... Rest> int wa_consts(F&& f, WaOneOf<Vs...> c, Rest... rest);
template <int V, class F, class... Rest> int wa_bind(F& f, Rest... rest) {
    return wa_consts([&](auto... cs) { return f(std::integral_constant<int, V>{}, cs...); }, rest...);
}
template <class F, int... Vs, class... Rest> int wa_consts(F&& f, WaOneOf<Vs...> c, Rest... rest) {
    int rc = DLWP_OK;
    const bool hit = ((c.v == Vs ? (rc = wa_bind<Vs>(f, rest...), true) : false) || ...);
    return hit ? rc : wa_not_built();
}

// ---- WA_INST(kernel, args...): the instantiation kernel<args...> with its accounting name "kernel<args...>" (as rocprofv3 prints
// it, without the namespace), formatted from the same constants; defaulted template arguments are written out, so the name is whole
struct WaName {
    const char* base;
    int n, val[6];
    bool is_bool[6];
};
template <class... Ts> constexpr WaName wa_name(const char* base, Ts... v) {
    return WaName{base, (int)sizeof...(Ts), {(int)v...}, {std::is_same<Ts, bool>::value...}};
}
inline int wa_format(const WaName& nm, char* buf, size_t n) {
    int len = snprintf(buf, n, "%s", nm.base);
    for (int i = 0; i < nm.n && (size_t)len < n; ++i)
        len += nm.is_bool[i] ? snprintf(buf + len, n - len, "%s%s", i ? ", " : "<", nm.val[i] ? "true" : "false")
                             : snprintf(buf + len, n - len, "%s%d", i ? ", " : "<", nm.val[i]);
    return nm.n && (size_t)len < n ? len + snprintf(buf + len, n - len, ">") : len;
}
template <class... P> struct WaInst { void (*knl)(P...); WaName name; };
template <class... P> constexpr WaInst<P...> wa_inst(void (*knl)(P...), WaName name) { return WaInst<P...>{knl, name}; }
#define WA_INST(KERNEL, ...) wa_inst(KERNEL<__VA_ARGS__>, wa_name(#KERNEL, __VA_ARGS__))

// ---- the launch: dlwp_ensure_lds, the accounting scope, the kernel; nothing is formatted or allocated while live accounting is off
template <class... P, class... Args>
int wa_launch(const WaInst<P...>& k, dim3 grid, dim3 block, size_t lds, double flops, double bytes, void* stream, const Args&... args) {
    if (lds)
        if (int rc = dlwp_ensure_lds(reinterpret_cast<const void*>(k.knl), lds, k.name.base)) return rc;
    char name[96] = "";
    if (dlwp_prof_on()) wa_format(k.name, name, sizeof name);
    dlwp_prof_scope prof((hipStream_t)stream, flops, bytes, "%s", name);
    hipLaunchKernelGGL(k.knl, grid, block, lds, (hipStream_t)stream, args...);
    return DLWP_OK;
}
