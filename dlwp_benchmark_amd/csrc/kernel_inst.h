// From a route's run-time integers to one launched kernel instantiation, for every kernel family that is dispatched by a route
// (winattn_route.h, gemm_route.h): the integers as compile-time constants (ki_consts), the instantiation with its accounting name
// formed from the same constants (KI_INST), and the one launch helper (ki_launch).
#pragma once
#include <cstdio>
#include <type_traits>
#include "common.hip.h"
#include "dlwpmi_internal.h"

inline int ki_not_built() { dlwp_set_error("the route names a kernel instantiation that is not built"); return DLWP_E_UNSUPPORTED; }

// ---- a route's run-time integers -> compile-time constants: ki_consts(f, KiOneOf<1, 2>{ndb}, KiBool{bf}, ...) calls
// f(std::integral_constant<int, ndb>{}, std::integral_constant<int, bf>{}, ...); KI_C / KI_B read such a constant inside f
template <int... Vs> struct KiOneOf { int v; };
using KiBool = KiOneOf<0, 1>;
#define KI_C(c) decltype(c)::value
#define KI_B(c) (decltype(c)::value != 0)
template <class F> int ki_consts(F&& f) { return f(); }
template <class F, int... Vs, class... Rest> int ki_consts(F&& f, KiOneOf<Vs...> c, Rest... rest);
template <int V, class F, class... Rest> int ki_bind(F& f, Rest... rest) {
    return ki_consts([&](auto... cs) { return f(std::integral_constant<int, V>{}, cs...); }, rest...);
}
template <class F, int... Vs, class... Rest> int ki_consts(F&& f, KiOneOf<Vs...> c, Rest... rest) {
    int rc = DLWP_OK;
    const bool hit = ((c.v == Vs ? (rc = ki_bind<Vs>(f, rest...), true) : false) || ...);
    return hit ? rc : ki_not_built();
}

// ---- KI_INST(kernel, args...): the instantiation kernel<args...> with its accounting name "kernel<args...>" (as rocprofv3 prints
// it, without the namespace), formatted from the same constants; defaulted template arguments are written out, so the name is whole
struct KiName {
    const char* base;
    int n, val[6];
    bool is_bool[6];
};
template <class... Ts> constexpr KiName ki_name(const char* base, Ts... v) {
    return KiName{base, (int)sizeof...(Ts), {(int)v...}, {std::is_same<Ts, bool>::value...}};
}
inline int ki_format(const KiName& nm, char* buf, size_t n) {
    int len = snprintf(buf, n, "%s", nm.base);
    for (int i = 0; i < nm.n && (size_t)len < n; ++i)
        len += nm.is_bool[i] ? snprintf(buf + len, n - len, "%s%s", i ? ", " : "<", nm.val[i] ? "true" : "false")
                             : snprintf(buf + len, n - len, "%s%d", i ? ", " : "<", nm.val[i]);
    return nm.n && (size_t)len < n ? len + snprintf(buf + len, n - len, ">") : len;
}
template <class... P> struct KiInst { void (*knl)(P...); KiName name; };
template <class... P> constexpr KiInst<P...> ki_inst(void (*knl)(P...), KiName name) { return KiInst<P...>{knl, name}; }
#define KI_INST(KERNEL, ...) ki_inst(KERNEL<__VA_ARGS__>, ki_name(#KERNEL, __VA_ARGS__))

// ---- the launch: dlwp_ensure_lds, the accounting scope, the kernel; nothing is formatted or allocated while live accounting is off.
// KiTag{text}: a suffix of the accounting name (the GEMM's shape tag under dlwp_prof_enable(2)), given in front of the kernel's arguments
struct KiTag { const char* s; };
template <class... P, class... Args>
int ki_launch(const KiInst<P...>& k, dim3 grid, dim3 block, size_t lds, double flops, double bytes, void* stream, KiTag tag, const Args&... args) {
    if (lds)
        if (int rc = dlwp_ensure_lds(reinterpret_cast<const void*>(k.knl), lds, k.name.base)) return rc;
    char name[96] = "";
    if (dlwp_prof_on()) ki_format(k.name, name, sizeof name);
    dlwp_prof_scope prof((hipStream_t)stream, flops, bytes, "%s%s", name, tag.s);
    hipLaunchKernelGGL(k.knl, grid, block, lds, (hipStream_t)stream, args...);
    return DLWP_OK;
}
template <class... P, class... Args>
int ki_launch(const KiInst<P...>& k, dim3 grid, dim3 block, size_t lds, double flops, double bytes, void* stream, const Args&... args) {
    return ki_launch(k, grid, block, lds, flops, bytes, stream, KiTag{""}, args...);
}
