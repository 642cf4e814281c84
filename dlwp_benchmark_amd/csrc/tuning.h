// tuning.hip -- the registry of measurement knobs: the override of knob `name` (dlwp_set_tuning, else the environment variable
// DLWP_<name>, read at the time of the call) or DLWP_TUNE_UNSET = "the library's own choice".  Standard headers only: the pure host
// route functions (gemm_route.h) include this file and nothing of HIP.
#pragma once
#include <climits>
constexpr int DLWP_TUNE_UNSET = INT_MIN;
int dlwp_tune(const char* name);
inline bool dlwp_tune_on(const char* name) { const int v = dlwp_tune(name); return v != DLWP_TUNE_UNSET && v != 0; }
inline int dlwp_tune_or(const char* name, int dflt) { const int v = dlwp_tune(name); return v == DLWP_TUNE_UNSET ? dflt : v; }
