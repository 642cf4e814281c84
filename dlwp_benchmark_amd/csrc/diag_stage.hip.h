// Device helpers shared by the evaluation kernels that read HEALPix planes through the 4-tap hpx2ll table (csrc/rollout_diag.hip,
// csrc/spectra.hip): the interpolation of one lat-lon point and the copy of a group of frames' planes to LDS.  One definition, so
// that both kernels form an interpolated value with the same four products and three additions.
#pragma once
#include "common.hip.h"

namespace {

__device__ __forceinline__ float tap4(const float* __restrict__ s, const int4 i, const float4 w) {
    return fmaf(w.w, s[i.w], fmaf(w.z, s[i.z], fmaf(w.y, s[i.y], w.x * s[i.x])));
}
// the planes of `nf` frames -> LDS, frame k at lds + 2 k npix (out, then target; o == nullptr: the targets alone).  Four loads are
// issued before their four LDS stores, so a thread has 64 bytes (vec) in flight per pass and the frames of a group arrive together
__device__ __forceinline__ void stage_group(float* lds, const float* __restrict__ o, long long ots, const float* __restrict__ t,
                                            long long tts, int nf, int npix, int vec) {
    const int per = vec ? npix >> 2 : npix;                  // pieces per plane
    const int total = nf * 2 * per;
    for (int base = threadIdx.x; base < total; base += 4 * 256) {
        float4 r[4];
        int dst[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = base + u * 256;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            int d = -1;
            if (e < total) {
                const int pl = e / per, off = e - pl * per, k = pl >> 1;      // plane pl = 2 k (out) or 2 k + 1 (target)
                const float* src = (pl & 1) ? t + k * tts : (o ? o + k * ots : nullptr);
                if (src) {
                    d = pl * npix + (vec ? 4 * off : off);
                    if (vec) x = reinterpret_cast<const float4*>(src)[off];
                    else x.x = src[off];
                }
            }
            r[u] = x;
            dst[u] = d;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (dst[u] >= 0) {
                if (vec) *reinterpret_cast<float4*>(lds + dst[u]) = r[u];
                else lds[dst[u]] = r[u].x;
            }
    }
}

}  // namespace
