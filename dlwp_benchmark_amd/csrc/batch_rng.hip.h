// The noise stream of the batch-assembly kernels (batch_ops.hip): Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw,
// "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the map from its words to standard normals.  Host and device
// compile the same text, so the known answers of docs/kernels/data.md can be checked without a GPU.
//
// Element e (linear index inside ONE sample's noisy tensor) of dataset item i in epoch p under the 64-bit seed s:
//   counter = (e >> 2, i, p, tag)   key = (s & 0xffffffff, s >> 32)   -> words w[0..3]
//   j = e & 3, q = j >> 1:  u1 = ((w[2q] >> 8) + 1) 2^-24 in (0, 1],  u2 = (w[2q + 1] >> 8) 2^-24 in [0, 1)
//   z = sqrt(-2 ln u1) * (j even ? cos(2 pi u2) : sin(2 pi u2))
// so the four elements of an aligned group of four share one Philox call, and |z| <= sqrt(48 ln 2) = 5.77.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

struct dlwp_philox_words {
    uint32_t w[4];
};

__host__ __device__ inline void dlwp_mulhilo32(uint32_t a, uint32_t b, uint32_t* hi, uint32_t* lo) {
    const uint64_t p = (uint64_t)a * b;
    *hi = (uint32_t)(p >> 32);
    *lo = (uint32_t)p;
}

__host__ __device__ inline dlwp_philox_words dlwp_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                                uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        uint32_t hi0, lo0, hi1, lo1;
        dlwp_mulhilo32(0xD2511F53u, c0, &hi0, &lo0);
        dlwp_mulhilo32(0xCD9E8D57u, c2, &hi1, &lo1);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
        k0 += 0x9E3779B9u;      // (the bump after the last round is unused)
        k1 += 0xBB67AE85u;
    }
    return dlwp_philox_words{{c0, c1, c2, c3}};
}

// the two normals of the word pair (a, b): cos branch in *zc, sin branch in *zs.  2 u2 is exact in fp32, so sincospif sees the
// angle without the rounding of 2 pi u2
__host__ __device__ inline void dlwp_box_muller(uint32_t a, uint32_t b, float* zc, float* zs) {
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;
    const float u2x2 = (float)(b >> 8) * 0x1p-23f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
#ifdef __HIP_DEVICE_COMPILE__
    sincospif(u2x2, &s, &c);
#else
    s = sinf(3.14159265358979323846f * u2x2), c = cosf(3.14159265358979323846f * u2x2);      // host: known-answer checks only
#endif
    *zc = r * c;
    *zs = r * s;
}

// the four normals of the elements 4 g .. 4 g + 3 of item `item` in epoch `epoch`
__host__ __device__ inline void dlwp_noise4(uint32_t g, uint32_t item, uint32_t epoch, uint32_t tag, uint32_t k0, uint32_t k1,
                                            float z[4]) {
    const dlwp_philox_words p = dlwp_philox4x32_10(g, item, epoch, tag, k0, k1);
    dlwp_box_muller(p.w[0], p.w[1], &z[0], &z[1]);
    dlwp_box_muller(p.w[2], p.w[3], &z[2], &z[3]);
}
