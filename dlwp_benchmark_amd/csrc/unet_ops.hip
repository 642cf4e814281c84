// The U-Net layers that are not 3 x 3 convolutions: the 2 x 2 average pool, ConvTranspose2d(kernel_size=2, stride=2) and the
// 1 x 1 output convolution.  Reference call sites: th.nn.AvgPool2d(2, 2) of UNetEncoder, th.nn.ConvTranspose2d(.., 2, 2) and
// output_layer = th.nn.Conv2d(.., kernel_size=1) of UNetDecoder in src/nsbench/models/unet/unet.py (:100, :165-171, :178-182) and
// src/dlwpbench/models/unet/unet.py (:177, :260-265, :272-276).
//
// Layout: activations are channels-last fp32 [B][H][W][C], as in conv3x3.hip.  No kernel here uses atomics.
//
// Pool: element-wise, HBM-bound; 16-byte accesses where C % 4 == 0.
//
// Pixel GEMM (pixel_gemm_kernel): Y[M pixels][N] = X[M][K] . Wm[K][N] on the exact-fp32 MFMA, in three addressing modes.
// * PLAIN: row m of X and of Y is pixel m.  The 1 x 1 convolution (K = Cin, N = Cout, Wm[k][n] = w[n][k]) and its input
//   gradient (K = Cout, N = Cin, Wm[k][n] = w[k][n]): the two strides of w are launch arguments.
// * SCATTER: a 2 x 2 stride-2 transposed convolution has no overlap between taps, so it is a 1 x 1 convolution to 4 Cout columns
//   n = tap * Cout + co (tap = 2 di + dj) whose epilogue writes column block tap of input pixel (i, j) to output pixel
//   (2i + di, 2j + dj).  Wm[k][n] = w[k][co][di][dj] of nn.ConvTranspose2d's own [Cin][Cout][2][2].
// * GATHER: its input gradient, dx[p][ci] = sum_{tap, co} dy[pixel(p, tap)][co] w[ci][co][tap]: K = 4 Cout with the same
//   tap-major order, the operand load gathers from the four output pixels, Wm[k][n] = w[n][co][tap].
// One workgroup (4 waves) owns 64 pixels x NS*16 columns and runs the chunk loop of row_gemm.hip.h (row_gemm_chunks) on them: a
// mode is a pair of loaders (the weights straight from the parameter's layout) and an epilogue.
//
// Weight gradients (pixel_wgrad_kernel): gW = X^T . dY with K = pixels, M = input channels, N = columns (Cout, or 4 Cout
// tap-major for the up-convolution, gathered like GATHER), on the split-K tile walk of row_gemm.hip.h (row_wgrad_tiles); the fold
// adds the partial sums INTO gw and gb in the parameter's own layout.  The bias gradient rides along as input channel Cin, loaded
// as the constant 1 (for the up-convolution the fold adds its four tap columns, tap = 0..3).
#include "row_gemm.hip.h"

namespace {

using namespace rowgemm;

// ---------------------------------------------------------------- average pool
// VEC floats of one pooled pixel per thread: y = 0.25 * (((a + b) + c) + d), a..d = (2i, 2j), (2i, 2j+1), (2i+1, 2j), (2i+1, 2j+1)
template <int VEC>
__global__ __launch_bounds__(256) void avgpool2x2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long total,
                                                             int Ho, int Wo, int Cv) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;      // (b, i, j, channel group), channel group fastest
    if (e >= total) return;
    const int cg = (int)(e % Cv);
    long long q = e / Cv;
    const int j = (int)(q % Wo); q /= Wo;
    const int i = (int)(q % Ho);
    const long long b = q / Ho;
    const long long C = (long long)Cv * VEC, rowf = 2ll * Wo * C;
    const float* p = x + ((b * 2 * Ho + 2 * i) * 2 * Wo + 2 * j) * C + (long long)cg * VEC;
    float* o = y + ((b * Ho + i) * Wo + j) * C + (long long)cg * VEC;
    if constexpr (VEC == 4) {
        const float4 a = *reinterpret_cast<const float4*>(p), bb = *reinterpret_cast<const float4*>(p + C);
        const float4 c = *reinterpret_cast<const float4*>(p + rowf), d = *reinterpret_cast<const float4*>(p + rowf + C);
        float4 r;
        r.x = 0.25f * (((a.x + bb.x) + c.x) + d.x);
        r.y = 0.25f * (((a.y + bb.y) + c.y) + d.y);
        r.z = 0.25f * (((a.z + bb.z) + c.z) + d.z);
        r.w = 0.25f * (((a.w + bb.w) + c.w) + d.w);
        *reinterpret_cast<float4*>(o) = r;
    } else {
        o[0] = 0.25f * (((p[0] + p[C]) + p[rowf]) + p[rowf + C]);
    }
}

// dx = 0.25 * dy at all four positions
template <int VEC>
__global__ __launch_bounds__(256) void avgpool2x2_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, long long total,
                                                             int Ho, int Wo, int Cv) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int cg = (int)(e % Cv);
    long long q = e / Cv;
    const int j = (int)(q % Wo); q /= Wo;
    const int i = (int)(q % Ho);
    const long long b = q / Ho;
    const long long C = (long long)Cv * VEC, rowf = 2ll * Wo * C;
    const float* g = dy + ((b * Ho + i) * Wo + j) * C + (long long)cg * VEC;
    float* o = dx + ((b * 2 * Ho + 2 * i) * 2 * Wo + 2 * j) * C + (long long)cg * VEC;
    if constexpr (VEC == 4) {
        const float4 v = *reinterpret_cast<const float4*>(g);
        const float4 r = make_float4(0.25f * v.x, 0.25f * v.y, 0.25f * v.z, 0.25f * v.w);
        *reinterpret_cast<float4*>(o) = r;
        *reinterpret_cast<float4*>(o + C) = r;
        *reinterpret_cast<float4*>(o + rowf) = r;
        *reinterpret_cast<float4*>(o + rowf + C) = r;
    } else {
        const float r = 0.25f * g[0];
        o[0] = r; o[C] = r; o[rowf] = r; o[rowf + C] = r;
    }
}

// ---------------------------------------------------------------- pixel GEMM
enum { PLAIN = 0, SCATTER = 1, GATHER = 2 };

struct PixArgs {
    const float* x;           // PLAIN / SCATTER: [M][K];  GATHER: dy [B][2H][2W][Cu]
    const float* w;
    const float* bias;        // nullable; PLAIN: [N], SCATTER: [Cu]
    float* y;                 // PLAIN / GATHER: [M][N];  SCATTER: [B][2H][2W][Cu]
    int M, K, N;
    long long wsk, wsn;       // PLAIN: Wm[k][n] = w[k * wsk + n * wsn]
    int H, W, Cu;             // SCATTER / GATHER: the SMALL grid and the up-convolution's output channel count
};

// index of pixel (2i, 2j) of the large grid for pixel m = (b, i, j) of the small one
__device__ __forceinline__ long long up_base(int m, int H, int W) {
    const int j = m % W, q = m / W;
    const int i = q % H, b = q / H;
    return ((long long)b * 2 * H + 2 * i) * 2 * W + 2 * j;
}
// offset (in pixels of the large grid) of tap = 2 di + dj
__device__ __forceinline__ int tap_offset(int tap, int W) { return (tap >> 1) * 2 * W + (tap & 1); }

template <int MODE, int NS>
__global__ __launch_bounds__(256) void pixel_gemm_kernel(const PixArgs a) {
    constexpr int NC = NS * 16;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * NC;

    // staged pixel (tid >> 4) + 16 i: its row of x, or (GATHER) pixel (2i, 2j) of the large grid; -1 beyond M
    long long src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + (tid >> 4) + 16 * i;
        src[i] = m >= a.M ? -1 : (MODE == GATHER ? up_base(m, a.H, a.W) : (long long)m);
    }
    const long long ldx = a.K;                    // 64-bit here, once: widened inside the loader's condition it costs 4 instructions per load
    f32x4 acc[NS];
    row_gemm_chunks<NS>(
        a.K, acc,
        [&](int k, bool ok, float (&v)[4]) {
            if constexpr (MODE == GATHER) {                // k = tap * Cu + co
                const int tap = k / a.Cu, co = k - tap * a.Cu;
                const int off = tap_offset(tap, a.W);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = (ok && src[i] >= 0) ? a.x[(src[i] + off) * a.Cu + co] : 0.f;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = (ok && src[i] >= 0) ? a.x[src[i] * ldx + k] : 0.f;
            }
        },
        [&](int kk, int col, bool ok) -> float {
            const int n = n0 + col;
            if (!(ok && n < a.N)) return 0.f;
            if constexpr (MODE == PLAIN) {
                return a.w[kk * a.wsk + n * a.wsn];
            } else if constexpr (MODE == SCATTER) {        // w[ci = kk][co][tap], n = tap * Cu + co
                const int tap = n / a.Cu, co = n - tap * a.Cu;
                return a.w[((long long)kk * a.Cu + co) * 4 + tap];
            } else {                                       // w[ci = n][co][tap], kk = tap * Cu + co
                const int tap = kk / a.Cu, co = kk - tap * a.Cu;
                return a.w[((long long)n * a.Cu + co) * 4 + tap];
            }
        });

    // epilogue: lane (r, g) register j holds pixel m0 + 16w + 4g + j, column n0 + 16 ns + r
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + 16 * w + 4 * g + j;
        if (m >= a.M) continue;
        const long long ob = MODE == SCATTER ? up_base(m, a.H, a.W) : 0;
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) {
            const int n = n0 + ns * 16 + r;
            if (n >= a.N) continue;
            if constexpr (MODE == SCATTER) {
                const int tap = n / a.Cu, co = n - tap * a.Cu;
                a.y[(ob + tap_offset(tap, a.W)) * a.Cu + co] = acc[ns][j] + (a.bias ? a.bias[co] : 0.f);
            } else {
                a.y[(long long)m * a.N + n] = acc[ns][j] + (a.bias ? a.bias[n] : 0.f);
            }
        }
    }
}

template <int MODE>
int launch_pixel_gemm(const PixArgs& a, hipStream_t s) {
    const dim3 block(256);
    if (a.N <= 16) {
        hipLaunchKernelGGL((pixel_gemm_kernel<MODE, 1>), dim3(ceil_div(a.M, TM), 1), block, 0, s, a);
    } else {
        hipLaunchKernelGGL((pixel_gemm_kernel<MODE, 4>), dim3(ceil_div(a.M, TM), ceil_div(a.N, 64)), block, 0, s, a);
    }
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

// ---------------------------------------------------------------- weight and bias gradients
struct PixWgradArgs {
    const float *x, *dy;      // x [M][Cin];  dy: [M][N] (plain) or [B][2H][2W][Cu] (UP, N = 4 Cu tap-major columns)
    float* ws;                // [S][k_pad][n_pad]
    int M, Cin, N, H, W, Cu, ntiles, S, k_pad, n_pad;
};

template <bool UP>
__global__ __launch_bounds__(256) void pixel_wgrad_kernel(const PixWgradArgs a) {
    const int tid = threadIdx.x;
    const int c = blockIdx.x * KC + (tid & 15);           // input channel this thread stages; channel Cin is the constant 1
    const int col = blockIdx.y * 64 + (tid & 63);         // dy column this thread stages
    const int tap = UP ? col / a.Cu : 0, co = UP ? col - tap * a.Cu : col;
    const int toff = UP ? tap_offset(tap, a.W) : 0;
    row_wgrad_tiles(
        a.ws, a.ntiles, a.S, a.k_pad, a.n_pad,
        [&](int m) -> float { return m < a.M ? (c < a.Cin ? a.x[(long long)m * a.Cin + c] : (c == a.Cin ? 1.f : 0.f)) : 0.f; },
        [&](int m) -> float {
            if (m >= a.M || col >= a.N) return 0.f;
            if constexpr (UP) return a.dy[(up_base(m, a.H, a.W) + toff) * a.Cu + co];
            else return a.dy[(long long)m * a.N + col];
        });
}

// The up-convolution's fold (the plain one is row_wgrad_fold_kernel): N = 4 Cu tap-major columns into the parameter's own layout,
// gw[ci][co][tap] += sum_s ws[s][ci][tap * Cu + co],  gb[co] += sum_tap sum_s ws[s][Cin][tap * Cu + co]
__global__ __launch_bounds__(256) void upconv_wgrad_fold_kernel(const float* __restrict__ ws, float* gw, float* gb, int Cin, int N, int S,
                                                                int k_pad, int n_pad) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;      // (ci <= Cin, column), column fastest
    if (e >= (long long)(Cin + 1) * N) return;
    const int col = (int)(e % N), ci = (int)(e / N), Cu = N / 4;
    const long long stride = (long long)k_pad * n_pad;
    if (ci < Cin) {
        const float* p = ws + (long long)ci * n_pad + col;
        float s = 0.f;
        for (int i = 0; i < S; ++i) s += p[i * stride];
        const int tap = col / Cu, co = col - tap * Cu;
        gw[((long long)ci * Cu + co) * 4 + tap] += s;
    } else if (gb && col < Cu) {
        float s = 0.f;
        for (int tap = 0; tap < 4; ++tap) {
            const float* p = ws + (long long)Cin * n_pad + tap * Cu + col;
            for (int i = 0; i < S; ++i) s += p[i * stride];
        }
        gb[col] += s;
    }
}

constexpr long long PIX_LIMIT = 1ll << 31;

template <bool BWD>
int launch_pool(const float* src, float* dst, int B, int H, int W, int C, hipStream_t s) {
    const int Ho = H / 2, Wo = W / 2;
    const bool vec = C % 4 == 0 && ((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0);
    const int Cv = vec ? C / 4 : C;
    const long long total = (long long)B * Ho * Wo * Cv;
    const double n = (double)B * H * W * C;
    dlwp_prof_scope ps(s, BWD ? 0.25 * n : n, 5.0 * n, BWD ? "avgpool2x2_bwd" : "avgpool2x2_fwd");
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (BWD) {
        if (vec) hipLaunchKernelGGL(avgpool2x2_bwd_kernel<4>, grid, block, 0, s, src, dst, total, Ho, Wo, Cv);
        else hipLaunchKernelGGL(avgpool2x2_bwd_kernel<1>, grid, block, 0, s, src, dst, total, Ho, Wo, Cv);
    } else {
        if (vec) hipLaunchKernelGGL(avgpool2x2_fwd_kernel<4>, grid, block, 0, s, src, dst, total, Ho, Wo, Cv);
        else hipLaunchKernelGGL(avgpool2x2_fwd_kernel<1>, grid, block, 0, s, src, dst, total, Ho, Wo, Cv);
    }
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

}  // namespace

#define POOL_CHECKS(name)                                                                                                          \
    DLWP_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, DLWP_E_INVALID, name ": bad shape (B %d, H %d, W %d, C %d)", B, H, W, C);       \
    DLWP_REQUIRE(H % 2 == 0 && W % 2 == 0, DLWP_E_UNSUPPORTED, name ": odd grid %d x %d (the U-Net's skip connection needs even sizes)", H, W); \
    DLWP_REQUIRE((long long)B * H * W * C < (1ll << 38), DLWP_E_UNSUPPORTED, name ": more than 2^38 elements")

extern "C" int dlwp_avgpool2x2_fwd(const float* x, float* y, int B, int H, int W, int C, void* stream_) {
    DLWP_REQUIRE(x && y, DLWP_E_INVALID, "avgpool2x2_fwd: NULL argument");
    POOL_CHECKS("avgpool2x2_fwd");
    return launch_pool<false>(x, y, B, H, W, C, (hipStream_t)stream_);
}

extern "C" int dlwp_avgpool2x2_bwd(const float* dy, float* dx, int B, int H, int W, int C, void* stream_) {
    DLWP_REQUIRE(dy && dx, DLWP_E_INVALID, "avgpool2x2_bwd: NULL argument");
    POOL_CHECKS("avgpool2x2_bwd");
    return launch_pool<true>(dy, dx, B, H, W, C, (hipStream_t)stream_);
}

#define CONV1X1_SHAPE(name)                                                                                                        \
    DLWP_REQUIRE(npix > 0 && Cin > 0 && Cout > 0, DLWP_E_INVALID, name ": bad shape (%lld pixels, Cin %d, Cout %d)", npix, Cin, Cout); \
    DLWP_REQUIRE(npix < PIX_LIMIT, DLWP_E_UNSUPPORTED, name ": more than 2^31 pixels")
#define UPCONV_SHAPE(name)                                                                                                         \
    DLWP_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, DLWP_E_INVALID, name ": bad shape (B %d, H %d, W %d, Cin %d, Cout %d)", B, \
                 H, W, Cin, Cout);                                                                                                 \
    DLWP_REQUIRE(4ll * B * H * W < PIX_LIMIT && 4ll * Cout < PIX_LIMIT, DLWP_E_UNSUPPORTED, name ": more than 2^31 output pixels or columns")

extern "C" int dlwp_conv1x1_fwd(const float* x, const float* w, const float* bias, float* y, long long npix, int Cin, int Cout,
                                void* stream_) {
    DLWP_REQUIRE(x && w && y, DLWP_E_INVALID, "conv1x1_fwd: NULL argument");
    CONV1X1_SHAPE("conv1x1_fwd");
    PixArgs a{};
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.M = (int)npix; a.K = Cin; a.N = Cout; a.wsk = 1; a.wsn = Cin;
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, 2.0 * npix * Cin * Cout, 4.0 * ((double)npix * (Cin + Cout) + (double)Cin * Cout), "conv1x1");
    return launch_pixel_gemm<PLAIN>(a, s);
}

extern "C" int dlwp_conv1x1_dgrad(const float* dy, const float* w, float* dx, long long npix, int Cin, int Cout, void* stream_) {
    DLWP_REQUIRE(dy && w && dx, DLWP_E_INVALID, "conv1x1_dgrad: NULL argument");
    CONV1X1_SHAPE("conv1x1_dgrad");
    PixArgs a{};
    a.x = dy; a.w = w; a.y = dx; a.M = (int)npix; a.K = Cout; a.N = Cin; a.wsk = Cin; a.wsn = 1;
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, 2.0 * npix * Cin * Cout, 4.0 * ((double)npix * (Cin + Cout) + (double)Cin * Cout), "conv1x1");
    return launch_pixel_gemm<PLAIN>(a, s);
}

extern "C" int dlwp_upconv2x2_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Cout,
                                  void* stream_) {
    DLWP_REQUIRE(x && w && y, DLWP_E_INVALID, "upconv2x2_fwd: NULL argument");
    UPCONV_SHAPE("upconv2x2_fwd");
    PixArgs a{};
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.M = B * H * W; a.K = Cin; a.N = 4 * Cout; a.H = H; a.W = W; a.Cu = Cout;
    hipStream_t s = (hipStream_t)stream_;
    const double px = (double)B * H * W;
    dlwp_prof_scope ps(s, 8.0 * px * Cin * Cout, 4.0 * (px * (Cin + 4.0 * Cout) + 4.0 * Cin * Cout), "upconv2x2_fwd");
    return launch_pixel_gemm<SCATTER>(a, s);
}

extern "C" int dlwp_upconv2x2_dgrad(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Cout, void* stream_) {
    DLWP_REQUIRE(dy && w && dx, DLWP_E_INVALID, "upconv2x2_dgrad: NULL argument");
    UPCONV_SHAPE("upconv2x2_dgrad");
    PixArgs a{};
    a.x = dy; a.w = w; a.y = dx; a.M = B * H * W; a.K = 4 * Cout; a.N = Cin; a.H = H; a.W = W; a.Cu = Cout;
    hipStream_t s = (hipStream_t)stream_;
    const double px = (double)B * H * W;
    dlwp_prof_scope ps(s, 8.0 * px * Cin * Cout, 4.0 * (px * (Cin + 4.0 * Cout) + 4.0 * Cin * Cout), "upconv2x2_dgrad");
    return launch_pixel_gemm<GATHER>(a, s);
}

extern "C" long long dlwp_conv1x1_wgrad_ws_floats(long long npix, int Cin, int Cout) {
    if (npix <= 0 || npix >= PIX_LIMIT || Cin <= 0 || Cout <= 0) {
        dlwp_set_error("conv1x1_wgrad_ws_floats: bad shape (%lld pixels, Cin %d, Cout %d)", npix, Cin, Cout);
        return DLWP_E_INVALID;
    }
    return row_wgrad_ws_floats(npix, Cin, Cout);
}

extern "C" long long dlwp_upconv2x2_wgrad_ws_floats(int B, int H, int W, int Cin, int Cout) {
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || 4ll * B * H * W >= PIX_LIMIT || 4ll * Cout >= PIX_LIMIT) {
        dlwp_set_error("upconv2x2_wgrad_ws_floats: bad shape (B %d, H %d, W %d, Cin %d, Cout %d)", B, H, W, Cin, Cout);
        return DLWP_E_INVALID;
    }
    return row_wgrad_ws_floats((long long)B * H * W, Cin, 4 * Cout);
}

extern "C" int dlwp_conv1x1_wgrad(const float* x, const float* dy, float* ws, float* gw, float* gb, long long npix, int Cin, int Cout,
                                  void* stream_) {
    DLWP_REQUIRE(x && dy && ws && gw, DLWP_E_INVALID, "conv1x1_wgrad: NULL argument");
    CONV1X1_SHAPE("conv1x1_wgrad");
    PixWgradArgs a{};
    a.x = x; a.dy = dy; a.ws = ws; a.M = (int)npix; a.Cin = Cin; a.N = Cout; a.Cu = Cout;
    return launch_row_wgrad(pixel_wgrad_kernel<false>, a, a.M, Cin, a.N, gw, gb, (hipStream_t)stream_, "pixel_wgrad", "pixel_wgrad_fold");
}

extern "C" int dlwp_upconv2x2_wgrad(const float* x, const float* dy, float* ws, float* gw, float* gb, int B, int H, int W, int Cin,
                                    int Cout, void* stream_) {
    DLWP_REQUIRE(x && dy && ws && gw, DLWP_E_INVALID, "upconv2x2_wgrad: NULL argument");
    UPCONV_SHAPE("upconv2x2_wgrad");
    PixWgradArgs a{};
    a.x = x; a.dy = dy; a.ws = ws; a.M = B * H * W; a.Cin = Cin; a.N = 4 * Cout; a.H = H; a.W = W; a.Cu = Cout;
    return launch_row_wgrad(pixel_wgrad_kernel<true>, a, a.M, Cin, a.N, gw, gb, (hipStream_t)stream_, "pixel_wgrad", "pixel_wgrad_fold",
                            upconv_wgrad_fold_kernel);
}
