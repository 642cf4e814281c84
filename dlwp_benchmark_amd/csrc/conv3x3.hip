// 3 x 3 convolutions (stride 1, "same" size) as implicit GEMMs on the exact-fp32 MFMA, and the ConvLSTM cell built on them.
// Reference call sites: every nn.Conv2d(kernel_size=3, padding=1) of src/nsbench/models/convlstm/convlstm.py (:31-39, :105-128,
// circular padding on both axes) and of src/dlwpbench/models/convlstm/convlstm.py (CylinderPad: circular in longitude, zeros
// in latitude), and the cell update of ConvLSTMCell.forward (:67-80).
//
// Layout: activations are channels-last fp32 [B][H][W][C].  M = B*H*W pixels, N = Cout, K = 9*Cin.
//
// One workgroup (4 waves) owns an 8 x 16 pixel tile and NS*16 output columns.  Per chunk of 16 input channels it stages the
// haloed 10 x 18 tile ONCE in LDS and uses it for all nine taps; the halo is resolved while staging (wrap or zeros per axis),
// so no padded copy of a tensor exists anywhere.  The input channels may come from two tensors (x | h_prev): the chunk loop
// runs over the concatenated axis and picks the source per channel, so cat(x, h_prev) is never written either.  K and N are
// zero-filled up to the instruction shape in LDS and in the packed weight image only.
//
// MFMA (common.hip.h mfma16_chunk): lane (r, g) supplies A[pixel r][channels 4g..4g+3] and B[channels 4g..4g+3][column r] and
// receives D[pixels 4g..4g+3][column r]: wave w owns the tile rows 2w and 2w+1 (one 16-pixel row segment per MFMA tile).
//
// Weight images (dlwp_conv3x3_pack) are [column block][channel chunk][tap][g][column][4 channels]: the B fragment of a lane is
// one 16-byte LDS read and a chunk's image is one contiguous copy.  kind 1 reorders the columns of a cell weight so that the
// four gate pre-activations of a hidden channel are the four column tiles of ONE lane; kind 2 is the flipped, transposed image
// that turns the same kernel into the input-gradient product.
//
// HEALPix padding (PAD_HEALPIX, both axes at once; src/dlwpbench/utils/healpix.py HEALPixPadding(1) in front of every
// nn.Conv2d(3) of a HEALPixLayer): B = 12 * spheres square faces, face index fastest.  A ring cell of a face is one pixel of a
// neighbour face or the mean of two (hpx_halo.hip.h), resolved while staging like the other modes (MODE_HPX of the kernels).
// Its input gradient is NOT the same convolution with the flipped weight: MODE_HPX_DGRAD runs the flipped-weight product over
// the PADDED domain (n + 2) x (n + 2) of every face (dz read as zero outside the face) into a scratch, and conv3x3_hpx_fold_kernel
// gives every pixel its interior value plus, in a fixed order, the weighted ring cells that read it (gather form, no atomics).
#include "hpx_halo.hip.h"
#include "row_gemm.hip.h"

namespace {

constexpr int TH = 8, TW = 16;            // pixel tile
constexpr int HR = TH + 2, HC = TW + 2;   // with halo
using rowgemm::KC;                        // channels per chunk
using rowgemm::AP;                        // LDS floats per haloed pixel in the forward kernel
using rowgemm::ZP;                        // LDS floats per pixel of the dz tile in the weight-gradient kernel
constexpr int NPIX_H = HR * HC;           // 180
constexpr int STAGE_IT = (NPIX_H + 15) / 16;

enum { PAD_ZEROS = 0, PAD_CIRCULAR = 1, PAD_HEALPIX = 2 };
enum { MODE_STD = 0, MODE_HPX = 1, MODE_HPX_DGRAD = 2 };   // how a kernel resolves its halo (template parameter)
enum { ACT_NONE = 0, ACT_TANH = 1, ACT_RELU = 2 };
enum { IMG_FWD = 0, IMG_GATES = 1, IMG_DGRAD = 2 };

struct ConvArgs {
    const float *x1, *x2;      // [B][H][W][C1], [B][H][W][C2] (x2 nullable with C2 = 0)
    const float* wimg;
    const float* bias;         // [N] nullable
    float *y1, *y2;            // columns [0, N1) -> y1 [..][N1], [N1, N1 + N2) -> y2 [..][N2]; either may be NULL (not written)
    const float* c_prev;       // cell: [B][H][W][hid] nullable (zeros)
    float *c_out, *gates;      // cell: c [..][hid], activated gates [..][4 hid] (nullable)
    int C1, C2, N1, N2, act;
    int B, H, W, pad_h, pad_w, tiles_h, tiles_w;
    int nchunks, img_chunks;   // chunks walked; chunks per column block of the image (>= nchunks)
};

// source pixel of haloed position (pr, pc) of the tile at (y0, x0): its index b*H*W + y*W + x, or -1 for a zero
__device__ __forceinline__ int halo_pixel(int b, int y0, int x0, int pr, int pc, int H, int W, int pad_h, int pad_w) {
    int yy = y0 - 1 + pr, xx = x0 - 1 + pc;
    if (yy > H || xx > W) return -1;                       // beyond what any pixel of the image reads
    if (yy < 0 || yy == H) { if (pad_h != PAD_CIRCULAR) return -1; yy = yy < 0 ? H - 1 : 0; }
    if (xx < 0 || xx == W) { if (pad_w != PAD_CIRCULAR) return -1; xx = xx < 0 ? W - 1 : 0; }
    return (b * H + yy) * W + xx;
}

// MODE_HPX: faces are n x n (H = W = n), b = 12 * sphere + face.  *second: the other pixel of a mean-of-two cell, or -1.
__device__ __forceinline__ int halo_pixel_hpx(int b, int y0, int x0, int pr, int pc, int n, int* second) {
    const int yy = y0 - 1 + pr, xx = x0 - 1 + pc;
    *second = -1;
    if (yy > n || xx > n) return -1;
    if (yy >= 0 && yy < n && xx >= 0 && xx < n) return (b * n + yy) * n + xx;
    const int sphere = b / hpx::FACES;
    int s0, s1;
    hpx::halo_sources(n, b - sphere * hpx::FACES, yy + 1, xx + 1, &s0, &s1);
    const int base = sphere * hpx::FACES * n * n;
    if (s1 >= 0) *second = base + s1;
    return base + s0;
}

// MODE_HPX_DGRAD: the tile lies in the PADDED domain np x np (np = n + 2) of face b; position p of it reads dz at p - 1
// of the n x n face, zero outside.
__device__ __forceinline__ int halo_pixel_hpx_dgrad(int b, int y0, int x0, int pr, int pc, int np) {
    const int n = np - 2, yy = y0 - 2 + pr, xx = x0 - 2 + pc;
    if (yy < 0 || yy >= n || xx < 0 || xx >= n) return -1;
    return (b * n + yy) * n + xx;
}

__device__ __forceinline__ float sigmoid_f(float z) { return 1.0f / (1.0f + expf(-z)); }

// CELL = false: y = act(conv + bias) to one or two destinations.  CELL = true (NS = 4, image kind 1): the LSTM update.
// MODE: MODE_STD (zeros / circular per axis), MODE_HPX, or MODE_HPX_DGRAD (H = W = n + 2: the padded domain is the output).
template <int NS, bool CELL, int MODE>
__global__ __launch_bounds__(256) void conv3x3_kernel(const ConvArgs a) {
    extern __shared__ float lds[];
    float* As = lds;                          // [180][AP]
    float* Ws = lds + NPIX_H * AP;            // [9][4][NS*16][4]
    constexpr int WIMG = 9 * 4 * NS * 16 * 4;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    int t = blockIdx.x;
    const int tx = t % a.tiles_w; t /= a.tiles_w;
    const int ty = t % a.tiles_h;
    const int b = t / a.tiles_h;
    const int y0 = ty * TH, x0 = tx * TW, nblk = blockIdx.y;
    const int Cin = a.C1 + a.C2;

    // this thread stages channel (tid & 15) of the haloed pixels (tid >> 4) + 16 i
    int src[STAGE_IT];
    int src2[MODE == MODE_HPX ? STAGE_IT : 1];          // MODE_HPX: the second pixel of a mean-of-two cell, or -1
#pragma unroll
    for (int i = 0; i < STAGE_IT; ++i) {
        const int p = (tid >> 4) + 16 * i;
        const int pr = p / HC, pc = p - pr * HC;
        if constexpr (MODE == MODE_HPX) {
            src[i] = p < NPIX_H ? halo_pixel_hpx(b, y0, x0, pr, pc, a.H, &src2[i]) : (src2[i] = -1, -2);
        } else if constexpr (MODE == MODE_HPX_DGRAD) {
            src[i] = p < NPIX_H ? halo_pixel_hpx_dgrad(b, y0, x0, pr, pc, a.H) : -2;
        } else {
            src[i] = p < NPIX_H ? halo_pixel(b, y0, x0, pr, pc, a.H, a.W, a.pad_h, a.pad_w) : -2;
        }
    }
    f32x4 acc[2][NS];
#pragma unroll
    for (int ms = 0; ms < 2; ++ms)
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) acc[ms][ns] = f32x4{0.f, 0.f, 0.f, 0.f};

    const float* wsrc = a.wimg + (long long)nblk * a.img_chunks * WIMG;
    constexpr int WIT = (WIMG / 4 + 255) / 256;
    float v[STAGE_IT];
    float4 wv[WIT];
    // chunk kc's activations and weight image, global -> registers (issued one chunk ahead: in flight during the MFMAs)
    auto fetch = [&](int kc) {
        const int c = kc * KC + (tid & 15);
        const float* xs = c < a.C1 ? a.x1 + c : (c < Cin ? a.x2 + (c - a.C1) : nullptr);
        const int cs = c < a.C1 ? a.C1 : a.C2;
#pragma unroll
        for (int i = 0; i < STAGE_IT; ++i) {
            v[i] = (xs && src[i] >= 0) ? xs[(long long)src[i] * cs] : 0.f;
            if constexpr (MODE == MODE_HPX)
                if (xs && src2[i] >= 0) v[i] = 0.5f * (v[i] + xs[(long long)src2[i] * cs]);
        }
        const float4* w4 = reinterpret_cast<const float4*>(wsrc + (long long)kc * WIMG);
#pragma unroll
        for (int i = 0; i < WIT; ++i) {
            const int u = tid + 256 * i;
            wv[i] = u < WIMG / 4 ? w4[u] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    fetch(0);
    for (int kc = 0; kc < a.nchunks; ++kc) {
        if (kc) __syncthreads();              // the previous chunk's fragments have been read
#pragma unroll
        for (int i = 0; i < STAGE_IT; ++i)
            if (src[i] != -2) As[((tid >> 4) + 16 * i) * AP + (tid & 15)] = v[i];
#pragma unroll
        for (int i = 0; i < WIT; ++i) {
            const int u = tid + 256 * i;
            if (u < WIMG / 4) reinterpret_cast<float4*>(Ws)[u] = wv[i];
        }
        __syncthreads();
        if (kc + 1 < a.nchunks) fetch(kc + 1);      // after the barrier: __syncthreads() waits for loads in flight
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap % 3;
            f32x4 af[2];
#pragma unroll
            for (int ms = 0; ms < 2; ++ms)
                af[ms] = *reinterpret_cast<const f32x4*>(&As[((2 * w + ms + dy) * HC + r + dx) * AP + 4 * g]);
#pragma unroll
            for (int ns = 0; ns < NS; ++ns) {
                const f32x4 bf = *reinterpret_cast<const f32x4*>(&Ws[((tap * 4 + g) * (NS * 16) + ns * 16 + r) * 4]);
#pragma unroll
                for (int ms = 0; ms < 2; ++ms) acc[ms][ns] = mfma16_chunk(af[ms], bf, acc[ms][ns]);
            }
        }
    }

    // epilogue: lane (r, g) holds pixels (row 2w + ms, columns 4g + j) of column tile ns, column r
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
        const int yy = y0 + 2 * w + ms;
        if (yy >= a.H) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = x0 + 4 * g + j;
            if (xx >= a.W) continue;
            const long long pix = ((long long)b * a.H + yy) * a.W + xx;
            if constexpr (CELL) {
                const int hid = a.N1, ch = nblk * 16 + r;
                if (ch >= hid) continue;
                float z[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) z[q] = acc[ms][q][j] + (a.bias ? a.bias[q * hid + ch] : 0.f);
                const float gi = tanhf(z[0]), ig = sigmoid_f(z[1]), fg = sigmoid_f(z[2]), og = sigmoid_f(z[3]);
                const float cp = a.c_prev ? a.c_prev[pix * hid + ch] : 0.f;
                const float cn = fg * cp + ig * gi;
                a.c_out[pix * hid + ch] = cn;
                a.y1[pix * hid + ch] = og * tanhf(cn);
                if (a.gates) {
                    float* gp = a.gates + pix * 4 * hid + ch;
                    gp[0] = gi; gp[hid] = ig; gp[2 * hid] = fg; gp[3 * hid] = og;
                }
            } else {
#pragma unroll
                for (int ns = 0; ns < NS; ++ns) {
                    const int n = (nblk * NS + ns) * 16 + r;
                    if (n >= a.N1 + a.N2) continue;
                    float v = acc[ms][ns][j] + (a.bias ? a.bias[n] : 0.f);
                    if (a.act == ACT_TANH) v = tanhf(v);
                    else if (a.act == ACT_RELU) v = fmaxf(v, 0.f);
                    if (n < a.N1) { if (a.y1) a.y1[pix * a.N1 + n] = v; }
                    else if (a.y2) a.y2[pix * a.N2 + (n - a.N1)] = v;
                }
            }
        }
    }
}

// ---- weight images
__host__ __device__ inline int img_ns(int ncols) { return ncols <= 16 ? 1 : 4; }

struct PackArgs {
    const float* w;       // [Cout][Cin][3][3]
    float* img;
    int Cin, Cout, kind, NS, nblk, nchunks;
};

__global__ __launch_bounds__(256) void conv3x3_pack_kernel(const PackArgs p) {
    const long long total = (long long)p.nblk * p.nchunks * 9 * 4 * p.NS * 16 * 4;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    long long q = e;
    const int s = q & 3; q >>= 2;
    const int n = q % (p.NS * 16); q /= p.NS * 16;
    const int g = q & 3; q >>= 2;
    const int tap = q % 9; q /= 9;
    const int kc = q % p.nchunks;
    const int nblk = (int)(q / p.nchunks);
    const int k = kc * KC + 4 * g + s;
    float v = 0.f;
    if (p.kind == IMG_DGRAD) {                      // K axis = output channels, columns = input channels, taps mirrored
        const int ci = nblk * p.NS * 16 + n;
        if (k < p.Cout && ci < p.Cin) v = p.w[((long long)k * p.Cin + ci) * 9 + (8 - tap)];
    } else {
        int co;
        if (p.kind == IMG_GATES) {
            const int hid = p.Cout / 4, ch = nblk * 16 + (n & 15);
            co = ch < hid ? (n >> 4) * hid + ch : p.Cout;
        } else {
            co = nblk * p.NS * 16 + n;
        }
        if (k < p.Cin && co < p.Cout) v = p.w[((long long)co * p.Cin + k) * 9 + tap];
    }
    p.img[e] = v;
}

// columns, K extent and column tiles per workgroup of an image
inline bool image_geometry(int Cin, int Cout, int kind, int* NS, int* nblk, int* nchunks) {
    if (kind == IMG_FWD) { *NS = img_ns(Cout); *nblk = ceil_div(Cout, *NS * 16); *nchunks = ceil_div(Cin, KC); }
    else if (kind == IMG_GATES) { *NS = 4; *nblk = ceil_div(Cout / 4, 16); *nchunks = ceil_div(Cin, KC); }
    else if (kind == IMG_DGRAD) { *NS = img_ns(Cin); *nblk = ceil_div(Cin, *NS * 16); *nchunks = ceil_div(Cout, KC); }
    else return false;
    return true;
}

// ---- gate backward of the cell (element-wise).  A kernel of its own: dz is read by TWO products (input and weight gradient),
// so it is formed once instead of in the operand-load stage of each.
__global__ __launch_bounds__(256) void convlstm_gate_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ dc_in,
                                                                const float* __restrict__ gates, const float* __restrict__ c_prev,
                                                                const float* __restrict__ c, float* __restrict__ dz,
                                                                float* __restrict__ dc_prev, long long npix, int hid) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= npix * hid) return;
    const long long pix = e / hid;
    const int ch = (int)(e - pix * hid);
    const float* gp = gates + pix * 4 * hid + ch;
    const float gi = gp[0], ig = gp[hid], fg = gp[2 * hid], og = gp[3 * hid];
    const float tc = tanhf(c[e]);
    const float gh = dh ? dh[e] : 0.f;
    const float dc = (dc_in ? dc_in[e] : 0.f) + gh * og * (1.f - tc * tc);
    const float cp = c_prev ? c_prev[e] : 0.f;
    float* zp = dz + pix * 4 * hid + ch;
    zp[0] = dc * ig * (1.f - gi * gi);
    zp[hid] = dc * gi * ig * (1.f - ig);
    zp[2 * hid] = dc * cp * fg * (1.f - fg);
    zp[3 * hid] = gh * tc * og * (1.f - og);
    dc_prev[e] = dc * fg;
}

// dz = gy * act'(y) from the activation's OUTPUT y (tanh: 1 - y^2, relu: y > 0)
__global__ __launch_bounds__(256) void conv3x3_act_bwd_kernel(const float* __restrict__ y, const float* __restrict__ gy,
                                                              float* __restrict__ dz, long long n, int act) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float yv = y[e];
    dz[e] = act == ACT_TANH ? gy[e] * (1.f - yv * yv) : (yv > 0.f ? gy[e] : 0.f);
}

// ---- weight and bias gradient.  dW[co][ci][tap] = sum_p in[p + tap][ci] dz[p][co]: per tap a GEMM with M = input channels,
// N = output channels, K = pixels.  Workgroup (ci block of 16, co block of 64, split s) walks the pixel tiles s, s + S, ...
// with the haloed input tile and the dz tile in LDS; wave w owns output channels 16w..16w+15 and the nine taps (nine
// independent accumulators).  The partial sums go to ws [S][9][Cin_pad][Cout_pad] and are folded in the fixed order s = 0..S-1
// by the fold kernel (no atomics: two launches on the same operands are bit-identical); S is row_gemm.hip.h's split_k_geometry, the
// rule of the row kernels' weight gradients.  The bias gradient rides along as input channel Cin, which is staged as the constant
// 1: its centre tap is sum_p dz[p][co].
struct WgradArgs {
    const float *x1, *x2, *dz;
    float* ws;
    int C1, C2, Cout, B, H, W, pad_h, pad_w, tiles_h, tiles_w, ntiles, S, cin_pad, cout_pad;
};

template <bool HPX>
__global__ __launch_bounds__(256) void conv3x3_wgrad_kernel(const WgradArgs a) {
    __shared__ float As[NPIX_H * KC];
    __shared__ float Zs[TH * TW * ZP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int Cin = a.C1 + a.C2;
    const int c = blockIdx.x * KC + (tid & 15);
    const float* xs = c < a.C1 ? a.x1 + c : (c < Cin ? a.x2 + (c - a.C1) : nullptr);
    const int cs = c < a.C1 ? a.C1 : a.C2;
    const float fill = c == Cin ? 1.f : 0.f;
    const int co0 = blockIdx.y * 64;
    f32x4 acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    float v[STAGE_IT];
    float zv[TH * TW / 4];
    const int co = co0 + (tid & 63);
    // tile t's haloed input channel and dz columns, global -> registers (issued one tile ahead)
    auto fetch = [&](int t) {
        int q = t;
        const int tx = q % a.tiles_w; q /= a.tiles_w;
        const int ty = q % a.tiles_h;
        const int b = q / a.tiles_h;
        const int y0 = ty * TH, x0 = tx * TW;
#pragma unroll
        for (int i = 0; i < STAGE_IT; ++i) {
            const int p = (tid >> 4) + 16 * i;
            const int pr = p / HC, pc = p - pr * HC;
            if constexpr (HPX) {
                int sp2 = -1;
                const int sp = p < NPIX_H ? halo_pixel_hpx(b, y0, x0, pr, pc, a.H, &sp2) : -1;
                v[i] = xs ? (sp >= 0 ? xs[(long long)sp * cs] : 0.f) : fill;
                if (xs && sp2 >= 0) v[i] = 0.5f * (v[i] + xs[(long long)sp2 * cs]);
            } else {
                const int sp = p < NPIX_H ? halo_pixel(b, y0, x0, pr, pc, a.H, a.W, a.pad_h, a.pad_w) : -1;
                v[i] = xs ? (sp >= 0 ? xs[(long long)sp * cs] : 0.f) : fill;
            }
        }
        // dz tile: thread -> column (tid & 63), pixels (tid >> 6) + 4 i
#pragma unroll
        for (int i = 0; i < TH * TW / 4; ++i) {
            const int m = (tid >> 6) + 4 * i;
            const int yy = y0 + (m >> 4), xx = x0 + (m & 15);
            zv[i] = (yy < a.H && xx < a.W && co < a.Cout) ? a.dz[(((long long)b * a.H + yy) * a.W + xx) * a.Cout + co] : 0.f;
        }
    };
    if ((int)blockIdx.z < a.ntiles) fetch(blockIdx.z);
    for (int t = blockIdx.z; t < a.ntiles; t += a.S) {
        __syncthreads();                      // the previous tile has been consumed
#pragma unroll
        for (int i = 0; i < STAGE_IT; ++i) {
            const int p = (tid >> 4) + 16 * i;
            if (p < NPIX_H) As[p * KC + (tid & 15)] = v[i];
        }
#pragma unroll
        for (int i = 0; i < TH * TW / 4; ++i) Zs[((tid >> 6) + 4 * i) * ZP + (tid & 63)] = zv[i];
        __syncthreads();
        if (t + a.S < a.ntiles) fetch(t + a.S);
#pragma unroll 4
        for (int i = 0; i < TH * TW / 4; ++i) {
            const int m = 4 * i + g, row = m >> 4, col = m & 15;
            const float bz = Zs[m * ZP + 16 * w + r];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
                acc[tap] = mfma16(As[((row + tap / 3) * HC + col + tap % 3) * KC + r], bz, acc[tap]);
        }
    }
    // lane (r, g) register j: input channel 4g + j of the block, output channel 16w + r
    float* dst = a.ws + (long long)blockIdx.z * 9 * a.cin_pad * a.cout_pad;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            dst[((long long)tap * a.cin_pad + blockIdx.x * KC + 4 * g + j) * a.cout_pad + co0 + 16 * w + r] = acc[tap][j];
}

// gw[co][ci][tap] += sum_s ws[s][tap][ci][co];  gb[co] += sum_s ws[s][centre][Cin][co]
__global__ __launch_bounds__(256) void conv3x3_wgrad_fold_kernel(const float* __restrict__ ws, float* gw, float* gb, int Cin,
                                                                 int Cout, int S, int cin_pad, int cout_pad) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;      // (tap, ci <= Cin, co), co fastest
    if (e >= (long long)9 * (Cin + 1) * Cout) return;
    const int co = (int)(e % Cout);
    const int ci = (int)((e / Cout) % (Cin + 1));
    const int tap = (int)(e / ((long long)Cout * (Cin + 1)));
    if (ci == Cin && (tap != 4 || !gb)) return;
    const long long stride = (long long)9 * cin_pad * cout_pad;
    const float* p = ws + ((long long)tap * cin_pad + ci) * cout_pad + co;
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += p[i * stride];
    if (ci == Cin) gb[co] += s;
    else gw[((long long)co * Cin + ci) * 9 + tap] += s;
}

inline void wgrad_geometry(int B, int H, int W, int Cin, int Cout, int* cin_pad, int* cout_pad, int* ntiles, int* S) {
    *ntiles = B * ceil_div(H, TH) * ceil_div(W, TW);
    rowgemm::split_k_geometry(*ntiles, Cin + 1, Cout, cin_pad, cout_pad, S);
}

// ---- HEALPix input gradient, second half: dx = P^T G with G [B][n + 2][n + 2][C] the flipped-weight product over the padded
// domain.  Gather form: pixel (b, y, x) takes its interior value G[b][y + 1][x + 1] and then, in the order of the table, the
// at most four ring cells that read it.  table [12][4 n - 4][4]: per border pixel (hpx::ring_pixel) entries
// (cell << 1) | half, cell = (face * (n + 2) + pr) * (n + 2) + pc within the sphere, half = 1 for weight 0.5; -1 = none.
// Channel c < C1 goes to g1 [..][C1], the others to g2 [..][C - C1]; a NULL destination is skipped.
__global__ __launch_bounds__(256) void conv3x3_hpx_fold_kernel(const float* __restrict__ G, const int* __restrict__ table,
                                                               float* __restrict__ g1, float* __restrict__ g2, int B, int n, int C1,
                                                               int C) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)B * n * n * C) return;
    const int c = (int)(e % C);
    const int pix = (int)(e / C);
    const int x = pix % n, y = (pix / n) % n, b = pix / (n * n);
    const int np = n + 2, ncell = hpx::FACES * np * np;
    float v = G[(((long long)b * np + y + 1) * np + x + 1) * C + c];
    if (y == 0 || y == n - 1 || x == 0 || x == n - 1) {
        const int sphere = b / hpx::FACES, f = b - sphere * hpx::FACES;
        const int* t = table + ((long long)f * (4 * n - 4) + hpx::ring_pixel(n, y, x)) * 4;
        const float* Gs = G + (long long)sphere * ncell * C + c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ent = t[q];
            if (ent < 0 || (ent >> 1) >= ncell) continue;       // no reader (or a table that is not this face size's)
            const float gv = Gs[(long long)(ent >> 1) * C];
            v += (ent & 1) ? 0.5f * gv : gv;
        }
    }
    if (c < C1) { if (g1) g1[(long long)pix * C1 + c] = v; }
    else if (g2) g2[(long long)pix * (C - C1) + (c - C1)] = v;
}

bool pad_ok(int p) { return p == PAD_ZEROS || p == PAD_CIRCULAR; }

// the padding pair of an entry point: 0 = per-axis zeros / circular, 1 = HEALPix (valid), negative = refused (error set)
int pad_mode(const char* who, int pad_h, int pad_w, int B, int H, int W) {
    if (pad_h != PAD_HEALPIX && pad_w != PAD_HEALPIX) {
        if (pad_ok(pad_h) && pad_ok(pad_w)) return MODE_STD;
        dlwp_set_error("%s: unknown padding code (%d, %d)", who, pad_h, pad_w);
        return DLWP_E_INVALID;
    }
    if (pad_h != pad_w) {
        dlwp_set_error("%s: HEALPix padding applies to both axes at once (padding codes %d, %d)", who, pad_h, pad_w);
        return DLWP_E_INVALID;
    }
    if (B % hpx::FACES != 0 || H != W || H < 2) {
        dlwp_set_error("%s: HEALPix padding needs 12 square faces of at least 2 x 2 pixels per sphere (B %d, H %d, W %d)", who, B, H, W);
        return DLWP_E_INVALID;
    }
    return MODE_HPX;
}

template <int NS, bool CELL, int MODE>
int launch_conv(const ConvArgs& a, int nblk, hipStream_t s) {
    const size_t lds = (size_t)(NPIX_H * AP + 9 * 4 * NS * 16 * 4) * sizeof(float);
    int rc = dlwp_ensure_lds((const void*)conv3x3_kernel<NS, CELL, MODE>, lds, "conv3x3");
    if (rc) return rc;
    hipLaunchKernelGGL((conv3x3_kernel<NS, CELL, MODE>), dim3(a.B * a.tiles_h * a.tiles_w, nblk), dim3(256), lds, s, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

}  // namespace

extern "C" long long dlwp_conv3x3_image_floats(int Cin, int Cout, int kind) {
    int NS, nblk, nchunks;
    if (Cin <= 0 || Cout <= 0 || !image_geometry(Cin, Cout, kind, &NS, &nblk, &nchunks) || (kind == IMG_GATES && Cout % 4)) {
        dlwp_set_error("conv3x3_image_floats: bad argument (Cin %d, Cout %d, kind %d)", Cin, Cout, kind);
        return DLWP_E_INVALID;
    }
    return (long long)nblk * nchunks * 9 * 4 * NS * 16 * 4;
}

extern "C" int dlwp_conv3x3_pack(const float* w, float* img, int Cin, int Cout, int kind, void* stream_) {
    DLWP_REQUIRE(w && img, DLWP_E_INVALID, "conv3x3_pack: NULL argument");
    DLWP_REQUIRE(Cin > 0 && Cout > 0, DLWP_E_INVALID, "conv3x3_pack: channel counts must be positive (Cin %d, Cout %d)", Cin, Cout);
    PackArgs p{w, img, Cin, Cout, kind, 0, 0, 0};
    DLWP_REQUIRE(image_geometry(Cin, Cout, kind, &p.NS, &p.nblk, &p.nchunks), DLWP_E_INVALID, "conv3x3_pack: unknown image kind %d",
                 kind);
    DLWP_REQUIRE(kind != IMG_GATES || Cout % 4 == 0, DLWP_E_INVALID, "conv3x3_pack: a cell weight has 4 * hidden output channels");
    const long long total = (long long)p.nblk * p.nchunks * 9 * 4 * p.NS * 16 * 4;
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, 0.0, 4.0 * (9.0 * Cin * Cout + total), "conv3x3_pack");
    hipLaunchKernelGGL(conv3x3_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_conv3x3_fwd(const float* x1, const float* x2, const float* wimg, const float* bias, float* y1, float* y2, int B,
                                int H, int W, int C1, int C2, int N1, int N2, int pad_h, int pad_w, int act, void* stream_) {
    DLWP_REQUIRE(x1 && wimg && (y1 || y2), DLWP_E_INVALID, "conv3x3_fwd: NULL argument");
    DLWP_REQUIRE(B > 0 && H > 0 && W > 0 && C1 > 0 && C2 >= 0 && N1 >= 0 && N2 >= 0 && N1 + N2 > 0, DLWP_E_INVALID,
                 "conv3x3_fwd: bad shape (B %d, H %d, W %d, C %d + %d, N %d + %d)", B, H, W, C1, C2, N1, N2);
    DLWP_REQUIRE((C2 == 0) == (x2 == nullptr), DLWP_E_INVALID, "conv3x3_fwd: the second input and its channel count go together");
    DLWP_REQUIRE((!y1 || N1 > 0) && (!y2 || N2 > 0), DLWP_E_INVALID, "conv3x3_fwd: a destination without columns");
    const int mode = pad_mode("conv3x3_fwd", pad_h, pad_w, B, H, W);
    if (mode < 0) return mode;
    DLWP_REQUIRE(act >= ACT_NONE && act <= ACT_RELU, DLWP_E_INVALID, "conv3x3_fwd: unknown activation code %d", act);
    DLWP_REQUIRE((long long)B * H * W < (1ll << 31), DLWP_E_UNSUPPORTED, "conv3x3_fwd: more than 2^31 pixels");
    ConvArgs a{};
    a.x1 = x1; a.x2 = x2; a.wimg = wimg; a.bias = bias; a.y1 = y1; a.y2 = y2;
    a.C1 = C1; a.C2 = C2; a.N1 = N1; a.N2 = N2; a.act = act;
    a.B = B; a.H = H; a.W = W; a.pad_h = pad_h; a.pad_w = pad_w;
    a.tiles_h = ceil_div(H, TH); a.tiles_w = ceil_div(W, TW);
    int NS, nblk;
    image_geometry(C1 + C2, N1 + N2, IMG_FWD, &NS, &nblk, &a.nchunks);
    a.img_chunks = a.nchunks;
    hipStream_t s = (hipStream_t)stream_;
    const double px = (double)B * H * W;
    dlwp_prof_scope ps(s, 2.0 * px * 9 * (C1 + C2) * (N1 + N2), 4.0 * (px * (C1 + C2 + N1 + N2) + 9.0 * (C1 + C2) * (N1 + N2)),
                       mode == MODE_HPX ? (NS == 1 ? "conv3x3_hpx_n16" : "conv3x3_hpx_n64") : (NS == 1 ? "conv3x3_n16" : "conv3x3_n64"));
    if (mode == MODE_HPX) return NS == 1 ? launch_conv<1, false, MODE_HPX>(a, nblk, s) : launch_conv<4, false, MODE_HPX>(a, nblk, s);
    return NS == 1 ? launch_conv<1, false, MODE_STD>(a, nblk, s) : launch_conv<4, false, MODE_STD>(a, nblk, s);
}

extern "C" int dlwp_convlstm_cell_fwd(const float* x, const float* h_prev, const float* wimg, const float* bias, const float* c_prev,
                                      float* h, float* c, float* gates, int B, int H, int W, int Cx, int hid, int pad_h, int pad_w,
                                      void* stream_) {
    DLWP_REQUIRE(x && wimg && h && c, DLWP_E_INVALID, "convlstm_cell_fwd: NULL argument");
    DLWP_REQUIRE(B > 0 && H > 0 && W > 0 && Cx > 0 && hid > 0, DLWP_E_INVALID, "convlstm_cell_fwd: bad shape (B %d, H %d, W %d, Cx %d, hidden %d)",
                 B, H, W, Cx, hid);
    const int mode = pad_mode("convlstm_cell_fwd", pad_h, pad_w, B, H, W);
    if (mode < 0) return mode;
    DLWP_REQUIRE((long long)B * H * W < (1ll << 31), DLWP_E_UNSUPPORTED, "convlstm_cell_fwd: more than 2^31 pixels");
    ConvArgs a{};
    a.x1 = x; a.x2 = h_prev; a.wimg = wimg; a.bias = bias; a.y1 = h; a.c_prev = c_prev; a.c_out = c; a.gates = gates;
    a.C1 = Cx; a.C2 = h_prev ? hid : 0; a.N1 = hid;
    a.B = B; a.H = H; a.W = W; a.pad_h = pad_h; a.pad_w = pad_w;
    a.tiles_h = ceil_div(H, TH); a.tiles_w = ceil_div(W, TW);
    int NS, nblk;
    image_geometry(Cx + hid, 4 * hid, IMG_GATES, &NS, &nblk, &a.img_chunks);   // the image always spans x | h_prev
    // zero state (h_prev NULL): the chunks beyond x add nothing; one that straddles x | h_prev reads zeros for the absent half
    a.nchunks = h_prev ? a.img_chunks : ceil_div(Cx, KC);
    hipStream_t s = (hipStream_t)stream_;
    const double px = (double)B * H * W;
    dlwp_prof_scope ps(s, 2.0 * px * 9 * (Cx + a.C2) * 4 * hid, 4.0 * (px * (Cx + a.C2 + 3 * hid + (gates ? 4 * hid : 0)) + 36.0 * (Cx + hid) * hid),
                       mode == MODE_HPX ? "convlstm_cell_hpx_fwd" : "convlstm_cell_fwd");
    return mode == MODE_HPX ? launch_conv<4, true, MODE_HPX>(a, nblk, s) : launch_conv<4, true, MODE_STD>(a, nblk, s);
}

extern "C" int dlwp_convlstm_gate_bwd(const float* dh, const float* dc, const float* gates, const float* c_prev, const float* c,
                                      float* dz, float* dc_prev, long long npix, int hid, void* stream_) {
    DLWP_REQUIRE(gates && c && dz && dc_prev && (dh || dc), DLWP_E_INVALID, "convlstm_gate_bwd: NULL argument");
    DLWP_REQUIRE(npix > 0 && hid > 0, DLWP_E_INVALID, "convlstm_gate_bwd: bad shape (%lld pixels, hidden %d)", npix, hid);
    hipStream_t s = (hipStream_t)stream_;
    const double n = (double)npix * hid;
    dlwp_prof_scope ps(s, 30.0 * n, 4.0 * n * 13, "convlstm_gate_bwd");
    hipLaunchKernelGGL(convlstm_gate_bwd_kernel, dim3((unsigned)((npix * hid + 255) / 256)), dim3(256), 0, s, dh, dc, gates, c_prev, c,
                       dz, dc_prev, npix, hid);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_conv3x3_act_bwd(const float* y, const float* gy, float* dz, long long n, int act, void* stream_) {
    DLWP_REQUIRE(y && gy && dz, DLWP_E_INVALID, "conv3x3_act_bwd: NULL argument");
    DLWP_REQUIRE(n > 0, DLWP_E_INVALID, "conv3x3_act_bwd: bad element count %lld", n);
    DLWP_REQUIRE(act == ACT_TANH || act == ACT_RELU, DLWP_E_INVALID, "conv3x3_act_bwd: unknown activation code %d", act);
    hipStream_t s = (hipStream_t)stream_;
    dlwp_prof_scope ps(s, 3.0 * n, 12.0 * n, "conv3x3_act_bwd");
    hipLaunchKernelGGL(conv3x3_act_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, gy, dz, n, act);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" long long dlwp_conv3x3_wgrad_ws_floats(int B, int H, int W, int Cin, int Cout) {
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) {
        dlwp_set_error("conv3x3_wgrad_ws_floats: bad shape (B %d, H %d, W %d, Cin %d, Cout %d)", B, H, W, Cin, Cout);
        return DLWP_E_INVALID;
    }
    int cin_pad, cout_pad, ntiles, S;
    wgrad_geometry(B, H, W, Cin, Cout, &cin_pad, &cout_pad, &ntiles, &S);
    return (long long)S * 9 * cin_pad * cout_pad;
}

extern "C" int dlwp_conv3x3_wgrad(const float* x1, const float* x2, const float* dz, float* ws, float* gw, float* gb, int B, int H,
                                  int W, int C1, int C2, int Cout, int pad_h, int pad_w, void* stream_) {
    DLWP_REQUIRE(x1 && dz && ws && gw, DLWP_E_INVALID, "conv3x3_wgrad: NULL argument");
    DLWP_REQUIRE(B > 0 && H > 0 && W > 0 && C1 > 0 && C2 >= 0 && Cout > 0, DLWP_E_INVALID,
                 "conv3x3_wgrad: bad shape (B %d, H %d, W %d, C %d + %d, Cout %d)", B, H, W, C1, C2, Cout);
    DLWP_REQUIRE((C2 == 0) == (x2 == nullptr), DLWP_E_INVALID, "conv3x3_wgrad: the second input and its channel count go together");
    const int mode = pad_mode("conv3x3_wgrad", pad_h, pad_w, B, H, W);
    if (mode < 0) return mode;
    DLWP_REQUIRE((long long)B * H * W < (1ll << 31), DLWP_E_UNSUPPORTED, "conv3x3_wgrad: more than 2^31 pixels");
    WgradArgs a{};
    a.x1 = x1; a.x2 = x2; a.dz = dz; a.ws = ws;
    a.C1 = C1; a.C2 = C2; a.Cout = Cout; a.B = B; a.H = H; a.W = W; a.pad_h = pad_h; a.pad_w = pad_w;
    a.tiles_h = ceil_div(H, TH); a.tiles_w = ceil_div(W, TW);
    wgrad_geometry(B, H, W, C1 + C2, Cout, &a.cin_pad, &a.cout_pad, &a.ntiles, &a.S);
    hipStream_t s = (hipStream_t)stream_;
    const double px = (double)B * H * W;
    const int Cin = C1 + C2;
    {
        dlwp_prof_scope ps(s, 2.0 * px * 9 * Cin * Cout, 4.0 * (px * (Cin + Cout) + (double)a.S * 9 * a.cin_pad * a.cout_pad),
                           mode == MODE_HPX ? "conv3x3_hpx_wgrad" : "conv3x3_wgrad");
        const dim3 grid(a.cin_pad / KC, a.cout_pad / 64, a.S);
        if (mode == MODE_HPX) hipLaunchKernelGGL(conv3x3_wgrad_kernel<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(conv3x3_wgrad_kernel<false>, grid, dim3(256), 0, s, a);
        DLWP_LAUNCH_CHECK();
    }
    return dlwp_conv3x3_wgrad_fold(ws, gw, gb, Cin, Cout, a.S, a.cin_pad, a.cout_pad, s);
}

int dlwp_conv3x3_wgrad_fold(const float* ws, float* gw, float* gb, int Cin, int Cout, int S, int cin_pad, int cout_pad, hipStream_t s) {
    const long long n = (long long)9 * (Cin + 1) * Cout;
    dlwp_prof_scope ps(s, (double)S * n, 4.0 * (S + 2.0) * n, "conv3x3_wgrad_fold");
    hipLaunchKernelGGL(conv3x3_wgrad_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws, gw, gb, Cin, Cout, S, cin_pad,
                       cout_pad);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

// ---- HEALPix
extern "C" int dlwp_hpx_halo_sources(int n, int* out) {
    DLWP_REQUIRE(out, DLWP_E_INVALID, "hpx_halo_sources: NULL argument");
    DLWP_REQUIRE(n >= 1 && n <= 4096, DLWP_E_INVALID, "hpx_halo_sources: bad face size %d", n);
    for (int f = 0; f < hpx::FACES; ++f)
        for (int pr = 0; pr < n + 2; ++pr)
            for (int pc = 0; pc < n + 2; ++pc) {
                if (pr != 0 && pr != n + 1 && pc != 0 && pc != n + 1) continue;
                int* o = out + ((long long)f * (4 * n + 4) + hpx::ring_cell(n, pr, pc)) * 2;
                hpx::halo_sources(n, f, pr, pc, o, o + 1);
            }
    return DLWP_OK;
}

extern "C" long long dlwp_conv3x3_hpx_dgrad_ws_floats(int B, int n, int Cin) {
    if (B <= 0 || B % hpx::FACES != 0 || n < 2 || Cin <= 0) {
        dlwp_set_error("conv3x3_hpx_dgrad_ws_floats: bad shape (B %d, face size %d, Cin %d)", B, n, Cin);
        return DLWP_E_INVALID;
    }
    return (long long)B * (n + 2) * (n + 2) * Cin;
}

extern "C" int dlwp_conv3x3_hpx_dgrad(const float* dz, const float* wimg, const int* table, float* ws, float* g1, float* g2, int B,
                                      int n, int Cout, int C1, int C2, void* stream_) {
    DLWP_REQUIRE(dz && wimg && table && ws && (g1 || g2), DLWP_E_INVALID, "conv3x3_hpx_dgrad: NULL argument");
    DLWP_REQUIRE(B > 0 && Cout > 0 && C1 > 0 && C2 >= 0, DLWP_E_INVALID, "conv3x3_hpx_dgrad: bad shape (B %d, face size %d, Cout %d, C %d + %d)",
                 B, n, Cout, C1, C2);
    DLWP_REQUIRE(B % hpx::FACES == 0 && n >= 2, DLWP_E_INVALID,
                 "conv3x3_hpx_dgrad: HEALPix padding needs 12 square faces of at least 2 x 2 pixels per sphere (B %d, face size %d)", B, n);
    DLWP_REQUIRE(!g2 || C2 > 0, DLWP_E_INVALID, "conv3x3_hpx_dgrad: a destination without columns");
    const int np = n + 2, C = C1 + C2;
    DLWP_REQUIRE((long long)B * np * np < (1ll << 31), DLWP_E_UNSUPPORTED, "conv3x3_hpx_dgrad: more than 2^31 pixels");
    ConvArgs a{};
    a.x1 = dz; a.wimg = wimg; a.y1 = ws;
    a.C1 = Cout; a.N1 = C; a.act = ACT_NONE;
    a.B = B; a.H = np; a.W = np; a.pad_h = a.pad_w = PAD_HEALPIX;
    a.tiles_h = ceil_div(np, TH); a.tiles_w = ceil_div(np, TW);
    int NS, nblk;
    image_geometry(C, Cout, IMG_DGRAD, &NS, &nblk, &a.nchunks);
    a.img_chunks = a.nchunks;
    hipStream_t s = (hipStream_t)stream_;
    const double px = (double)B * np * np;
    {
        dlwp_prof_scope ps(s, 2.0 * px * 9 * Cout * C, 4.0 * ((double)B * n * n * Cout + px * C + 9.0 * Cout * C),
                           NS == 1 ? "conv3x3_hpx_dgrad_n16" : "conv3x3_hpx_dgrad_n64");
        const int rc = NS == 1 ? launch_conv<1, false, MODE_HPX_DGRAD>(a, nblk, s) : launch_conv<4, false, MODE_HPX_DGRAD>(a, nblk, s);
        if (rc) return rc;
    }
    {
        const long long nel = (long long)B * n * n * C;
        dlwp_prof_scope ps(s, 4.0 * nel, 4.0 * (px * C + nel), "conv3x3_hpx_fold");
        hipLaunchKernelGGL(conv3x3_hpx_fold_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, s, ws, table, g1, g2, B, n, C1, C);
        DLWP_LAUNCH_CHECK();
    }
    return DLWP_OK;
}
