// Face-packed 3 x 3 convolutions under HEALPix padding for SMALL faces (n <= 8): the levels of the HEALPix U-Net below its top
// (src/dlwpbench/models/unet/unet.py with mesh = "healpix": faces of 8, 4, 2 and 1 pixels at the published HPX8 width).
//
// conv3x3.hip gives one 8 x 16 pixel tile to ONE face, so an 8 x 8 face fills half of the 128 MFMA rows, a 4 x 4 face an eighth
// and a 2 x 2 face 4 of 128, and it refuses n = 1.  Here the M axis of a workgroup is the pixels of FPT whole CONSECUTIVE faces of
// the folded [12 * spheres][n][n][C] tensor (row m of the tile is pixel f0 * n * n + m: output rows are contiguous in memory):
//
//     n     faces per tile   rows    haloed cells staged per 16-channel chunk
//     1     64               64      576      (128 faces would fit the 160 KiB of LDS too -- 101 KB of cells beside the 37 KB
//     2     32               128     512       weight image -- but cost 72 staging registers per lane, and the level has only
//     4     8                128     288       12 faces per sphere: the smaller tile gives it twice the workgroups)
//     8     2                128     200
//
// A tile may start and end in the middle of a sphere; a halo cell's source in another face is read from global memory.  Per
// chunk of 16 input channels the (n + 2)^2 haloed cells of every packed face are staged ONCE in LDS and serve all nine taps.  The
// sources of every cell (hpx::halo_sources; a mean-of-two cell is staged as 0.5 (a + b)) are resolved once per workgroup into an
// LDS table before the chunk loop; the next chunk's global loads are in flight during the MFMAs.  A lane's row base address is
// computed once per row subtile, after which a tap is the uniform LDS offset (dy (n + 2) + dx) AP.  Channels come from one or two
// tensors, and the weight images are conv3x3.hip's (dlwp_conv3x3_pack kinds 0 and 2), column blocks of 16 and of 64.
//
// The kernel is written for any domain size P; the input gradient is the same kernel over the PADDED domain P = n + 2 of every
// face (PMODE_DGRAD: the staged cell reads dz at offset -2, zero outside the face; 14 / 8 / 3 / 1 faces per tile, the rows past
// faces * P * P masked), followed by the gather fold over a table with up to R readers per pixel (10 at n = 1, where one pixel
// is the whole face).  The weight gradient walks the same packed tiles as its K axis.  Face sizes 3, 5, 6 and 7 are REFUSED
// (DLWP_E_UNSUPPORTED): no HEALPix level of a power-of-two mesh has them, and each would be two more kernel instances per product.
#include "hpx_halo.hip.h"
#include "row_gemm.hip.h"

namespace {

using rowgemm::KC;
using rowgemm::AP;
using rowgemm::ZP;

enum { ACT_NONE = 0, ACT_TANH = 1, ACT_RELU = 2 };
enum { PMODE_FWD = 0, PMODE_DGRAD = 1 };

// tile geometry of domain size P (FWD: P = n; DGRAD: P = n + 2)
template <int P, int MODE>
struct Geo {
    static constexpr int PP = P + 2, CELLS = PP * PP, PIX = P * P;
    static constexpr int FPT = (MODE == PMODE_FWD && P == 1) ? 64 : 128 / PIX;      // faces per tile
    static constexpr int ROWS = FPT * PIX;                                          // <= 128
    static constexpr int MS = (ROWS + 63) / 64;                                     // 16-row subtiles per wave
    static constexpr int NCELL = FPT * CELLS;
    static constexpr int STAGE_IT = (NCELL + 15) / 16;
};

struct PackedArgs {
    const float *x1, *x2;      // [B][n][n][C1], [..][C2] (DGRAD: x1 = dz [B][n][n][C1], x2 = NULL)
    const float* wimg;
    const float* bias;
    float *y1, *y2;            // columns [0, N1) -> y1, [N1, N1 + N2) -> y2; rows are the pixels of the P x P domain of every face
    int C1, C2, N1, N2, act, B, nchunks;
};

// the source pixel(s) of staged cell (pr, pc) of the (P + 2)^2 haloed domain of face b: .x the pixel index (or -1: zero), .y the
// second pixel of a mean-of-two cell (or -1)
template <int P, int MODE>
__device__ __forceinline__ int2 cell_source(int b, int pr, int pc) {
    if constexpr (MODE == PMODE_FWD) {
        constexpr int n = P;
        if (pr >= 1 && pr <= n && pc >= 1 && pc <= n) return make_int2((b * n + pr - 1) * n + pc - 1, -1);
        const int sphere = b / hpx::FACES;
        int s0, s1;
        hpx::halo_sources(n, b - sphere * hpx::FACES, pr, pc, &s0, &s1);
        const int base = sphere * hpx::FACES * n * n;
        return make_int2(base + s0, s1 >= 0 ? base + s1 : -1);
    } else {
        constexpr int n = P - 2;
        const int yy = pr - 2, xx = pc - 2;
        if (yy < 0 || yy >= n || xx < 0 || xx >= n) return make_int2(-1, -1);
        return make_int2((b * n + yy) * n + xx, -1);
    }
}

template <int P, int NS, int MODE>
__global__ __launch_bounds__(256) void conv3x3_hpxp_kernel(const PackedArgs a) {
    using G = Geo<P, MODE>;
    constexpr int WIMG = 9 * 4 * NS * 16 * 4;
    extern __shared__ float lds[];
    float* As = lds;                                          // [NCELL][AP]
    float* Ws = lds + G::NCELL * AP;                          // [9][4][NS*16][4]
    int2* Src = reinterpret_cast<int2*>(Ws + WIMG);           // [NCELL]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int f0 = blockIdx.x * G::FPT, nblk = blockIdx.y;
    const int Cin = a.C1 + a.C2;

    for (int c = tid; c < G::NCELL; c += 256) {
        const int fi = c / G::CELLS, q = c - fi * G::CELLS, pr = q / G::PP, pc = q - pr * G::PP;
        Src[c] = f0 + fi < a.B ? cell_source<P, MODE>(f0 + fi, pr, pc) : make_int2(-1, -1);
    }
    // the LDS base of this lane's row of each subtile: row m = face m / P^2, pixel (py, px) -> cell (py, px) of the haloed face
    int abase[G::MS];
#pragma unroll
    for (int ms = 0; ms < G::MS; ++ms) {
        const int m = (w * G::MS + ms) * 16 + r;
        const int fi = m / G::PIX, q = m - fi * G::PIX, py = q / P, px = q - py * P;
        abase[ms] = (m < G::ROWS ? (fi * G::CELLS + py * G::PP + px) * AP : 0) + 4 * g;     // a masked row reads cell 0
    }
    f32x4 acc[G::MS][NS];
#pragma unroll
    for (int ms = 0; ms < G::MS; ++ms)
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) acc[ms][ns] = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();

    const float* wsrc = a.wimg + (long long)nblk * a.nchunks * WIMG;
    constexpr int WIT = (WIMG / 4 + 255) / 256;
    float v[G::STAGE_IT];
    float4 wv[WIT];
    // chunk kc's activations and weight image, global -> registers (issued one chunk ahead: in flight during the MFMAs)
    auto fetch = [&](int kc) {
        const int c = kc * KC + (tid & 15);
        const float* xs = c < a.C1 ? a.x1 + c : (c < Cin ? a.x2 + (c - a.C1) : nullptr);
        const int cs = c < a.C1 ? a.C1 : a.C2;
#pragma unroll
        for (int i = 0; i < G::STAGE_IT; ++i) {
            const int cell = (tid >> 4) + 16 * i;
            const int2 s = cell < G::NCELL ? Src[cell] : make_int2(-1, -1);
            v[i] = (xs && s.x >= 0) ? xs[(long long)s.x * cs] : 0.f;
            if constexpr (MODE == PMODE_FWD)
                if (xs && s.y >= 0) v[i] = 0.5f * (v[i] + xs[(long long)s.y * cs]);
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
        for (int i = 0; i < G::STAGE_IT; ++i) {
            const int cell = (tid >> 4) + 16 * i;
            if (cell < G::NCELL) As[cell * AP + (tid & 15)] = v[i];
        }
#pragma unroll
        for (int i = 0; i < WIT; ++i) {
            const int u = tid + 256 * i;
            if (u < WIMG / 4) reinterpret_cast<float4*>(Ws)[u] = wv[i];
        }
        __syncthreads();
        if (kc + 1 < a.nchunks) fetch(kc + 1);      // after the barrier: __syncthreads() waits for loads in flight
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int off = ((tap / 3) * G::PP + tap % 3) * AP;
            f32x4 af[G::MS];
#pragma unroll
            for (int ms = 0; ms < G::MS; ++ms) af[ms] = *reinterpret_cast<const f32x4*>(&As[abase[ms] + off]);
#pragma unroll
            for (int ns = 0; ns < NS; ++ns) {
                const f32x4 bf = *reinterpret_cast<const f32x4*>(&Ws[((tap * 4 + g) * (NS * 16) + ns * 16 + r) * 4]);
#pragma unroll
                for (int ms = 0; ms < G::MS; ++ms) acc[ms][ns] = mfma16_chunk(af[ms], bf, acc[ms][ns]);
            }
        }
    }

    // epilogue: lane (r, g) holds rows (w MS + ms) 16 + 4g + j of column tile ns, column r; row m is pixel f0 P^2 + m
    const long long npix = (long long)a.B * G::PIX;
#pragma unroll
    for (int ms = 0; ms < G::MS; ++ms) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = (w * G::MS + ms) * 16 + 4 * g + j;
            const long long pix = (long long)f0 * G::PIX + m;
            if (m >= G::ROWS || pix >= npix) continue;
#pragma unroll
            for (int ns = 0; ns < NS; ++ns) {
                const int n = (nblk * NS + ns) * 16 + r;
                if (n >= a.N1 + a.N2) continue;
                float val = acc[ms][ns][j] + (a.bias ? a.bias[n] : 0.f);
                if (a.act == ACT_TANH) val = tanhf(val);
                else if (a.act == ACT_RELU) val = fmaxf(val, 0.f);
                if (n < a.N1) { if (a.y1) a.y1[pix * a.N1 + n] = val; }
                else if (a.y2) a.y2[pix * a.N2 + (n - a.N1)] = val;
            }
        }
    }
}

// ---- weight and bias gradient: conv3x3.hip's conv3x3_wgrad_kernel with the packed tile as the K step.  Workgroup (ci block of
// 16, co block of 64, split s) walks the packed tiles s, s + S, ...: the haloed cells of its 16 input channels and the dz rows
// of its 64 output channels in LDS, wave w owns output channels 16w..16w+15 and the nine taps.  Input channel Cin is staged as
// the constant 1 (the bias gradient: its centre tap).  A face beyond the last one stages zeros on both sides.  The sources of the
// cells of the 12 faces of a sphere are resolved once per workgroup into an LDS table; a tile's fetch adds its sphere's base.
struct PackedWgradArgs {
    const float *x1, *x2, *dz;
    float* ws;
    int C1, C2, Cout, B, ntiles, S, cin_pad, cout_pad;
};

template <int P>
__global__ __launch_bounds__(256) void conv3x3_hpxp_wgrad_kernel(const PackedWgradArgs a) {
    using G = Geo<P, PMODE_FWD>;
    static_assert((P & (P - 1)) == 0 && G::ROWS % 4 == 0, "the row -> cell arithmetic of the K loop is shifts");
    extern __shared__ float lds[];
    float* As = lds;                           // [NCELL][KC]
    float* Zs = lds + G::NCELL * KC;           // [ROWS][ZP]
    int2* Tb = reinterpret_cast<int2*>(Zs + G::ROWS * ZP);      // [12][CELLS]: the sources of every cell of a face, within its sphere
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    // the tiles change, the geometry of a sphere does not: resolved once, a fetch adds the sphere's base
    for (int e = tid; e < hpx::FACES * G::CELLS; e += 256) {
        const int f = e / G::CELLS, q = e - f * G::CELLS, pr = q / G::PP, pc = q - pr * G::PP;
        Tb[e] = cell_source<P, PMODE_FWD>(f, pr, pc);
    }
    __syncthreads();
    const int Cin = a.C1 + a.C2;
    const int c = blockIdx.x * KC + (tid & 15);
    const float* xs = c < a.C1 ? a.x1 + c : (c < Cin ? a.x2 + (c - a.C1) : nullptr);
    const int cs = c < a.C1 ? a.C1 : a.C2;
    const float fill = c == Cin ? 1.f : 0.f;
    const int co0 = blockIdx.y * 64;
    const int co = co0 + (tid & 63);
    const long long npix = (long long)a.B * G::PIX;
    f32x4 acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    float v[G::STAGE_IT];
    float zv[G::ROWS / 4];
    // tile t's haloed input channel and dz columns, global -> registers (issued one tile ahead)
    auto fetch = [&](int t) {
        const int f0 = t * G::FPT;
#pragma unroll
        for (int i = 0; i < G::STAGE_IT; ++i) {
            const int cell = (tid >> 4) + 16 * i;
            const int fi = cell / G::CELLS, q = cell - fi * G::CELLS, b = f0 + fi;
            float val = 0.f;
            if (cell < G::NCELL && b < a.B) {
                const int sphere = b / hpx::FACES;
                const int2 s = Tb[(b - sphere * hpx::FACES) * G::CELLS + q];
                const int base = sphere * hpx::FACES * G::PIX;
                val = xs ? xs[(long long)(base + s.x) * cs] : fill;
                if (xs && s.y >= 0) val = 0.5f * (val + xs[(long long)(base + s.y) * cs]);
            }
            v[i] = val;
        }
        // dz rows: thread -> column (tid & 63), rows (tid >> 6) + 4 i
#pragma unroll
        for (int i = 0; i < G::ROWS / 4; ++i) {
            const long long pix = (long long)f0 * G::PIX + (tid >> 6) + 4 * i;
            zv[i] = (pix < npix && co < a.Cout) ? a.dz[pix * a.Cout + co] : 0.f;
        }
    };
    if ((int)blockIdx.z < a.ntiles) fetch(blockIdx.z);
    for (int t = blockIdx.z; t < a.ntiles; t += a.S) {
        __syncthreads();                      // the previous tile has been consumed
#pragma unroll
        for (int i = 0; i < G::STAGE_IT; ++i) {
            const int cell = (tid >> 4) + 16 * i;
            if (cell < G::NCELL) As[cell * KC + (tid & 15)] = v[i];
        }
#pragma unroll
        for (int i = 0; i < G::ROWS / 4; ++i) Zs[((tid >> 6) + 4 * i) * ZP + (tid & 63)] = zv[i];
        __syncthreads();
        if (t + a.S < a.ntiles) fetch(t + a.S);
#pragma unroll 4
        for (int i = 0; i < G::ROWS / 4; ++i) {
            const int m = 4 * i + g;
            const int fi = m / G::PIX, q = m - fi * G::PIX, py = q / P, px = q - py * P;
            const int cb = fi * G::CELLS + py * G::PP + px;
            const float bz = Zs[m * ZP + 16 * w + r];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) acc[tap] = mfma16(As[(cb + (tap / 3) * G::PP + tap % 3) * KC + r], bz, acc[tap]);
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

// ---- input gradient, second half: dx = P^T G with G [B][n + 2][n + 2][C] the flipped-weight product over the padded domain.
// Gather form: pixel (b, y, x) takes its interior value G[b][y + 1][x + 1] and then, in the order of the table, the ring cells
// that read it.  table [12][n * n][R] (conv_ops.hpx_fold_rows): entries (cell << 1) | half, ascending, padded with -1.
__global__ __launch_bounds__(256) void conv3x3_hpxp_fold_kernel(const float* __restrict__ G, const int* __restrict__ table, int R,
                                                                float* __restrict__ g1, float* __restrict__ g2, int B, int n, int C1,
                                                                int C) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)B * n * n * C) return;
    const int c = (int)(e % C);
    const int pix = (int)(e / C);
    const int x = pix % n, y = (pix / n) % n, b = pix / (n * n);
    const int np = n + 2, ncell = hpx::FACES * np * np;
    float v = G[(((long long)b * np + y + 1) * np + x + 1) * C + c];
    const int sphere = b / hpx::FACES, f = b - sphere * hpx::FACES;
    const int* t = table + ((long long)(f * n + y) * n + x) * R;
    const float* Gs = G + (long long)sphere * ncell * C + c;
    for (int q = 0; q < R; ++q) {
        const int ent = t[q];
        if (ent < 0) break;                                 // the rows are padded at the end
        if ((ent >> 1) >= ncell) continue;                  // a table that is not this face size's
        const float gv = Gs[(long long)(ent >> 1) * C];
        v += (ent & 1) ? 0.5f * gv : gv;
    }
    if (c < C1) { if (g1) g1[(long long)pix * C1 + c] = v; }
    else if (g2) g2[(long long)pix * (C - C1) + (c - C1)] = v;
}

inline bool packed_face_size(int n) { return n == 1 || n == 2 || n == 4 || n == 8; }

// 12 square faces per sphere of a supported size: DLWP_OK, or the error (set) of entry point `who`
int check_faces(const char* who, int B, int H, int W) {
    if (B <= 0 || B % hpx::FACES != 0 || H != W || H < 1) {
        dlwp_set_error("%s: HEALPix padding needs 12 square faces per sphere (B %d, H %d, W %d)", who, B, H, W);
        return DLWP_E_INVALID;
    }
    if (!packed_face_size(H)) {
        dlwp_set_error("%s: the face-packed kernels are built for faces of 1, 2, 4 and 8 pixels, not %d", who, H);
        return DLWP_E_UNSUPPORTED;
    }
    return DLWP_OK;
}

inline int img_ns(int ncols) { return ncols <= 16 ? 1 : 4; }

template <int P, int NS, int MODE>
int launch_packed(const PackedArgs& a, int nblk, hipStream_t s) {
    using G = Geo<P, MODE>;
    const size_t lds = (size_t)(G::NCELL * AP + 9 * 4 * NS * 16 * 4) * sizeof(float) + (size_t)G::NCELL * sizeof(int2);
    int rc = dlwp_ensure_lds((const void*)conv3x3_hpxp_kernel<P, NS, MODE>, lds, "conv3x3_hpxp");
    if (rc) return rc;
    hipLaunchKernelGGL((conv3x3_hpxp_kernel<P, NS, MODE>), dim3(ceil_div(a.B, G::FPT), nblk), dim3(256), lds, s, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

// n: the FACE size (the domain of MODE_DGRAD is n + 2)
template <int MODE>
int dispatch_packed(const PackedArgs& a, int n, int NS, int nblk, hipStream_t s) {
    constexpr int D = MODE == PMODE_DGRAD ? 2 : 0;
    switch (n) {
        case 1: return NS == 1 ? launch_packed<1 + D, 1, MODE>(a, nblk, s) : launch_packed<1 + D, 4, MODE>(a, nblk, s);
        case 2: return NS == 1 ? launch_packed<2 + D, 1, MODE>(a, nblk, s) : launch_packed<2 + D, 4, MODE>(a, nblk, s);
        case 4: return NS == 1 ? launch_packed<4 + D, 1, MODE>(a, nblk, s) : launch_packed<4 + D, 4, MODE>(a, nblk, s);
        default: return NS == 1 ? launch_packed<8 + D, 1, MODE>(a, nblk, s) : launch_packed<8 + D, 4, MODE>(a, nblk, s);
    }
}

template <int P>
int launch_packed_wgrad(const PackedWgradArgs& a, hipStream_t s) {
    using G = Geo<P, PMODE_FWD>;
    const size_t lds = (size_t)(G::NCELL * KC + G::ROWS * ZP) * sizeof(float) + (size_t)hpx::FACES * G::CELLS * sizeof(int2);
    int rc = dlwp_ensure_lds((const void*)conv3x3_hpxp_wgrad_kernel<P>, lds, "conv3x3_hpxp_wgrad");
    if (rc) return rc;
    hipLaunchKernelGGL(conv3x3_hpxp_wgrad_kernel<P>, dim3(a.cin_pad / KC, a.cout_pad / 64, a.S), dim3(256), lds, s, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

inline int faces_per_tile(int n) { return n == 1 ? 64 : 128 / (n * n); }

inline void packed_wgrad_geometry(int B, int n, int Cin, int Cout, int* cin_pad, int* cout_pad, int* ntiles, int* S) {
    *ntiles = ceil_div(B, faces_per_tile(n));
    rowgemm::split_k_geometry(*ntiles, Cin + 1, Cout, cin_pad, cout_pad, S);
}

}  // namespace

extern "C" int dlwp_conv3x3_hpxp_fwd(const float* x1, const float* x2, const float* wimg, const float* bias, float* y1, float* y2,
                                     int B, int H, int W, int C1, int C2, int N1, int N2, int act, void* stream_) {
    DLWP_REQUIRE(x1 && wimg && (y1 || y2), DLWP_E_INVALID, "conv3x3_hpxp_fwd: NULL argument");
    DLWP_REQUIRE(C1 > 0 && C2 >= 0 && N1 >= 0 && N2 >= 0 && N1 + N2 > 0, DLWP_E_INVALID,
                 "conv3x3_hpxp_fwd: bad shape (B %d, H %d, W %d, C %d + %d, N %d + %d)", B, H, W, C1, C2, N1, N2);
    DLWP_REQUIRE((C2 == 0) == (x2 == nullptr), DLWP_E_INVALID, "conv3x3_hpxp_fwd: the second input and its channel count go together");
    DLWP_REQUIRE((!y1 || N1 > 0) && (!y2 || N2 > 0), DLWP_E_INVALID, "conv3x3_hpxp_fwd: a destination without columns");
    const int rc = check_faces("conv3x3_hpxp_fwd", B, H, W);
    if (rc) return rc;
    DLWP_REQUIRE(act >= ACT_NONE && act <= ACT_RELU, DLWP_E_INVALID, "conv3x3_hpxp_fwd: unknown activation code %d", act);
    DLWP_REQUIRE((long long)B * H * W < (1ll << 31), DLWP_E_UNSUPPORTED, "conv3x3_hpxp_fwd: more than 2^31 pixels");
    PackedArgs a{};
    a.x1 = x1; a.x2 = x2; a.wimg = wimg; a.bias = bias; a.y1 = y1; a.y2 = y2;
    a.C1 = C1; a.C2 = C2; a.N1 = N1; a.N2 = N2; a.act = act; a.B = B;
    const int NS = img_ns(N1 + N2), nblk = ceil_div(N1 + N2, NS * 16);
    a.nchunks = ceil_div(C1 + C2, KC);
    hipStream_t s = (hipStream_t)stream_;
    const double px = (double)B * H * W;
    dlwp_prof_scope ps(s, 2.0 * px * 9 * (C1 + C2) * (N1 + N2), 4.0 * (px * (C1 + C2 + N1 + N2) + 9.0 * (C1 + C2) * (N1 + N2)),
                       NS == 1 ? "conv3x3_hpxp_n16" : "conv3x3_hpxp_n64");
    return dispatch_packed<PMODE_FWD>(a, H, NS, nblk, s);
}

extern "C" long long dlwp_conv3x3_hpxp_dgrad_ws_floats(int B, int n, int Cin) {
    if (B <= 0 || B % hpx::FACES != 0 || n < 1 || Cin <= 0) {
        dlwp_set_error("conv3x3_hpxp_dgrad_ws_floats: bad shape (B %d, face size %d, Cin %d)", B, n, Cin);
        return DLWP_E_INVALID;
    }
    return (long long)B * (n + 2) * (n + 2) * Cin;
}

extern "C" int dlwp_conv3x3_hpxp_dgrad(const float* dz, const float* wimg, const int* table, int R, float* ws, float* g1, float* g2,
                                       int B, int n, int Cout, int C1, int C2, void* stream_) {
    DLWP_REQUIRE(dz && wimg && table && ws && (g1 || g2), DLWP_E_INVALID, "conv3x3_hpxp_dgrad: NULL argument");
    DLWP_REQUIRE(Cout > 0 && C1 > 0 && C2 >= 0 && R >= 1 && R <= 16, DLWP_E_INVALID,
                 "conv3x3_hpxp_dgrad: bad shape (B %d, face size %d, Cout %d, C %d + %d, %d readers per pixel)", B, n, Cout, C1, C2, R);
    const int rc = check_faces("conv3x3_hpxp_dgrad", B, n, n);
    if (rc) return rc;
    DLWP_REQUIRE(!g2 || C2 > 0, DLWP_E_INVALID, "conv3x3_hpxp_dgrad: a destination without columns");
    const int np = n + 2, C = C1 + C2;
    DLWP_REQUIRE((long long)B * np * np < (1ll << 31), DLWP_E_UNSUPPORTED, "conv3x3_hpxp_dgrad: more than 2^31 pixels");
    PackedArgs a{};
    a.x1 = dz; a.wimg = wimg; a.y1 = ws;
    a.C1 = Cout; a.N1 = C; a.act = ACT_NONE; a.B = B;
    const int NS = img_ns(C), nblk = ceil_div(C, NS * 16);
    a.nchunks = ceil_div(Cout, KC);
    hipStream_t s = (hipStream_t)stream_;
    const double px = (double)B * np * np;
    {
        dlwp_prof_scope ps(s, 2.0 * px * 9 * Cout * C, 4.0 * ((double)B * n * n * Cout + px * C + 9.0 * Cout * C),
                           NS == 1 ? "conv3x3_hpxp_dgrad_n16" : "conv3x3_hpxp_dgrad_n64");
        const int rc2 = dispatch_packed<PMODE_DGRAD>(a, n, NS, nblk, s);
        if (rc2) return rc2;
    }
    {
        const long long nel = (long long)B * n * n * C;
        dlwp_prof_scope ps(s, (double)R * nel, 4.0 * (px * C + nel), "conv3x3_hpxp_fold");
        hipLaunchKernelGGL(conv3x3_hpxp_fold_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, s, ws, table, R, g1, g2, B, n, C1,
                           C);
        DLWP_LAUNCH_CHECK();
    }
    return DLWP_OK;
}

extern "C" long long dlwp_conv3x3_hpxp_wgrad_ws_floats(int B, int n, int Cin, int Cout) {
    if (B <= 0 || !packed_face_size(n) || Cin <= 0 || Cout <= 0) {
        dlwp_set_error("conv3x3_hpxp_wgrad_ws_floats: bad shape (B %d, face size %d, Cin %d, Cout %d)", B, n, Cin, Cout);
        return DLWP_E_INVALID;
    }
    int cin_pad, cout_pad, ntiles, S;
    packed_wgrad_geometry(B, n, Cin, Cout, &cin_pad, &cout_pad, &ntiles, &S);
    return (long long)S * 9 * cin_pad * cout_pad;
}

extern "C" int dlwp_conv3x3_hpxp_wgrad(const float* x1, const float* x2, const float* dz, float* ws, float* gw, float* gb, int B,
                                       int n, int C1, int C2, int Cout, void* stream_) {
    DLWP_REQUIRE(x1 && dz && ws && gw, DLWP_E_INVALID, "conv3x3_hpxp_wgrad: NULL argument");
    DLWP_REQUIRE(C1 > 0 && C2 >= 0 && Cout > 0, DLWP_E_INVALID, "conv3x3_hpxp_wgrad: bad shape (B %d, face size %d, C %d + %d, Cout %d)", B,
                 n, C1, C2, Cout);
    DLWP_REQUIRE((C2 == 0) == (x2 == nullptr), DLWP_E_INVALID, "conv3x3_hpxp_wgrad: the second input and its channel count go together");
    const int rc = check_faces("conv3x3_hpxp_wgrad", B, n, n);
    if (rc) return rc;
    DLWP_REQUIRE((long long)B * n * n < (1ll << 31), DLWP_E_UNSUPPORTED, "conv3x3_hpxp_wgrad: more than 2^31 pixels");
    PackedWgradArgs a{};
    a.x1 = x1; a.x2 = x2; a.dz = dz; a.ws = ws;
    a.C1 = C1; a.C2 = C2; a.Cout = Cout; a.B = B;
    const int Cin = C1 + C2;
    packed_wgrad_geometry(B, n, Cin, Cout, &a.cin_pad, &a.cout_pad, &a.ntiles, &a.S);
    hipStream_t s = (hipStream_t)stream_;
    const double px = (double)B * n * n;
    {
        dlwp_prof_scope ps(s, 2.0 * px * 9 * Cin * Cout, 4.0 * (px * (Cin + Cout) + (double)a.S * 9 * a.cin_pad * a.cout_pad),
                           "conv3x3_hpxp_wgrad");
        const int rc2 = n == 1 ? launch_packed_wgrad<1>(a, s) : n == 2 ? launch_packed_wgrad<2>(a, s)
                        : n == 4 ? launch_packed_wgrad<4>(a, s) : launch_packed_wgrad<8>(a, s);
        if (rc2) return rc2;
    }
    return dlwp_conv3x3_wgrad_fold(ws, gw, gb, Cin, Cout, a.S, a.cin_pad, a.cout_pad, s);
}
