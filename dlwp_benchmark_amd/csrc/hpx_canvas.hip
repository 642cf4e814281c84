// HEALPix faces <-> the patch tokens of the 3n x 4n canvas, one launch per direction.
//
// Reference: SwinTransformerHPX (src/dlwpbench/models/swintransformer/swin_transformer.py:745-896) lays the 12 faces of every
// tensor out on a rectangle -- face f, pixel (y, x) -> canvas row (f / 4) n + y, column (f % 4) n + x (_faces2rect :826-834) --
// three times per lead time (constants, prescribed, prognostic), concatenates the three canvases (:862-865), and the patch
// embedding's convolution unfolds the result; after the head _reshape_output (:867-879) splits the canvas into faces again.
// Here:
//   gather : up to three face tensors [B][C_k][12][n][n] (batch stride given: sliding windows are read in place)
//            -> tok [B][3n/ph][4n/pw][Ctot][ph][pw], Ctot = sum C_k -- the rows of the patch-embedding GEMM in the K order of
//            the [O][C ph pw] weight; for patch (1, 1) the channels-last canvas
//   scatter: channels [c0, c0 + C) of such a tok tensor -> dense faces [B][C][12][n][n]
// Each is the other's adjoint: every element has one reader and one writer, nothing is summed, results are bit-exact.
//
// A channel's 12 n n face pixels are one contiguous run (index g = f n n + y n + x), a token's channels another.  One workgroup
// moves a tile of 32 channels x 32 face pixels through LDS: on the face side lanes run along g, on the token side along the
// channel, so both global sides see 128-byte runs per half wave.  tile[32][33]: ds_read_b32 / ds_write_b32 bank = dword % 32
// per 32-lane half; rows are read along the channel with stride 33 dwords -> bank (c + p) % 32, conflict-free both ways.
#include "common.hip.h"
#include "dlwpmi_internal.h"

namespace {

constexpr int TILE = 32;

struct CanvasDev {
    float* face[3];          // face-side tensors (read by the gather, written by the scatter)
    long long bs[3];         // their batch strides in floats
    int c1, c2;              // first canvas channel of face[1] / face[2] (face[0] starts at 0)
    int C;                   // channels moved (gather: Ctot)
    float* tok;
    int Ctot, c0;            // token-side channel count and the first channel moved
    int n, ph, pw;
    long long G;             // 12 n n
};

// offset inside tok of face-pixel g, moved channel c of sample b
__device__ __forceinline__ long long tok_offset(const CanvasDev& a, int b, long long g, int c) {
    const long long nn = (long long)a.n * a.n;
    const int f = (int)(g / nn);
    const int p = (int)(g % nn);
    const int Y = (f >> 2) * a.n + p / a.n, X = (f & 3) * a.n + p % a.n;
    const long long Hh = 3LL * a.n / a.ph, Ww = 4LL * a.n / a.pw;
    return ((((long long)b * Hh + Y / a.ph) * Ww + X / a.pw) * a.Ctot + a.c0 + c) * ((long long)a.ph * a.pw) + (long long)(Y % a.ph) * a.pw +
           X % a.pw;
}

__device__ __forceinline__ float* face_ptr(const CanvasDev& a, int b, long long g, int c) {
    if (c >= a.c2) return a.face[2] + (long long)b * a.bs[2] + (long long)(c - a.c2) * a.G + g;
    if (c >= a.c1) return a.face[1] + (long long)b * a.bs[1] + (long long)(c - a.c1) * a.G + g;
    return a.face[0] + (long long)b * a.bs[0] + (long long)c * a.G + g;
}

template <bool SCATTER>
__global__ __launch_bounds__(256) void hpx_canvas_kernel(CanvasDev a) {
    __shared__ float tile[TILE][TILE + 1];       // [channel][face pixel]
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long long g0 = (long long)blockIdx.x * TILE;
    const int cb = blockIdx.y * TILE, b = blockIdx.z;
    if (!SCATTER) {
        const long long g = g0 + tx;
        for (int cl = ty; cl < TILE; cl += 8)
            if (g < a.G && cb + cl < a.C) tile[cl][tx] = *face_ptr(a, b, g, cb + cl);
    } else {
        const int c = cb + tx;
        for (int pl = ty; pl < TILE; pl += 8)
            if (g0 + pl < a.G && c < a.C) tile[tx][pl] = a.tok[tok_offset(a, b, g0 + pl, c)];
    }
    __syncthreads();
    if (!SCATTER) {
        const int c = cb + tx;
        for (int pl = ty; pl < TILE; pl += 8)
            if (g0 + pl < a.G && c < a.C) a.tok[tok_offset(a, b, g0 + pl, c)] = tile[tx][pl];
    } else {
        const long long g = g0 + tx;
        for (int cl = ty; cl < TILE; cl += 8)
            if (g < a.G && cb + cl < a.C) *face_ptr(a, b, g, cb + cl) = tile[cl][tx];
    }
}

int canvas_check(const char* who, int B, int n, int ph, int pw, int Ctot) {
    DLWP_REQUIRE(n >= 1 && n <= 16384, DLWP_E_INVALID, "%s: face size n %d outside [1, 16384]", who, n);
    DLWP_REQUIRE(ph >= 1 && pw >= 1 && (3 * n) % ph == 0 && (4 * n) % pw == 0, DLWP_E_INVALID,
                 "%s: canvas %d x %d is not divisible by the patch %d x %d", who, 3 * n, 4 * n, ph, pw);
    DLWP_REQUIRE(Ctot >= 1 && Ctot <= 65535 * TILE, DLWP_E_INVALID, "%s: Ctot %d outside [1, %d]", who, Ctot, 65535 * TILE);
    DLWP_REQUIRE(B >= 1 && B <= 65535, DLWP_E_INVALID, "%s: B %d outside the grid limit [1, 65535]", who, B);
    return DLWP_OK;
}

dim3 canvas_grid(const CanvasDev& a, int B) {
    return dim3((unsigned)((a.G + TILE - 1) / TILE), (unsigned)((a.C + TILE - 1) / TILE), (unsigned)B);
}

}  // namespace

extern "C" int dlwp_hpx_canvas_gather(const float* src0, long long bs0, int C0, const float* src1, long long bs1, int C1,
                                      const float* src2, long long bs2, int C2, float* tok, int B, int n, int ph, int pw,
                                      void* stream) {
    DLWP_REQUIRE(tok, DLWP_E_INVALID, "hpx_canvas_gather: NULL tok");
    const float* src[3] = {src0, src1, src2};
    const long long bs[3] = {bs0, bs1, bs2};
    const int Ck[3] = {C0, C1, C2};
    long long Ctot = 0;
    for (int k = 0; k < 3; ++k) {
        DLWP_REQUIRE(Ck[k] >= 0 && (Ck[k] > 0) == (src[k] != nullptr), DLWP_E_INVALID,
                     "hpx_canvas_gather: source %d has %d channels and a %s pointer (a skipped source is NULL with 0 channels)", k,
                     Ck[k], src[k] ? "non-NULL" : "NULL");
        Ctot += Ck[k];
    }
    DLWP_REQUIRE(Ctot <= 65535LL * TILE, DLWP_E_INVALID, "hpx_canvas_gather: Ctot %lld too large", Ctot);
    int rc = canvas_check("hpx_canvas_gather", B, n, ph, pw, (int)Ctot);
    if (rc) return rc;
    CanvasDev a{};
    a.G = 12LL * n * n;
    for (int k = 0; k < 3; ++k) {
        DLWP_REQUIRE(Ck[k] == 0 || bs[k] >= Ck[k] * a.G, DLWP_E_INVALID,
                     "hpx_canvas_gather: source %d batch stride %lld < its sample block %lld", k, bs[k], Ck[k] * a.G);
        a.face[k] = const_cast<float*>(src[k]);
        a.bs[k] = bs[k];
    }
    a.c1 = C0; a.c2 = C0 + C1; a.C = a.Ctot = (int)Ctot; a.c0 = 0; a.tok = tok; a.n = n; a.ph = ph; a.pw = pw;
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 8.0 * B * (double)Ctot * a.G, "hpx_canvas_gather");
    hipLaunchKernelGGL(hpx_canvas_kernel<false>, canvas_grid(a, B), dim3(256), 0, (hipStream_t)stream, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}

extern "C" int dlwp_hpx_canvas_scatter(const float* tok, float* faces, int B, int n, int ph, int pw, int Ctot, int c0, int C,
                                       void* stream) {
    DLWP_REQUIRE(tok && faces, DLWP_E_INVALID, "hpx_canvas_scatter: NULL argument");
    int rc = canvas_check("hpx_canvas_scatter", B, n, ph, pw, Ctot);
    if (rc) return rc;
    DLWP_REQUIRE(c0 >= 0 && C >= 1 && C <= Ctot && c0 <= Ctot - C, DLWP_E_INVALID,
                 "hpx_canvas_scatter: channel range [%d, %d + %d) outside Ctot %d", c0, c0, C, Ctot);
    CanvasDev a{};
    a.G = 12LL * n * n;
    a.face[0] = a.face[1] = a.face[2] = faces;
    a.bs[0] = a.bs[1] = a.bs[2] = C * a.G;
    a.c1 = a.c2 = C;                         // every moved channel lives in face[0]
    a.C = C; a.Ctot = Ctot; a.c0 = c0; a.tok = const_cast<float*>(tok); a.n = n; a.ph = ph; a.pw = pw;
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 8.0 * B * (double)C * a.G, "hpx_canvas_scatter");
    hipLaunchKernelGGL(hpx_canvas_kernel<true>, canvas_grid(a, B), dim3(256), 0, (hipStream_t)stream, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}
