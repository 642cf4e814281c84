// Power spectra of forecast and target per lead time: the power per spherical-harmonic degree of fields on the sphere and the
// shell-binned spectrum E(k) of doubly periodic planes, each with the cross-spectrum between forecast and target.
//
// The reference has no spectra; correctness is defined by the float64 restatement tests/spectra_ref.py.  Everything here follows
// csrc/rollout_diag.hip: NORMALISED outputs (free batch and time strides, or NULL) and dense targets are read, nothing is
// de-normalised (a per-variable shift moves degree 0 only: the host applies it to a00), sums run in a fixed order without atomics,
// every output address has one writer, and a chunk's results are written at its global frame indices, so a rollout analysed in time
// chunks and batch chunks gives the bits of one call.
//
// ---- sphere: dlwp_sphere_spectra ----------------------------------------------------------------------------------------------------
// Operands built by the caller in float64 and rounded once: F [2 M][W], rows 2 m and 2 m + 1 = (2 pi / W) cos, -(2 pi / W) sin of
// 2 pi m n / W, and Wf [M][L][H] = P~_l^m(cos theta_k) w_k.  The kernel never evaluates a sine or a recurrence: any grid whose rows
// carry a quadrature weight is a table.
//   stage 1   T[k][m]  = sum_n F[2 m (+1)][n] x[k][n]                    (re, im) of output and target, n ascending
//   stage 2   a[l][m]  = sum_k Wf[m][l][k] T[k][m]                       k ascending
//   power     P_l      = (1 / 4 pi) sum_m c_m |a_lm|^2, c_0 = 1, c_m = 2 (cross: Re(a^out conj a^tgt))
// Decomposition.  A workgroup of 256 threads owns one (sample, frame, variable) field PAIR and a block of `mb` orders.  It walks the
// plane in blocks of `rb` latitude rows: the rows of output and target are copied to LDS (HPX: interpolated there through the 4-tap
// hpx2ll table from planes staged in LDS once, or gathered from global memory when two planes exceed HPX_LDS_BYTES -- no lat-lon
// tensor is written on either path), a thread then owns (two rows, one order) and forms T for both fields, which stays in LDS as
// [H][mb][4] (re_o, im_o, re_t, im_t).  After the last row block a thread owns (two degrees, m), reads their table rows Wf[m][l][:]
// from global memory (16-byte pieces when H % 4 == 0; the same k order either way) and the four T values of each k as ONE LDS read,
// and leaves c_m |a|^2 of both fields and the cross term in LDS [3][L][mb]; a thread per (quantity, l) adds them over m in ascending
// order.  (The 2 x 2 register tiles change no sum: every accumulator still adds its own terms in ascending n or k.)
// With one order block (every plane whose tables fit: 32 x 64 with L = M = 32 takes 48 KiB) the sum times 1 / 4 pi is the result and
// a field pair is read once; with more (mb < M) the block sums go to the workspace, spectra_fold_kernel adds them in ascending
// block order, and the pair is read once per block (served by L2: the blocks of a pair are neighbours in the grid).  No a_lm leaves the chip.
// (mb, rb) are the largest that fit SPEC_LDS_BUDGET, mb first: a function of (H, W, L, M, mesh, n) only -- never of Bc, Tc, the
// chunking or the device.  Knobs: SPEC_MB / SPEC_RB force them, SPEC_HPX the staging (1 LDS, 2 direct).
// Roof: 32 x 64, L = M = 32 is 2 x 8 KiB read per pair against 2 x 2 x (2 M W H + 2 M L H) = 0.79 MFLOP of plain fp32 FMAs (arithmetic
// intensity 48 FLOP / byte): the kernel is bound by the LDS reads that feed the vector ALU (three LDS words per four FMAs in stage 1) and by
// the reads of Wf from L2 (the whole table per workgroup), not by HBM.
//
// ---- plane: dlwp_plane_spectra ------------------------------------------------------------------------------------------------------
// dlwp_rfft2 (channels-first, norm "backward") of targets and outputs into the workspace, then plane_bin_kernel: a workgroup owns a
// field pair, a thread a shell k, and adds c |u|^2 of both fields and c Re(u^out conj u^tgt) over the shell's CSR list
// (entry index into the half spectrum [H][W/2+1], weight c) in LIST order; the sums times 1 / (H W)^2 are the result.
#include "common.hip.h"
#include "dlwpmi_internal.h"
#include "diag_stage.hip.h"
#include <algorithm>

namespace {

constexpr int SPEC_LDS_BUDGET = 64 * 1024;    // bytes of LDS of the sphere kernel, staged HPX planes included
constexpr int HPX_LDS_BYTES = 24 * 1024;      // two HPX planes are staged up to this size (HPX16), else gathered from global memory
constexpr int SPEC_MAX_H = 256, SPEC_MAX_W = 512;

struct SphArgs {
    const float *out, *target, *F, *Wf;
    const int* idx;
    const float* w;
    long long bs, ts;
    int npix, Bc, Tc, V, H, W, L, M, t_begin, T, mb, nmb, rb, vec, wvec, fs, off_t, off_a;
    float *power, *cross, *a00, *part;
};

enum { SPH_LL = 0, SPH_HPX_LDS = 1, SPH_HPX_DIRECT = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void sphere_spectra_kernel(const SphArgs a) {
    extern __shared__ __align__(16) float lds[];
    // [2 npix] staged HPX planes (SPH_HPX_LDS) | Tt [H][mb][4] | region A: Fs [2 mb][fs], rows [2][rb][W]; later red [3][L][mb]
    float* Tt = lds + a.off_t;
    float* Fs = lds + a.off_a;
    float* rows = Fs + 2 * a.mb * a.fs;
    float* red = Fs;
    const int tid = threadIdx.x;
    const int tc = blockIdx.x / a.nmb, j = blockIdx.x - tc * a.nmb, v = blockIdx.y, b = blockIdx.z;
    const int m0 = j * a.mb, mbk = min(a.mb, a.M - m0), nq = 2 * mbk;
    const int H = a.H, W = a.W, L = a.L;
    const bool has_out = a.out != nullptr;
    const float* op = has_out ? a.out + b * a.bs + tc * a.ts + (long long)v * a.npix : nullptr;
    const float* tp = a.target + (((long long)b * a.Tc + tc) * a.V + v) * a.npix;

    for (int e = tid; e < nq * W; e += 256) {                // the block's rows of F
        const int q = e / W, n = e - q * W;
        Fs[q * a.fs + n] = a.F[(long long)(2 * m0 + q) * W + n];
    }
    const float *so = op, *st = tp;
    if constexpr (MODE == SPH_HPX_LDS) {
        stage_group(lds, op, 0, tp, 0, 1, a.npix, a.vec);
        so = lds, st = lds + a.npix;
    }
    __syncthreads();

    for (int r0 = 0; r0 < H; r0 += a.rb) {
        const int rbk = min(a.rb, H - r0);
        for (int e = tid; e < rbk * W; e += 256) {           // rows r0 .. r0 + rbk - 1 of both fields
            const int p = r0 * W + e;
            float xo = 0.f, xt;
            if constexpr (MODE == SPH_LL) {
                xt = tp[p];
                if (has_out) xo = op[p];
            } else {
                const int4 i4 = reinterpret_cast<const int4*>(a.idx)[p];
                const float4 w4 = reinterpret_cast<const float4*>(a.w)[p];
                xt = tap4(st, i4, w4);
                if (has_out) xo = tap4(so, i4, w4);
            }
            rows[e] = xo;
            rows[a.rb * W + e] = xt;
        }
        __syncthreads();
        // stage 1: a thread owns two rows x one order (cos and sin row of F) x both fields: six LDS words feed eight multiply-adds;
        // every sum runs over n ascending.  An odd tail row is computed twice and written once
        const int nrp = (rbk + 1) >> 1;
        for (int e = tid; e < nrp * mbk; e += 256) {
            const int kp = e / mbk, mi = e - kp * mbk;
            const int k0 = 2 * kp, k1 = min(k0 + 1, rbk - 1);
            const float* fr = Fs + 2 * mi * a.fs;
            const float* fi = fr + a.fs;
            const float *xo0 = rows + k0 * W, *xo1 = rows + k1 * W, *xt0 = xo0 + a.rb * W, *xt1 = xo1 + a.rb * W;
            float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;      // (re_o, im_o, re_t, im_t) of row k0 and of row k1
            for (int n = 0; n < W; ++n) {
                const float c = fr[n], s = fi[n], a0 = xo0[n], b0 = xt0[n], a1 = xo1[n], b1 = xt1[n];
                s0.x = fmaf(c, a0, s0.x), s0.y = fmaf(s, a0, s0.y), s0.z = fmaf(c, b0, s0.z), s0.w = fmaf(s, b0, s0.w);
                s1.x = fmaf(c, a1, s1.x), s1.y = fmaf(s, a1, s1.y), s1.z = fmaf(c, b1, s1.z), s1.w = fmaf(s, b1, s1.w);
            }
            reinterpret_cast<float4*>(Tt)[(r0 + k0) * a.mb + mi] = s0;
            if (k0 + 1 < rbk) reinterpret_cast<float4*>(Tt)[(r0 + k0 + 1) * a.mb + mi] = s1;
        }
        __syncthreads();                                     // the next block overwrites the rows; stage 2 reads Tt and overwrites region A
    }

    // stage 2: a thread owns two degrees x one order: one 16-byte LDS read of T[k][m] feeds eight multiply-adds; k ascending.  An odd
    // tail degree is computed twice and written once
    const int nlp = (L + 1) >> 1;
    for (int e = tid; e < nlp * mbk; e += 256) {
        const int mi = e / nlp, lp = e - mi * nlp, m = m0 + mi;
        const int l0 = 2 * lp, l1 = min(l0 + 1, L - 1);
        const float* w0 = a.Wf + ((long long)m * L + l0) * H;
        const float* w1 = a.Wf + ((long long)m * L + l1) * H;
        const float4* t4 = reinterpret_cast<const float4*>(Tt) + mi;
        float4 c0 = make_float4(0.f, 0.f, 0.f, 0.f), c1 = c0;          // (re_o, im_o, re_t, im_t) of a[l0][m] and a[l1][m]
        auto step = [&](float u0, float u1, int k) {
            const float4 t = t4[k * a.mb];
            c0.x = fmaf(u0, t.x, c0.x), c0.y = fmaf(u0, t.y, c0.y), c0.z = fmaf(u0, t.z, c0.z), c0.w = fmaf(u0, t.w, c0.w);
            c1.x = fmaf(u1, t.x, c1.x), c1.y = fmaf(u1, t.y, c1.y), c1.z = fmaf(u1, t.z, c1.z), c1.w = fmaf(u1, t.w, c1.w);
        };
        if (a.wvec) {
            for (int k = 0; k < H; k += 4) {
                const float4 p = *reinterpret_cast<const float4*>(w0 + k), q = *reinterpret_cast<const float4*>(w1 + k);
                step(p.x, q.x, k), step(p.y, q.y, k + 1), step(p.z, q.z, k + 2), step(p.w, q.w, k + 3);
            }
        } else {
            for (int k = 0; k < H; ++k) step(w0[k], w1[k], k);
        }
        const float c = m == 0 ? 1.f : 2.f;
        auto leave = [&](int l, const float4 x) {
            red[(0 * L + l) * a.mb + mi] = c * (x.x * x.x + x.y * x.y);
            red[(1 * L + l) * a.mb + mi] = c * (x.z * x.z + x.w * x.w);
            red[(2 * L + l) * a.mb + mi] = c * (x.x * x.z + x.y * x.w);
        };
        leave(l0, c0);
        if (l0 + 1 < L) leave(l0 + 1, c1);
        if (m == 0 && l0 == 0) {                             // a00 [2][Bc][T][V]
            const long long z = ((long long)b * a.T + a.t_begin + tc) * a.V + v;
            a.a00[z] = c0.x;
            a.a00[z + (long long)a.Bc * a.T * a.V] = c0.z;
        }
    }
    __syncthreads();
    const float inv4pi = 0.07957747154594767f;
    for (int e = tid; e < 3 * L; e += 256) {                 // (quantity, l): the orders of the block in ascending order
        const int which = e / L, l = e - which * L;
        float s = 0.f;
        for (int mi = 0; mi < mbk; ++mi) s += red[e * a.mb + mi];
        if (a.nmb == 1) {
            const long long z = (((long long)b * a.T + a.t_begin + tc) * a.V + v) * L + l;
            if (which == 2) a.cross[z] = s * inv4pi;
            else a.power[z + (long long)which * a.Bc * a.T * a.V * L] = s * inv4pi;
        } else {                                             // part [Bc][Tc][V][nmb][3][L]
            a.part[(((((long long)b * a.Tc + tc) * a.V + v) * a.nmb + j) * 3 + which) * L + l] = s;
        }
    }
}

// power / cross <- the order blocks' sums in ascending block order, times 1 / 4 pi
__global__ __launch_bounds__(256) void spectra_fold_kernel(const float* __restrict__ part, float* power, float* cross, long long n, int Bc,
                                                           int Tc, int V, int L, int nmb, int t_begin, int T) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;      // e = (((b Tc + tc) V + v) 3 + which) L + l
    if (e >= n) return;
    const int l = (int)(e % L);
    long long q = e / L;
    const int which = (int)(q % 3);
    q /= 3;                                                  // (b Tc + tc) V + v
    const int v = (int)(q % V);
    const long long bt = q / V;
    const int tc = (int)(bt % Tc);
    const long long b = bt / Tc;
    float s = 0.f;
    for (int jb = 0; jb < nmb; ++jb) s += part[((q * nmb + jb) * 3 + which) * L + l];
    const long long z = ((b * T + t_begin + tc) * V + v) * L + l;
    const float r = s * 0.07957747154594767f;
    if (which == 2) cross[z] = r;
    else power[z + (long long)which * Bc * T * V * L] = r;
}

struct PlaneArgs {
    const float *so, *st;       // half spectra [fields][H][W/2+1][2] of outputs (or NULL) and targets
    const int *rowptr, *entry;
    const float* weight;
    int K, nnz, NS, Bc, Tc, D, t_begin, T;
    float inv;                  // 1 / (H W)^2
    float *power, *cross;
};

__global__ __launch_bounds__(256) void plane_bin_kernel(const PlaneArgs a) {
    const long long f = blockIdx.x;                          // f = (b Tc + tc) D + d
    const int d = (int)(f % a.D);
    const long long bt = f / a.D;
    const int tc = (int)(bt % a.Tc);
    const long long b = bt / a.Tc;
    const float2* uo = a.so ? reinterpret_cast<const float2*>(a.so) + f * a.NS : nullptr;
    const float2* ut = reinterpret_cast<const float2*>(a.st) + f * a.NS;
    for (int k = threadIdx.x; k < a.K; k += 256) {
        const int e0 = min(max(a.rowptr[k], 0), a.nnz), e1 = min(max(a.rowptr[k + 1], e0), a.nnz);
        float po = 0.f, pt = 0.f, cr = 0.f;
        for (int e = e0; e < e1; ++e) {                      // list order
            const int i = min(max(a.entry[e], 0), a.NS - 1);      // (0 <= entry < NS is the caller's precondition; never an address outside the spectrum)
            const float c = a.weight[e];
            const float2 y = ut[i];
            const float2 x = uo ? uo[i] : make_float2(0.f, 0.f);
            po = fmaf(c, x.x * x.x + x.y * x.y, po);
            pt = fmaf(c, y.x * y.x + y.y * y.y, pt);
            cr = fmaf(c, x.x * y.x + x.y * y.y, cr);
        }
        const long long z = (((long long)b * a.T + a.t_begin + tc) * a.D + d) * a.K + k;
        a.power[z] = po * a.inv;
        a.power[z + (long long)a.Bc * a.T * a.D * a.K] = pt * a.inv;
        a.cross[z] = cr * a.inv;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct SphShape {
    int mb, nmb, rb, fs, hpx_lds, off_t, off_a;
    size_t bytes;
};

long long sph_floats(int H, int W, int L, int mb, int rb, int fs, int planes) {
    const long long region_a = std::max<long long>(2LL * mb * fs + 2LL * rb * W, 3LL * L * mb);
    return planes + 4LL * H * mb + region_a;
}

// (orders per block, rows per block, staging): the largest that fit SPEC_LDS_BUDGET, orders first.  A function of the shape only.
int sph_shape(const char* who, int H, int W, int L, int M, bool hpx, int n, SphShape* s) {
    const int f_mb = dlwp_tune_or("SPEC_MB", 0), f_rb = dlwp_tune_or("SPEC_RB", 0), f_hpx = dlwp_tune_or("SPEC_HPX", 0);
    DLWP_REQUIRE(f_mb >= 0 && f_rb >= 0 && f_hpx >= 0 && f_hpx <= 2, DLWP_E_INVALID,
                 "%s: SPEC_MB %d, SPEC_RB %d must not be negative and SPEC_HPX %d must be 0 (auto), 1 (LDS) or 2 (direct)", who, f_mb, f_rb, f_hpx);
    const long long npix = hpx ? 12LL * n * n : 0;
    const bool fits = 8 * npix <= HPX_LDS_BYTES;
    DLWP_REQUIRE(!hpx || f_hpx != 1 || fits, DLWP_E_UNSUPPORTED, "%s: SPEC_HPX=1 but two planes of %lld floats do not fit %d bytes of LDS", who,
                 npix, HPX_LDS_BYTES);
    s->hpx_lds = hpx && (f_hpx == 1 || (f_hpx == 0 && fits));
    const int planes = s->hpx_lds ? (int)round_up((int)(2 * npix), 4) : 0;
    s->fs = W | 1;                                           // odd row pitch of F in LDS: the lanes of a wave read distinct banks
    int mb = f_mb ? std::min(f_mb, M) : M, rb = f_rb ? std::min(f_rb, H) : H;
    for (;;) {
        if (4 * sph_floats(H, W, L, mb, rb, s->fs, planes) <= SPEC_LDS_BUDGET) break;
        if (!f_rb && rb > 1) rb = (rb + 1) / 2;
        else if (!f_mb && mb > 1) mb = (mb + 1) / 2, rb = f_rb ? rb : H;
        else {
            dlwp_set_error("%s: SPEC_MB %d / SPEC_RB %d need %lld bytes of LDS, above %d", who, f_mb, f_rb,
                           4 * sph_floats(H, W, L, mb, rb, s->fs, planes), SPEC_LDS_BUDGET);
            return DLWP_E_UNSUPPORTED;
        }
    }
    s->mb = mb, s->rb = rb, s->nmb = ceil_div(M, mb);
    s->off_t = planes, s->off_a = planes + 4 * H * mb;
    s->bytes = 4 * (size_t)sph_floats(H, W, L, mb, rb, s->fs, planes);
    return DLWP_OK;
}

int sph_check_shape(const char* who, int Bc, int Tc, int V, int H, int W, int L, int M) {
    DLWP_REQUIRE(Bc > 0 && Tc > 0 && V > 0 && H > 0 && W > 0 && L > 0 && M > 0, DLWP_E_INVALID,
                 "%s: Bc %d, Tc %d, V %d, H %d, W %d, L %d, M %d must be positive", who, Bc, Tc, V, H, W, L, M);
    DLWP_REQUIRE(H <= SPEC_MAX_H, DLWP_E_UNSUPPORTED, "%s: H %d above %d rows", who, H, SPEC_MAX_H);
    DLWP_REQUIRE(W <= SPEC_MAX_W, DLWP_E_UNSUPPORTED, "%s: W %d above %d columns", who, W, SPEC_MAX_W);
    DLWP_REQUIRE(L <= H, DLWP_E_INVALID, "%s: L %d degrees above H %d rows", who, L, H);
    DLWP_REQUIRE(2 * M <= W, DLWP_E_INVALID, "%s: M %d orders above W / 2 = %d (the Nyquist order is left out)", who, M, W / 2);
    DLWP_REQUIRE(V <= 65535 && Bc <= 65535, DLWP_E_UNSUPPORTED, "%s: grid limits (V %d, Bc %d above 65535)", who, V, Bc);
    return DLWP_OK;
}

}  // namespace

extern "C" long long dlwp_sphere_spectra_ws_floats(int Bc, int Tc, int V, int H, int W, int L, int M, int n) {
    int rc = sph_check_shape("sphere_spectra_ws_floats", Bc, Tc, V, H, W, L, M);
    if (rc) return rc;
    if (n < 0 || n > 8192) {
        dlwp_set_error("sphere_spectra_ws_floats: nside n %d must lie in 0 (lat-lon) .. 8192", n);
        return DLWP_E_INVALID;
    }
    SphShape s;
    rc = sph_shape("sphere_spectra_ws_floats", H, W, L, M, n > 0, n, &s);
    if (rc) return rc;
    return s.nmb == 1 ? 1 : (long long)Bc * Tc * V * s.nmb * 3 * L;      // (never 0: the caller allocates it)
}

extern "C" int dlwp_sphere_spectra(const float* out, long long out_bstride, long long out_tstride, const float* target, const float* F,
                                   const float* Wf, const int* idx, const float* w, int n, int Bc, int Tc, int V, int H, int W, int L,
                                   int M, int t_begin, int T, float* power, float* cross, float* a00, float* ws, void* stream) {
    DLWP_REQUIRE(target, DLWP_E_INVALID, "sphere_spectra: target is NULL");
    DLWP_REQUIRE(F, DLWP_E_INVALID, "sphere_spectra: F is NULL");
    DLWP_REQUIRE(Wf, DLWP_E_INVALID, "sphere_spectra: Wf is NULL");
    DLWP_REQUIRE(power, DLWP_E_INVALID, "sphere_spectra: power is NULL");
    DLWP_REQUIRE(cross, DLWP_E_INVALID, "sphere_spectra: cross is NULL");
    DLWP_REQUIRE(a00, DLWP_E_INVALID, "sphere_spectra: a00 is NULL");
    DLWP_REQUIRE(ws, DLWP_E_INVALID, "sphere_spectra: ws is NULL (dlwp_sphere_spectra_ws_floats gives its size)");
    DLWP_REQUIRE((idx != nullptr) == (w != nullptr), DLWP_E_INVALID, "sphere_spectra: the hpx2ll table needs both idx and w, not one (NULL idx %d, NULL w %d)",
                 idx == nullptr, w == nullptr);
    const bool hpx = idx != nullptr;
    int rc = sph_check_shape("sphere_spectra", Bc, Tc, V, H, W, L, M);
    if (rc) return rc;
    DLWP_REQUIRE(T > 0, DLWP_E_INVALID, "sphere_spectra: T %d must be positive", T);
    DLWP_REQUIRE(!hpx || n > 0, DLWP_E_INVALID, "sphere_spectra: nside n %d must be positive with an hpx2ll table", n);
    DLWP_REQUIRE(!hpx || n <= 8192, DLWP_E_UNSUPPORTED, "sphere_spectra: n %d above 8192", n);
    DLWP_REQUIRE(out_bstride >= 0 && out_tstride >= 0, DLWP_E_INVALID, "sphere_spectra: negative stride of out (batch %lld, time %lld)",
                 out_bstride, out_tstride);
    DLWP_REQUIRE(t_begin >= 0 && (long long)t_begin + Tc <= T, DLWP_E_INVALID, "sphere_spectra: chunk t_begin %d + Tc %d is outside the rollout T %d",
                 t_begin, Tc, T);
    DLWP_REQUIRE(!hpx || (aligned16(idx) && aligned16(w)), DLWP_E_INVALID, "sphere_spectra: idx and w must be 16-byte aligned");
    SphShape s;
    rc = sph_shape("sphere_spectra", H, W, L, M, hpx, n, &s);
    if (rc) return rc;
    DLWP_REQUIRE((long long)Tc * s.nmb <= INT_MAX, DLWP_E_UNSUPPORTED, "sphere_spectra: Tc %d x %d order blocks are too many workgroups", Tc, s.nmb);
    SphArgs a;
    a.out = out, a.target = target, a.F = F, a.Wf = Wf, a.idx = idx, a.w = w, a.bs = out_bstride, a.ts = out_tstride;
    a.npix = hpx ? 12 * n * n : H * W;
    a.Bc = Bc, a.Tc = Tc, a.V = V, a.H = H, a.W = W, a.L = L, a.M = M, a.t_begin = t_begin, a.T = T;
    a.mb = s.mb, a.nmb = s.nmb, a.rb = s.rb, a.fs = s.fs, a.off_t = s.off_t, a.off_a = s.off_a;
    a.vec = (!out || (aligned16(out) && out_bstride % 4 == 0 && out_tstride % 4 == 0)) && aligned16(target) && a.npix % 4 == 0;
    a.wvec = H % 4 == 0 && aligned16(Wf);
    a.power = power, a.cross = cross, a.a00 = a00, a.part = ws;
    const int mode = !hpx ? SPH_LL : s.hpx_lds ? SPH_HPX_LDS : SPH_HPX_DIRECT;
    const double fields = (double)Bc * Tc * V;
    const double flops = fields * 2.0 * (2.0 * 2 * M * (double)W * H + 2.0 * 2 * M * (double)L * H);
    const double bytes = 4.0 * fields * a.npix * (out ? 2 : 1) + 4.0 * fields * 3 * L;
    {
        dlwp_prof_scope prof((hipStream_t)stream, flops, bytes, "%s",
                             mode == SPH_LL ? "sphere_spectra_ll" : mode == SPH_HPX_LDS ? "sphere_spectra_hpx_lds" : "sphere_spectra_hpx_direct");
        const dim3 grid((unsigned)(Tc * s.nmb), V, Bc);
#define DLWP_SPH_LAUNCH(MODE_)                                                                                           \
    do {                                                                                                                 \
        rc = dlwp_ensure_lds((const void*)sphere_spectra_kernel<MODE_>, s.bytes, "sphere_spectra");                      \
        if (rc) return rc;                                                                                               \
        hipLaunchKernelGGL((sphere_spectra_kernel<MODE_>), grid, dim3(256), s.bytes, (hipStream_t)stream, a);            \
    } while (0)
        if (mode == SPH_LL) DLWP_SPH_LAUNCH(SPH_LL);
        else if (mode == SPH_HPX_LDS) DLWP_SPH_LAUNCH(SPH_HPX_LDS);
        else DLWP_SPH_LAUNCH(SPH_HPX_DIRECT);
#undef DLWP_SPH_LAUNCH
        DLWP_LAUNCH_CHECK();
    }
    if (s.nmb > 1) {
        const long long nf = (long long)Bc * Tc * V * 3 * L;
        DLWP_REQUIRE((nf + 255) / 256 <= INT_MAX, DLWP_E_UNSUPPORTED, "sphere_spectra: %lld sums are too many", nf);
        dlwp_prof_scope prof((hipStream_t)stream, 0.0, 4.0 * nf * (s.nmb + 1), "sphere_spectra_fold");
        hipLaunchKernelGGL(spectra_fold_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, power, cross, nf,
                           Bc, Tc, V, L, s.nmb, t_begin, T);
        DLWP_LAUNCH_CHECK();
    }
    return DLWP_OK;
}

namespace {
int plane_check_shape(const char* who, int Bc, int Tc, int D, int H, int W) {
    DLWP_REQUIRE(Bc > 0 && Tc > 0 && D > 0 && H > 0 && W > 1, DLWP_E_INVALID, "%s: Bc %d, Tc %d, D %d, H %d must be positive and W %d at least 2", who,
                 Bc, Tc, D, H, W);
    DLWP_REQUIRE((long long)Bc * Tc * D <= INT_MAX && (long long)H * (W / 2 + 1) <= INT_MAX / 4, DLWP_E_UNSUPPORTED,
                 "%s: grid limits (%lld fields, or a half spectrum of %d x %d)", who, (long long)Bc * Tc * D, H, W / 2 + 1);
    return DLWP_OK;
}
}  // namespace

extern "C" long long dlwp_plane_spectra_ws_floats(int Bc, int Tc, int D, int H, int W) {
    const int rc = plane_check_shape("plane_spectra_ws_floats", Bc, Tc, D, H, W);
    if (rc) return rc;
    return 2LL * Bc * Tc * D * H * (W / 2 + 1) * 2;          // the half spectra of one chunk of outputs and targets
}

extern "C" int dlwp_plane_spectra(const dlwp_fft_plan* plan, const float* out, long long out_bstride, long long out_tstride,
                                  const float* target, const int* rowptr, const int* entry, const float* weight, int K, int nnz, int Bc,
                                  int Tc, int D, int H, int W, int t_begin, int T, float* power, float* cross, float* ws, void* stream) {
    DLWP_REQUIRE(plan, DLWP_E_INVALID, "plane_spectra: plan is NULL");
    DLWP_REQUIRE(target, DLWP_E_INVALID, "plane_spectra: target is NULL");
    DLWP_REQUIRE(rowptr, DLWP_E_INVALID, "plane_spectra: rowptr is NULL");
    DLWP_REQUIRE(entry, DLWP_E_INVALID, "plane_spectra: entry is NULL");
    DLWP_REQUIRE(weight, DLWP_E_INVALID, "plane_spectra: weight is NULL");
    DLWP_REQUIRE(power, DLWP_E_INVALID, "plane_spectra: power is NULL");
    DLWP_REQUIRE(cross, DLWP_E_INVALID, "plane_spectra: cross is NULL");
    DLWP_REQUIRE(ws, DLWP_E_INVALID, "plane_spectra: ws is NULL (dlwp_plane_spectra_ws_floats gives its size)");
    int rc = plane_check_shape("plane_spectra", Bc, Tc, D, H, W);
    if (rc) return rc;
    DLWP_REQUIRE(K > 0 && nnz > 0 && T > 0, DLWP_E_INVALID, "plane_spectra: K %d shells, nnz %d entries, T %d must be positive", K, nnz, T);
    DLWP_REQUIRE(out_bstride >= 0 && out_tstride >= 0, DLWP_E_INVALID, "plane_spectra: negative stride of out (batch %lld, time %lld)",
                 out_bstride, out_tstride);
    DLWP_REQUIRE(t_begin >= 0 && (long long)t_begin + Tc <= T, DLWP_E_INVALID, "plane_spectra: chunk t_begin %d + Tc %d is outside the rollout T %d",
                 t_begin, Tc, T);
    const long long NS = (long long)H * (W / 2 + 1), plane = (long long)D * H * W, fields = (long long)Bc * Tc * D;
    float* st = ws + fields * NS * 2;                        // ws: [outputs | targets]
    rc = dlwp_rfft2(plan, target, st, Bc * Tc, D, 1, 0, 0, stream);      // (a plan made for H x W is the caller's precondition)
    if (rc) return rc;
    if (out) {
        if (out_tstride == plane && out_bstride == plane * Tc) {
            rc = dlwp_rfft2(plan, out, ws, Bc * Tc, D, 1, 0, 0, stream);
            if (rc) return rc;
        } else {                                             // a strided view (a time slice, the persistence forecast): frame by frame
            for (int b = 0; b < Bc; ++b)
                for (int t = 0; t < Tc; ++t) {
                    rc = dlwp_rfft2(plan, out + b * out_bstride + t * out_tstride, ws + ((long long)b * Tc + t) * D * NS * 2, 1, D, 1, 0, 0, stream);
                    if (rc) return rc;
                }
        }
    }
    PlaneArgs a;
    a.so = out ? ws : nullptr, a.st = st, a.rowptr = rowptr, a.entry = entry, a.weight = weight;
    a.K = K, a.nnz = nnz, a.NS = (int)NS, a.Bc = Bc, a.Tc = Tc, a.D = D, a.t_begin = t_begin, a.T = T;
    a.inv = (float)(1.0 / ((double)H * W * (double)H * W));
    a.power = power, a.cross = cross;
    dlwp_prof_scope prof((hipStream_t)stream, 0.0, 8.0 * fields * NS * (out ? 2 : 1) + 12.0 * fields * K, "plane_spectra_bin");
    hipLaunchKernelGGL(plane_bin_kernel, dim3((unsigned)fields), dim3(256), 0, (hipStream_t)stream, a);
    DLWP_LAUNCH_CHECK();
    return DLWP_OK;
}
