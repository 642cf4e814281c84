// HEALPix padding of width 1 in closed form (HEALPixPadding of src/dlwpbench/utils/healpix.py at padding = 1), shared by the
// 3 x 3 kernels (device) and dlwp_hpx_halo_sources (host), so that the rule the kernels run is testable without a GPU.
//
// A sphere is 12 square faces of n x n pixels: face f = 4 * band + k with band 0 = north, 1 = equator, 2 = south and k the
// position around the axis.  With N(q) = q mod 4, E(q) = 4 + q mod 4, S(q) = 8 + q mod 4 the neighbours of a face are
//
//            top      top-left          left     bottom-left  bottom   bottom-right      right    top-right
//   north k  N(k+1)*  N(k+2)*           N(k+3)*  N(k+3)       E(k)     S(k)              E(k+1)   N(k+1)
//   equator  N(k)     mean(N(k),N(k+3)) N(k+3)   E(k+3)       S(k+3)   mean(S(k+3),S(k)) S(k)     E(k+1)
//   south k  E(k+1)   N(k)              E(k)     S(k+3)       S(k+3)*  S(k+2)*           S(k+1)*  S(k+1)
//
// (* = seen rotated: a pole face meets its pole neighbours along edges that are rows on one side and columns on the other).
// Every cell of the one-pixel ring around a face is ONE pixel of a neighbour, except the top-left and bottom-right corner cell of
// an equatorial face, where no face exists: the mean of the two pixels that touch that corner.
#pragma once

namespace hpx {

constexpr int FACES = 12;

// Sources of the ring cell (pr, pc) of face f, in the coordinates of the PADDED face (0 .. n + 1; the cell must lie on the
// ring).  Pixel indices within the sphere, (face * n + y) * n + x; *s1 = -1 unless the cell is the mean of two pixels.
__host__ __device__ inline void halo_sources(int n, int f, int pr, int pc, int* s0, int* s1) {
    const int band = f >> 2, k = f & 3, m = n - 1, i = pr - 1, j = pc - 1;
    const bool top = pr == 0, bot = pr == n + 1, left = pc == 0, right = pc == n + 1;
    const int Nk = k, N1 = (k + 1) & 3, N2 = (k + 2) & 3, N3 = (k + 3) & 3;
    const int Ek = 4 + k, E1 = 4 + N1, E3 = 4 + N3, Sk = 8 + k, S1 = 8 + N1, S2 = 8 + N2, S3 = 8 + N3;
    int F, y, x, F2 = -1, y2 = 0, x2 = 0;
    if (band == 0) {
        if (top) { if (left) { F = N2; y = 0; x = 0; } else if (right) { F = N1; y = m; x = 0; } else { F = N1; y = j; x = 0; } }
        else if (bot) { if (left) { F = N3; y = 0; x = m; } else if (right) { F = Sk; y = 0; x = 0; } else { F = Ek; y = 0; x = j; } }
        else if (left) { F = N3; y = 0; x = i; }
        else { F = E1; y = i; x = 0; }
    } else if (band == 1) {
        if (top) {
            if (left) { F = Nk; y = m; x = 0; F2 = N3; y2 = 0; x2 = m; }
            else if (right) { F = E1; y = m; x = 0; }
            else { F = Nk; y = m; x = j; }
        } else if (bot) {
            if (left) { F = E3; y = 0; x = m; }
            else if (right) { F = S3; y = 0; x = m; F2 = Sk; y2 = m; x2 = 0; }
            else { F = S3; y = 0; x = j; }
        } else if (left) { F = N3; y = i; x = m; }
        else { F = Sk; y = i; x = 0; }
    } else {
        if (top) { if (left) { F = Nk; y = m; x = m; } else if (right) { F = S1; y = m; x = 0; } else { F = E1; y = m; x = j; } }
        else if (bot) { if (left) { F = S3; y = 0; x = m; } else if (right) { F = S2; y = m; x = m; } else { F = S3; y = j; x = m; } }
        else if (left) { F = Ek; y = i; x = m; }
        else { F = S1; y = m; x = i; }
    }
    *s0 = (F * n + y) * n + x;
    *s1 = F2 < 0 ? -1 : (F2 * n + y2) * n + x2;
}

// index of a ring cell of the padded face, 0 .. 4 n + 3: top row, bottom row, left column, right column
__host__ __device__ inline int ring_cell(int n, int pr, int pc) {
    if (pr == 0) return pc;
    if (pr == n + 1) return n + 2 + pc;
    return pc == 0 ? 2 * (n + 2) + pr - 1 : 2 * (n + 2) + n + pr - 1;
}

// index of a border pixel of the face, 0 .. 4 n - 5 (n >= 2): top row, bottom row, left column, right column
__host__ __device__ inline int ring_pixel(int n, int y, int x) {
    if (y == 0) return x;
    if (y == n - 1) return n + x;
    return x == 0 ? 2 * n + y - 1 : 2 * n + (n - 2) + y - 1;
}

}  // namespace hpx
