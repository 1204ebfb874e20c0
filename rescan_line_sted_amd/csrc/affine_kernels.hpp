// affine_kernels.hpp -- rotation, scale and shear between views (rl_warp_images, rl_affine_sums, include/rlsted.h; DESIGN.md section
// 4n): the thread bodies of affine_kernels.hip, written as host-compilable templates so that the CPU tests run the very same code
// (tests/emu/warp_emu.cpp), the host builder of the prefilter's taps, and the launchers.
//
// WARP  dst[i][y][x] = max(spline of src[i] at (Y, X), floor) for an output grid of oy x ox pixels that is independent of the source's
//   sy x sx:  Y = fma(m00, y, fma(m01, x, o0)),  X = fma(m10, y, fma(m11, x, o1)),  xf[i] = (m00, m01, m10, m11, o0, o1) -- that is
//   scipy.ndimage.affine_transform(src[i], [[m00, m01], [m10, m11]], offset = (o0, o1), output_shape = (oy, ox), order, mode = 'mirror').
//   ORDER 3  the spline coefficients c are the prefilter alone, along x and then along y: per axis the FIR h[k] = sqrt(3) z^|k|,
//     z = sqrt(3) - 2, |k| <= K = 30 (61 taps, tap m reads sample mirror(. - K + m)) on the whole-sample mirror extension -- the
//     impulse response shift_taps folds its evaluation weights into, here on its own (warp_prefilter_taps, long double, rounded once)
//     -- run by k_shift_pass of register_kernels.hip with that tap table (acc = h[0] v_0, then fma(h[m], v_m, acc) for m = 1, 2, ...;
//     the dropped tail is at most 8.8e-18 max|src| per axis).  EVALUATION, per output pixel and per axis, every operation rounded on
//     its own (no contraction) unless written as fma:
//         F = floor(Y),  t = Y - F (exact),  u = 1 - t,  s = 1.0 / 6.0 (the double nearest 1/6)
//         w_0 = ((u u) u) s    w_1 = (((t t) (t - 2)) 3 + 4) s    w_2 = (((u u) (u - 2)) 3 + 4) s    w_3 = ((t t) t) s
//     at the offsets -1 .. 2 from F (wy from Y, wx from X).  With c_ij the coefficient at (mirror(Fy - 1 + i), mirror(Fx - 1 + j)):
//         r_i = wx_0 c_i0,  r_i = fma(wx_j, c_ij, r_i) for j = 1, 2, 3;      v = wy_0 r_0,  v = fma(wy_i, r_i, v) for i = 1, 2, 3
//   ORDER 1  w = (1 - t, t) at the offsets 0, 1 read from src itself: r_i = (1 - tx) s_i0, and r_i = fma(tx, s_i1, r_i) ONLY where
//     tx != 0; v = (1 - ty) r_0, and v = fma(ty, r_1, v) ONLY where ty != 0 (row 1 is then not formed at all).  A weight that is exactly
//     0 does not read its sample, so an integer translation is a bit-exact copy of the displaced pixels, as in rl_shift_images; and
//     diag(2, 2) with offset (0.5, 0.5) is the 2 x 2 mean (0.5 (0.5 a + 0.5 b) + ...: exact halves).
//   Then v < floor: floor, counted; one rounding to the destination type.
//   MIRROR  a coordinate is at most 1e9 in magnitude (the call checks the four corners of the output grid, and the map is affine), so
//     F converts exactly to a 32-bit integer; index i of an axis of n samples folds to i mod 2 (n - 1) (into [0, 2 (n - 1))), then
//     p - i where that is >= n; n = 1: 0.
//   WORK SPLIT  a workgroup of 256 threads per output tile of 32 x 32 pixels, thread t the column t mod 32 and the rows t / 32 + 8 k.
//     The tile's source footprint is the bounding box of its four corners' (Y, X) -- floor(min) - 1 .. floor(max) + 1, which covers the
//     coordinates' rounding -- widened by the spline's reach (order 3: -1 .. +2, order 1: 0 .. +1).  When its rows x columns are at
//     most kWarpLds = 6144 doubles (48 KB) it is staged once in LDS as float64, the mirror rule applied at staging (row stride = the
//     box's columns; lanes read neighbouring doubles); otherwise every sample is read from global memory through the mirror rule.  Both
//     paths run warp_pixel with another fetch: the same arithmetic in the same order, the same bits.  Any rotation of a 32 x 32 tile
//     (at most 31 sqrt(2) + 7 = 51 rows and columns) and 2 x binning (66 x 66) are staged.
//   STATISTICS per image, as rl_shift_images: the count of raised pixels and the sum of the stored values (widened to float64): a
//     thread over its outputs in increasing row order, the ingest kernels' tree over the 256 threads, the workgroups in increasing
//     order (k_warp_totals).  No atomics.
//
// AFFINE SUMS  For a pair (A, W) of ny x nx images -- A the reference, W the moving image already warped by the current estimate -- and
//   the interior I = [M, ny - M) x [M, nx - M), M >= 1, every value widened to float64:
//       gy = 0.5 (W[y+1][x] - W[y-1][x])    gx = 0.5 (W[y][x+1] - W[y][x-1])    w = W[y][x]    a = A[y][x]
//       yc = (double)y - 0.5 (double)(ny - 1)    xc = (double)x - 0.5 (double)(nx - 1)            (exact)
//       phi = (gy, gx, gy yc, gy xc, gx yc, gx xc, w, 1)                                          (each product rounded on its own)
//   the kAffFields = 45 sums over I:  [0, 36) the upper triangle of sum phi phi^T in row-major order (j <= k), fma(phi_j, phi_k, .);
//   [36, 44) sum phi_j a, fma(phi_j, a, .);  [44] sum a^2, fma(a, a, .).  ORDER OF EVERY SUM: the interior's n = (ny - 2 M)(nx - 2 M)
//   pixels in row-major order are cut into nb = aff_blocks(n) runs of ceil(n / nb) pixels, a workgroup of 256 threads per (pair, run);
//     thread     from 0.0 over the pixels t, t + 256, ... of its run in increasing order, its 45 sums in registers
//     workgroup  the tree s[t] = s[t] + s[t + h] for t < h, h = 128, ..., 1 (nine fields at a time through LDS)
//     pair       (((0.0 + run_0) + run_1) + ...) over the runs in increasing order (k_affine_totals)
//   No atomics: bit-identical from run to run, and a pair's numbers do not depend on the other pairs of a call.  Nothing outside an
//   image is read (M >= 1).  16 bytes of new data per pixel against about 60 fused multiply-adds.
#pragma once
#include "register_kernels.hpp"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rl {

// ---- WARP ------------------------------------------------------------------------------------------------------------------------
constexpr int kWarpTW = 32;          // output columns of a tile
constexpr int kWarpTH = 32;          // output rows of a tile
constexpr int kWarpLds = 6144;       // doubles a staged footprint may take (48 KB)
constexpr int kWarpFields = 2;       // raised, sum (RL_SHIFT_FIELDS)
constexpr int kWarpXf = 6;           // m00, m01, m10, m11, o0, o1
constexpr double kWarpMaxCoord = 1e9;
constexpr int kWarpPrefilterTaps = 2 * kShiftK + 1;

// the prefilter's taps for an axis of n samples: g[0 .. 61), tap m reads sample mirror(k + *off + m), *off = -K reduced
inline void warp_prefilter_taps(int n, double* g, int* off, int* nt) {
    const long double r3 = sqrtl(3.0L), z = r3 - 2.0L;
    long double h[kShiftK + 1];
    h[0] = r3;
    for (int k = 1; k <= kShiftK; ++k) h[k] = h[k - 1] * z;
    for (int j = 0; j < kWarpPrefilterTaps; ++j) g[j] = (double)h[j < kShiftK ? kShiftK - j : j - kShiftK];
    for (int j = kWarpPrefilterTaps; j < kShiftTaps; ++j) g[j] = 0.0;
    *nt = kWarpPrefilterTaps;
    const long long p = n > 1 ? 2LL * (n - 1) : 1;
    *off = (int)(((-(long long)kShiftK % p) + p) % p);
}

RL_HD int warp_mirror(int i, int n) {    // scipy 'mirror' (d c b | a b c d | c b a) for any i
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i = i % p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

RL_HD void warp_coord(const double* m, int y, int x, double& Y, double& X) {
    Y = __builtin_fma(m[0], (double)y, __builtin_fma(m[1], (double)x, m[4]));
    X = __builtin_fma(m[2], (double)y, __builtin_fma(m[3], (double)x, m[5]));
}

struct WarpArgs {
    const void* src;            // [n][sy][sx]: order 1 the images, order 3 their float64 coefficients
    void* dst;                  // [n][oy][ox]
    const double* xf;           // [n][6] (device)
    double* part;               // [n][blocks][2], or nullptr
    int n, sy, sx, oy, ox, order;
    int direct;                 // 1: no tile is staged
    double floor;
};
template <typename TS, typename TD>
struct WarpParams {
    const TS* src;
    TD* dst;
    const double* xf;
    double* part;
    int sy, sx, oy, ox, nby, nbx, direct;
    double floor;
};
RL_HD int warp_blocks_y(int oy) { return (oy + kWarpTH - 1) / kWarpTH; }
RL_HD int warp_blocks_x(int ox) { return (ox + kWarpTW - 1) / kWarpTW; }
template <typename TS, typename TD>
inline WarpParams<TS, TD> warp_params(const WarpArgs& a) {
    WarpParams<TS, TD> p;
    p.src = (const TS*)a.src; p.dst = (TD*)a.dst; p.xf = a.xf; p.part = a.part; p.sy = a.sy; p.sx = a.sx; p.oy = a.oy; p.ox = a.ox;
    p.nby = warp_blocks_y(a.oy); p.nbx = warp_blocks_x(a.ox); p.direct = a.direct; p.floor = a.floor;
    return p;
}

struct WarpBox {                // a tile's footprint in unfolded source indices
    int y0, x0, rows, cols;
    bool staged;
};

// the footprint of output tile (by, bx) under the map m; ORDER's reach included
template <int ORDER>
RL_HD WarpBox warp_box(const double* m, int oy, int ox, int by, int bx, int direct) {
    const int ya = by * kWarpTH, xa = bx * kWarpTW;
    const int yb = (ya + kWarpTH < oy ? ya + kWarpTH : oy) - 1, xb = (xa + kWarpTW < ox ? xa + kWarpTW : ox) - 1;
    double Y[4], X[4];
    warp_coord(m, ya, xa, Y[0], X[0]);
    warp_coord(m, ya, xb, Y[1], X[1]);
    warp_coord(m, yb, xa, Y[2], X[2]);
    warp_coord(m, yb, xb, Y[3], X[3]);
    double ylo = Y[0], yhi = Y[0], xlo = X[0], xhi = X[0];
    for (int k = 1; k < 4; ++k) {
        ylo = Y[k] < ylo ? Y[k] : ylo; yhi = Y[k] > yhi ? Y[k] : yhi;
        xlo = X[k] < xlo ? X[k] : xlo; xhi = X[k] > xhi ? X[k] : xhi;
    }
    const int lo = ORDER == 3 ? 2 : 1, hi = ORDER == 3 ? 3 : 2;      // one index for the rounding, then the reach
    WarpBox b;
    b.y0 = (int)floor(ylo) - lo; b.x0 = (int)floor(xlo) - lo;
    const long long rows = (long long)floor(yhi) + hi - b.y0 + 1, cols = (long long)floor(xhi) + hi - b.x0 + 1;
    b.staged = !direct && rows * cols <= kWarpLds;
    b.rows = b.staged ? (int)rows : 0; b.cols = b.staged ? (int)cols : 0;
    return b;
}

// thread t's share of staging the footprint: lds[r * cols + c] = src[mirror(y0 + r)][mirror(x0 + c)] as float64
template <typename TS>
RL_HD void warp_stage(const TS* s, int sy, int sx, const WarpBox& b, int t, double* lds) {
    for (int e = t; e < b.rows * b.cols; e += kRegThreads) {
        const int r = e / b.cols, c = e - r * b.cols;
        lds[e] = (double)s[(size_t)warp_mirror(b.y0 + r, sy) * sx + warp_mirror(b.x0 + c, sx)];
    }
}

struct WarpFetchLds {
    const double* lds;
    int y0, x0, cols;
    RL_HD double operator()(int y, int x) const { return lds[(y - y0) * cols + (x - x0)]; }
};
template <typename TS>
struct WarpFetchGlobal {
    const TS* s;
    int sy, sx;
    RL_HD double operator()(int y, int x) const { return (double)s[(size_t)warp_mirror(y, sy) * sx + warp_mirror(x, sx)]; }
};

RL_HD void warp_cubic_weights(double t, double* w) {
#pragma clang fp contract(off)
    const double u = 1.0 - t, s = 1.0 / 6.0;
    w[0] = ((u * u) * u) * s;
    w[1] = (((t * t) * (t - 2.0)) * 3.0 + 4.0) * s;
    w[2] = (((u * u) * (u - 2.0)) * 3.0 + 4.0) * s;
    w[3] = ((t * t) * t) * s;
}

// the spline at (Y, X) through `fetch` (unfolded indices), before the floor
template <int ORDER, typename Fetch>
RL_HD double warp_pixel(double Y, double X, const Fetch& fetch) {
#pragma clang fp contract(off)
    const double Fy = floor(Y), Fx = floor(X), ty = Y - Fy, tx = X - Fx;
    const int iy = (int)Fy, ix = (int)Fx;
    if (ORDER == 3) {
        double wy[4], wx[4], r[4];
        warp_cubic_weights(ty, wy);
        warp_cubic_weights(tx, wx);
        for (int i = 0; i < 4; ++i) {
            double acc = wx[0] * fetch(iy - 1 + i, ix - 1);
            for (int j = 1; j < 4; ++j) acc = __builtin_fma(wx[j], fetch(iy - 1 + i, ix - 1 + j), acc);
            r[i] = acc;
        }
        double v = wy[0] * r[0];
        for (int i = 1; i < 4; ++i) v = __builtin_fma(wy[i], r[i], v);
        return v;
    }
    const double ux = 1.0 - tx, uy = 1.0 - ty;
    double r0 = ux * fetch(iy, ix);
    if (tx != 0.0) r0 = __builtin_fma(tx, fetch(iy, ix + 1), r0);
    double v = uy * r0;
    if (ty != 0.0) {
        double r1 = ux * fetch(iy + 1, ix);
        if (tx != 0.0) r1 = __builtin_fma(tx, fetch(iy + 1, ix + 1), r1);
        v = __builtin_fma(ty, r1, v);
    }
    return v;
}

// thread t's outputs of tile (by, bx) of image i: column t mod 32, rows t / 32 + 8 k; sums[2] = raised, sum
template <typename TS, typename TD, int ORDER, typename Fetch>
RL_HD void warp_compute(const WarpParams<TS, TD>& p, size_t i, int by, int bx, int t, const Fetch& fetch, double* sums) {
#pragma clang fp contract(off)
    const double* m = p.xf + i * kWarpXf;
    const int x = bx * kWarpTW + t % kWarpTW;
    TD* d = p.dst + i * (size_t)p.oy * p.ox;
    double raised = 0.0, sum = 0.0;
    for (int r = t / kWarpTW; r < kWarpTH; r += kRegThreads / kWarpTW) {
        const int y = by * kWarpTH + r;
        if (y >= p.oy || x >= p.ox) continue;
        double Y, X;
        warp_coord(m, y, x, Y, X);
        double v = warp_pixel<ORDER>(Y, X, fetch);
        if (v < p.floor) {
            v = p.floor;
            raised = raised + 1.0;
        }
        const TD o = (TD)v;
        sum = sum + (double)o;
        d[(size_t)y * p.ox + x] = o;
    }
    sums[0] = raised; sums[1] = sum;
}

// ---- AFFINE SUMS -----------------------------------------------------------------------------------------------------------------
constexpr int kAffFields = 45;       // RL_AFFINE_FIELDS
constexpr int kAffBasis = 8;
constexpr int kAffPixels = 32;       // pixels per thread the work split aims at
constexpr int kAffBatch = 9;         // fields that share one pass of the workgroup tree
constexpr int kAffMaxBlocks = 4096;

struct AffGeom {
    int ny, nx, M, iw;
    unsigned n;                 // interior pixels
    unsigned nb, run;           // runs per pair, pixels per run
};
RL_HD unsigned aff_blocks(unsigned n) {
    const unsigned per = (unsigned)kRegThreads * kAffPixels, nb = (n + per - 1) / per;
    return nb < 1 ? 1 : (nb > (unsigned)kAffMaxBlocks ? (unsigned)kAffMaxBlocks : nb);
}
RL_HD AffGeom aff_geom(int ny, int nx, int M) {
    AffGeom g;
    g.ny = ny; g.nx = nx; g.M = M; g.iw = nx - 2 * M;
    g.n = (unsigned)(ny - 2 * M) * (unsigned)g.iw;
    g.nb = aff_blocks(g.n);
    g.run = (g.n + g.nb - 1) / g.nb;
    return g;
}

struct AffArgs {
    const void* a;              // reference images
    const void* w;              // warped moving images
    const long long* a_off;     // [pairs] element offsets (device)
    const long long* w_off;
    double* part;               // [pairs][nb][45]
    double* tot;                // [pairs][45]
    int pairs;
    AffGeom g;
};
template <typename TA, typename TW>
struct AffParams {
    const TA* a;
    const TW* w;
    const long long* a_off;
    const long long* w_off;
    double* part;
    AffGeom g;
};
template <typename TA, typename TW>
inline AffParams<TA, TW> aff_params(const AffArgs& s) {
    AffParams<TA, TW> p;
    p.a = (const TA*)s.a; p.w = (const TW*)s.w; p.a_off = s.a_off; p.w_off = s.w_off; p.part = s.part; p.g = s.g;
    return p;
}

// thread t of run b of `pair`: acc[45] from 0.0 over its pixels in increasing order
template <typename TA, typename TW>
RL_HD void aff_accumulate(const AffParams<TA, TW>& p, int pair, unsigned b, int t, double* acc) {
#pragma clang fp contract(off)
    const AffGeom& g = p.g;
    const TA* A = p.a + p.a_off[pair];
    const TW* W = p.w + p.w_off[pair];
    const double cy = 0.5 * (double)(g.ny - 1), cx = 0.5 * (double)(g.nx - 1);
    for (int f = 0; f < kAffFields; ++f) acc[f] = 0.0;
    const unsigned q0 = b * g.run, q1 = q0 + g.run < g.n ? q0 + g.run : g.n;
    for (unsigned q = q0 + (unsigned)t; q < q1; q += kRegThreads) {
        const unsigned r = q / (unsigned)g.iw;
        const int y = g.M + (int)r, x = g.M + (int)(q - r * (unsigned)g.iw);
        const size_t at = (size_t)y * g.nx + x;
        const double a = (double)A[at];
        const double gy = 0.5 * ((double)W[at + g.nx] - (double)W[at - g.nx]), gx = 0.5 * ((double)W[at + 1] - (double)W[at - 1]);
        const double yc = (double)y - cy, xc = (double)x - cx;
        double phi[kAffBasis];
        phi[0] = gy; phi[1] = gx; phi[2] = gy * yc; phi[3] = gy * xc; phi[4] = gx * yc; phi[5] = gx * xc; phi[6] = (double)W[at]; phi[7] = 1.0;
        int f = 0;
#pragma unroll
        for (int j = 0; j < kAffBasis; ++j)
#pragma unroll
            for (int k = j; k < kAffBasis; ++k, ++f) acc[f] = __builtin_fma(phi[j], phi[k], acc[f]);
#pragma unroll
        for (int j = 0; j < kAffBasis; ++j) acc[36 + j] = __builtin_fma(phi[j], a, acc[36 + j]);
        acc[44] = __builtin_fma(a, a, acc[44]);
    }
}

// ---- launchers (affine_kernels.hip), on stream s.  dtypes: RL_F32 / RL_F64.  All pointers are device pointers.
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
// the evaluation alone: order 1 from a.src of src_dtype, order 3 from float64 coefficients (src_dtype is then RL_F64); stats [n][2] or
// nullptr (then a.part may be nullptr too; otherwise a.part holds n * blocks * 2 values)
hipError_t warp_images(int src_dtype, int dst_dtype, const WarpArgs& a, double* stats, hipStream_t s);
hipError_t affine_sums(int a_dtype, int w_dtype, const AffArgs& a, hipStream_t s);
#endif

}  // namespace rl
