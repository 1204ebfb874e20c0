// register_kernels.hpp -- registration of acquired views and frames on the device (rl_register_sums, rl_shift_images,
// rl_register_peaks, rl_register_estimate, include/rlsted.h): the thread bodies of register_kernels.hip and
// register_peaks.hip, written as host-compilable templates so that the CPU tests run the very same code (tests/emu/register_emu.cpp,
// tests/emu/register_peaks_emu.cpp), the host builder of the shift's taps, the estimate's host rules, and the launchers.
//
// SUMS  For a pair (A, B) of ny x nx images, a search radius R and a margin M >= R, with the interior I = [M, ny - M) x [M, nx - M):
//       S_b(d) = sum_I B[y + dy][x + dx]    S_bb(d) = sum_I B[y + dy][x + dx]^2    S_ab(d) = sum_I A[y][x] B[y + dy][x + dx]
//   for every d = (dy, dx) in [-R, R]^2 (index (dy + R) * (2 R + 1) + dx + R), and S_a = sum_I A, S_aa = sum_I A^2.  Every value is
//   widened to float64 first.  Geometry (reg_geom, decided by R alone): W = 2 R + 1, nd = W^2 displacements; tiles of TY x 32 pixels,
//   TY = 16 for R <= 16, else 8; G = 1 for nd >= 256, else the largest power of two with G <= TY and G * nd <= 256; strips of
//   h = TY / G rows.  The interior's rows are cut into strips of h rows from y = M on (a band of TY rows is G strips; the last
//   strips may be short or empty), its columns into blocks of 32 from x = M on.  ORDER OF EVERY SUM:
//     strip, d   from 0.0: the column blocks in increasing order, inside a block the strip's rows in increasing order, inside a row
//                the columns in increasing order; per pixel, with b = B[y + dy][x + dx], a = A[y][x]:
//                    S_b = S_b + b;   S_bb = fma(b, b, S_bb);   S_ab = fma(a, b, S_ab)
//     pair, d    (((0.0 + strip_0) + strip_1) + ...) over ALL strips in increasing order (k_register_totals)
//     S_a, S_aa  per image row from 0.0 over its interior columns in increasing order (S_a + a; fma(a, a, S_aa)), then
//                (((0.0 + row_M) + row_{M+1}) + ...) in increasing order, rows of the last band beyond the interior being 0.0
//   No atomics: bit-identical from run to run, and a pair's numbers do not depend on the other pairs of a call.
//   Work split: a workgroup of 256 threads owns (pair, band, pass); thread t owns ONE displacement and one strip of the band --
//   G = 1: d = 256 * pass + t (passes = ceil(nd / 256)); G > 1: d = t mod nd, strip t / nd -- and keeps its three sums in registers
//   while the workgroup walks the band's column blocks: a block's A tile and B halo tile ((TY + 2 R) x (32 + 2 R)) are staged in LDS
//   as float64 (nothing outside an image is read: halo positions outside it are staged as 0 and never used, because M >= R).
//   LDS row stride of the halo tile: S = 32 + 2 R + 1 doubles.  The lanes of a wave hold consecutive d, lane l reads the double at
//   (y + dy) S + x + dx = const + d + 32 dy: consecutive doubles modulo 32 -- the 64 banks of a ds_read_b64 half-wave are hit once
//   each, wherever the lanes wrap to the next dy -- and every lane reads the same A element (a broadcast).
//   At R = 32: (8 + 64) * 97 + 8 * 32 doubles = 57,920 bytes, two workgroups per CU.
//
// SHIFT  dst[i][y][x] = max(spline of image i at (y + sy, x + sx), floor): scipy.ndimage.shift(src[i], (-sy, -sx), order, mode =
//   'mirror').  A translation keeps the fractional part constant along an axis, so prefilter and evaluation along one axis are ONE
//   finite impulse response on the whole-sample mirror extension of the image (shift_taps): with F = floor(s), t = s - F,
//     order 1   g = (1 - t, t) at offsets F, F + 1 (a zero weight is dropped: an integer shift is the tap 1.0 alone)
//     order 3   g[m] = sum_i w_i(t) h[m - (i - 1)], offsets F + m, m = -(K + 1) .. K + 2, K = 30 (64 taps); w the cubic B-spline
//               weights at offsets -1 .. 2, h[k] = sqrt(3) z^|k|, z = sqrt(3) - 2, |k| <= K: the impulse response of the recursive
//               prefilter with exact mirror initialisation, cut where |z|^(K+1) = 1.9e-18 -- the dropped tail is at most
//               2 sqrt(3) |z|^(K+1) / (1 - |z|) = 8.8e-18 max|image| per axis, below half a unit in the last place
//   formed in long double on the host and rounded once.  out = sum_m g[m] src[mirror(. + F + m)]: acc = g[0] * v_0, then
//   acc = fma(g[m], v_m, acc) for m = 1, 2, ... in increasing order.  Pass 1 runs along x into a float64 workspace, pass 2 along y,
//   applies the floor (acc < floor: floor, counted) and rounds once to the destination type.  Both passes stage a tile of 32 x 64
//   outputs plus its taps' reach in LDS with coalesced loads; lanes read consecutive doubles (conflict-free).
//   Statistics per image: the count of raised pixels and the sum of the stored values (widened to float64): a thread over its
//   outputs in increasing row order, the ingest kernels' tree over the 256 threads, the workgroups in increasing order.
#pragma once
#include "ingest_kernels.hpp"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rl {

constexpr int kRegThreads = 256;     // four waves
constexpr int kRegTX = 32;           // columns of a tile
constexpr int kRegMaxR = 32;
constexpr int kRegFields = 3;        // S_b, S_bb, S_ab (RL_REGISTER_FIELDS)

struct RegGeom {
    int ny, nx, R, M;
    int W, nd;          // 2 R + 1, W * W
    int TY, G, h;       // tile rows, strips per band, rows per strip
    int S;              // LDS row stride of the halo tile, doubles
    int passes, bands, ntx, strips;
};

RL_HD RegGeom reg_geom(int ny, int nx, int R, int M) {
    RegGeom g;
    g.ny = ny; g.nx = nx; g.R = R; g.M = M;
    g.W = 2 * R + 1;
    g.nd = g.W * g.W;
    g.TY = R <= 16 ? 16 : 8;
    g.G = 1;
    if (g.nd < kRegThreads)
        while (g.G * 2 <= g.TY && g.G * 2 * g.nd <= kRegThreads) g.G *= 2;
    g.h = g.TY / g.G;
    g.S = kRegTX + 2 * R + 1;
    g.passes = g.G > 1 ? 1 : (g.nd + kRegThreads - 1) / kRegThreads;
    g.bands = (ny - 2 * M + g.TY - 1) / g.TY;
    g.ntx = (nx - 2 * M + kRegTX - 1) / kRegTX;
    g.strips = g.bands * g.G;
    return g;
}
RL_HD size_t reg_lds_doubles(const RegGeom& g) { return (size_t)(g.TY + 2 * g.R) * g.S + (size_t)g.TY * kRegTX; }
// float64 values of a pair's partials: [strips][nd][3], then [bands * TY][2]
RL_HD size_t reg_part_doubles(const RegGeom& g) { return (size_t)g.strips * g.nd * kRegFields + (size_t)g.bands * g.TY * 2; }

struct RegSumArgs {
    const void* a;              // reference images
    const void* b;              // moving images
    const long long* a_off;     // [pairs] element offsets (device)
    const long long* b_off;
    double* part;               // [pairs][reg_part_doubles]
    double* tot;                // [pairs][nd * 3 + 2]
    int pairs;
    RegGeom g;
};
template <typename TA, typename TB>
struct RegSumParams {
    const TA* a;
    const TB* b;
    const long long* a_off;
    const long long* b_off;
    double* part;
    RegGeom g;
};
template <typename TA, typename TB>
inline RegSumParams<TA, TB> reg_sum_params(const RegSumArgs& s) {
    RegSumParams<TA, TB> p;
    p.a = (const TA*)s.a; p.b = (const TB*)s.b; p.a_off = s.a_off; p.b_off = s.b_off; p.part = s.part; p.g = s.g;
    return p;
}

// the displacement index and the strip (of its band) that thread t of pass `pass` owns; false: the thread owns nothing
RL_HD bool reg_slot(const RegGeom& g, int pass, int t, int& d, int& sub) {
    if (g.G > 1) {
        d = t % g.nd;
        sub = t / g.nd;
        return sub < g.G;
    }
    d = pass * kRegThreads + t;
    sub = 0;
    return d < g.nd;
}

// thread t's share of staging column block `tile` of `band`: B's halo tile, then A's tile, as float64
template <typename TA, typename TB>
RL_HD void reg_stage(const RegSumParams<TA, TB>& p, int pair, int band, int tile, int t, double* lds) {
    const RegGeom& g = p.g;
    const int y0 = g.M + band * g.TY, x0 = g.M + tile * kRegTX;
    const TA* A = p.a + p.a_off[pair];
    const TB* B = p.b + p.b_off[pair];
    const int hb = g.TY + 2 * g.R, wb = kRegTX + 2 * g.R;
    double* la = lds + (size_t)hb * g.S;
    for (int e = t; e < hb * wb; e += kRegThreads) {
        const int r = e / wb, c = e - r * wb;
        const int y = y0 - g.R + r, x = x0 - g.R + c;
        lds[r * g.S + c] = (y >= 0 && y < g.ny && x >= 0 && x < g.nx) ? (double)B[(size_t)y * g.nx + x] : 0.0;
    }
    for (int e = t; e < g.TY * kRegTX; e += kRegThreads) {
        const int r = e / kRegTX, c = e % kRegTX;
        const int y = y0 + r, x = x0 + c;
        la[e] = (y < g.ny - g.M && x < g.nx - g.M) ? (double)A[(size_t)y * g.nx + x] : 0.0;
    }
}

// thread t walks the staged block: acc[3] += its displacement's terms over its strip; pass 0, t < TY: row[2] += row t of A
RL_HD void reg_walk(const RegGeom& g, int band, int tile, int pass, int t, const double* lds, double* acc, double* row) {
    const int y0 = g.M + band * g.TY, x0 = g.M + tile * kRegTX;
    const int th = g.ny - g.M - y0 < g.TY ? g.ny - g.M - y0 : g.TY;
    const int tw = g.nx - g.M - x0 < kRegTX ? g.nx - g.M - x0 : kRegTX;
    const double* la = lds + (size_t)(g.TY + 2 * g.R) * g.S;
    int d, sub;
    if (reg_slot(g, pass, t, d, sub)) {
        const int dy = d / g.W, dx = d - dy * g.W;
        const int r1 = (sub + 1) * g.h < th ? (sub + 1) * g.h : th;
        double s_b = acc[0], s_bb = acc[1], s_ab = acc[2];
        for (int r = sub * g.h; r < r1; ++r) {
            const double* brow = lds + (r + dy) * g.S + dx;
            const double* arow = la + r * kRegTX;
            for (int x = 0; x < tw; ++x) {
                const double b = brow[x], a = arow[x];
                s_b = s_b + b;
                s_bb = __builtin_fma(b, b, s_bb);
                s_ab = __builtin_fma(a, b, s_ab);
            }
        }
        acc[0] = s_b; acc[1] = s_bb; acc[2] = s_ab;
    }
    if (pass == 0 && t < th) {
        const double* arow = la + t * kRegTX;
        double s_a = row[0], s_aa = row[1];
        for (int x = 0; x < tw; ++x) {
            const double a = arow[x];
            s_a = s_a + a;
            s_aa = __builtin_fma(a, a, s_aa);
        }
        row[0] = s_a; row[1] = s_aa;
    }
}

// thread t's partials of (pair, band, pass) go to the pair's block of `part`
RL_HD void reg_store(const RegGeom& g, double* part, int pair, int band, int pass, int t, const double* acc, const double* row) {
    double* pp = part + (size_t)pair * reg_part_doubles(g);
    int d, sub;
    if (reg_slot(g, pass, t, d, sub)) {
        double* o = pp + ((size_t)(band * g.G + sub) * g.nd + d) * kRegFields;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    }
    if (pass == 0 && t < g.TY) {
        double* o = pp + (size_t)g.strips * g.nd * kRegFields + ((size_t)band * g.TY + t) * 2;
        o[0] = row[0]; o[1] = row[1];
    }
}

// value `id` of a pair's totals [nd * 3 + 2] from its partials, in increasing order
RL_HD double reg_total(const RegGeom& g, const double* pp, int id) {
#pragma clang fp contract(off)
    double s = 0.0;
    if (id < g.nd * kRegFields) {
        for (int q = 0; q < g.strips; ++q) s = s + pp[(size_t)q * g.nd * kRegFields + id];
    } else {
        const double* ra = pp + (size_t)g.strips * g.nd * kRegFields + (id - g.nd * kRegFields);
        for (int r = 0; r < g.bands * g.TY; ++r) s = s + ra[(size_t)r * 2];
    }
    return s;
}

// ---- SHIFT -----------------------------------------------------------------------------------------------------------------------
constexpr int kShiftTaps = 64;       // 2 K + 4
constexpr int kShiftK = 30;
constexpr int kShiftTH = 32;         // output rows of a tile
constexpr int kShiftTW = 64;         // output columns of a tile
constexpr int kShiftFields = 2;      // raised, sum (RL_SHIFT_FIELDS)
constexpr int kShiftLds = (kShiftTH + kShiftTaps - 1) * kShiftTW;   // doubles; the x pass needs 32 * (64 + 63), less

struct ShiftImage {                  // one image's taps (device table)
    double gx[kShiftTaps], gy[kShiftTaps];
    int ox, oy;                      // offset of tap 0, reduced into [0, 2 (n - 1)) (0 for n = 1)
    int ntx, nty;
};

RL_HD int shift_mirror(int i, int n) {   // scipy 'mirror' (d c b | a b c d | c b a) for i >= 0
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i = i % p;
    return i >= n ? p - i : i;
}

// the taps of one axis of n samples for the shift s: g[0 .. *nt), tap m reads sample mirror(k + *off + m)
inline void shift_taps(double s, int order, int n, double* g, int* off, int* nt) {
    const long double F = floorl((long double)s), t = (long double)s - F;
    long long first;
    if (order == 1) {
        first = (long long)F;
        if (t == 0.0L) {
            g[0] = 1.0;
            *nt = 1;
        } else {
            g[0] = (double)(1.0L - t);
            g[1] = (double)t;
            *nt = 2;
        }
    } else {
        const long double u = 1.0L - t;
        const long double w[4] = {u * u * u / 6.0L, (t * t * (t - 2.0L) * 3.0L + 4.0L) / 6.0L, (u * u * (u - 2.0L) * 3.0L + 4.0L) / 6.0L,
                                  t * t * t / 6.0L};
        const long double r3 = sqrtl(3.0L), z = r3 - 2.0L;
        long double h[kShiftK + 1];
        h[0] = r3;
        for (int k = 1; k <= kShiftK; ++k) h[k] = h[k - 1] * z;
        for (int j = 0; j < kShiftTaps; ++j) {       // m = j - (K + 1)
            long double acc = 0.0L;
            for (int i = 0; i < 4; ++i) {
                const int k = j - (kShiftK + 1) - (i - 1);
                if (k >= -kShiftK && k <= kShiftK) acc += w[i] * h[k < 0 ? -k : k];
            }
            g[j] = (double)acc;
        }
        *nt = kShiftTaps;
        first = (long long)F - (kShiftK + 1);
    }
    const long long p = n > 1 ? 2LL * (n - 1) : 1;
    *off = (int)(((first % p) + p) % p);
}

struct ShiftArgs {
    const void* src;            // [n][ny][nx]
    void* dst;
    const ShiftImage* img;      // [n] (device)
    double* part;               // [n][blocks][2], or nullptr
    int n, ny, nx;
    double floor;
};
template <typename TS, typename TD>
struct ShiftParams {
    const TS* src;
    TD* dst;
    const ShiftImage* img;
    double* part;
    int ny, nx, nby, nbx;
    double floor;
};
RL_HD int shift_blocks_y(int ny) { return (ny + kShiftTH - 1) / kShiftTH; }
RL_HD int shift_blocks_x(int nx) { return (nx + kShiftTW - 1) / kShiftTW; }
template <typename TS, typename TD>
inline ShiftParams<TS, TD> shift_params(const ShiftArgs& a) {
    ShiftParams<TS, TD> p;
    p.src = (const TS*)a.src; p.dst = (TD*)a.dst; p.img = a.img; p.part = a.part; p.ny = a.ny; p.nx = a.nx;
    p.nby = shift_blocks_y(a.ny); p.nbx = shift_blocks_x(a.nx); p.floor = a.floor;
    return p;
}

// thread t's share of staging the inputs of output tile (by, bx) of image i: AXIS 1 (x): 32 rows of 64 + nt - 1 mirrored columns;
// AXIS 0 (y): 32 + nt - 1 mirrored rows of 64 columns.  Positions beyond the image on the other axis are staged as 0, unread.
template <typename TS, typename TD, int AXIS>
RL_HD void shift_stage(const ShiftParams<TS, TD>& p, size_t i, int by, int bx, int t, double* lds) {
    const ShiftImage& im = p.img[i];
    const int nt = AXIS == 1 ? im.ntx : im.nty, off = AXIS == 1 ? im.ox : im.oy;
    const int rows = kShiftTH + (AXIS == 0 ? nt - 1 : 0), cols = kShiftTW + (AXIS == 1 ? nt - 1 : 0);
    const int y0 = by * kShiftTH, x0 = bx * kShiftTW;
    const TS* s = p.src + i * (size_t)p.ny * p.nx;
    for (int e = t; e < rows * cols; e += kRegThreads) {
        const int r = e / cols, c = e - r * cols;
        int y = y0 + r, x = x0 + c;
        bool live;
        if (AXIS == 1) {
            live = y < p.ny && x0 < p.nx;
            x = shift_mirror(x + off, p.nx);
        } else {
            live = x < p.nx && y0 < p.ny;
            y = shift_mirror(y + off, p.ny);
        }
        lds[e] = live ? (double)s[(size_t)y * p.nx + x] : 0.0;
    }
}

// thread t's outputs of the tile: column t mod 64, rows t / 64 + 4 k.  FINAL: the floor, one rounding, sums[2] = raised, sum
template <typename TS, typename TD, int AXIS, bool FINAL>
RL_HD void shift_compute(const ShiftParams<TS, TD>& p, size_t i, int by, int bx, int t, const double* lds, double* sums) {
    const ShiftImage& im = p.img[i];
    const int nt = AXIS == 1 ? im.ntx : im.nty;
    const double* g = AXIS == 1 ? im.gx : im.gy;
    const int cols = kShiftTW + (AXIS == 1 ? nt - 1 : 0), step = AXIS == 1 ? 1 : cols;
    const int c = t % kShiftTW, x = bx * kShiftTW + c;
    TD* d = p.dst + i * (size_t)p.ny * p.nx;
    double raised = 0.0, sum = 0.0;
    for (int r = t / kShiftTW; r < kShiftTH; r += kRegThreads / kShiftTW) {
        const int y = by * kShiftTH + r;
        if (y >= p.ny || x >= p.nx) continue;
        const double* v = lds + r * cols + c;
        double acc = g[0] * v[0];
        for (int m = 1; m < nt; ++m) acc = __builtin_fma(g[m], v[(size_t)m * step], acc);
        if (FINAL) {
            if (acc < p.floor) {
                acc = p.floor;
                raised = raised + 1.0;
            }
            const TD o = (TD)acc;
            sum = sum + (double)o;
            d[(size_t)y * p.nx + x] = o;
        } else {
            d[(size_t)y * p.nx + x] = (TD)acc;
        }
    }
    sums[0] = raised; sums[1] = sum;
}

// ---- PEAKS -----------------------------------------------------------------------------------------------------------------------
// The host's stages 2 - 4 (registration.ncc_surface, surface_peak) on a pair's row of totals [nd * 3 + 2] as k_register_totals
// leaves it, bit for bit.  Per displacement, in float64, every product and quotient rounded on its own (no contraction):
//     va = saa - sa sa / n    vb = s1 - s0 s0 / n    c = (s2 - sa s0 / n) / sqrt(va vb)
// FLAT: !(va > 0) or !(vb > 0) for any d (nan counts): shift 0, value 0, at_limit 0, flat 1, a surface of zeros.
// PEAK: the first maximum in row-major order.  A workgroup of 256 threads per pair, thread t takes d = t, t + 256, ... in increasing
//   order and keeps (value, index), replaced only on a strict >; the LDS tree keeps the larger value and, on equal values, the
//   smaller index.  PARABOLA (thread 0): the five values at the peak recomputed by the same expression (the same bits);
//   den = (m - 2 z) + p, delta = (0.5 (m - p)) / den, 0 where den == 0; a peak on the window's border: at_limit, delta 0;
//   shift = (double)(i - R) + delta per axis.  No atomics; nothing outside the pair's rows is read or written.
constexpr int kPeakFields = 5;       // shift_y, shift_x, value, at_limit, flat (RL_PEAK_FIELDS)

struct RegPeakArgs {
    const double* tot;          // [pairs][nd * 3 + 2]
    double* peaks;              // [pairs][kPeakFields]
    double* surf;               // [pairs][nd], or nullptr
    int pairs, R;
    double n;                   // terms of every sum
};

RL_HD double reg_peak_va(const double* tp, int nd, double n) {
#pragma clang fp contract(off)
    const double sa = tp[(size_t)nd * kRegFields], saa = tp[(size_t)nd * kRegFields + 1];
    return saa - sa * sa / n;
}

// the NCC of displacement d; vb_ok: S_bb - S_b^2 / n > 0 (false for nan)
RL_HD double reg_ncc(const double* tp, int nd, int d, double n, bool& vb_ok) {
#pragma clang fp contract(off)
    const double sa = tp[(size_t)nd * kRegFields];
    const double va = reg_peak_va(tp, nd, n);
    const double s0 = tp[(size_t)d * kRegFields], s1 = tp[(size_t)d * kRegFields + 1], s2 = tp[(size_t)d * kRegFields + 2];
    const double vb = s1 - s0 * s0 / n;
    vb_ok = vb > 0.0;
    return (s2 - sa * s0 / n) / sqrt(va * vb);
}

// thread t's first maximum over its displacements; flat: 1 when va or one of its vb is not positive
RL_HD void reg_peak_scan(const double* tp, int nd, double n, int t, double& v, int& i, int& flat) {
    v = -__builtin_inf();
    i = nd;
    flat = reg_peak_va(tp, nd, n) > 0.0 ? 0 : 1;
    for (int d = t; d < nd; d += kRegThreads) {
        bool ok;
        const double c = reg_ncc(tp, nd, d, n, ok);
        if (!ok) flat = 1;
        if (c > v) {
            v = c;
            i = d;
        }
    }
}

// one step of the LDS tree, t < h: the larger value, on equal values the smaller index; flat is or-ed
RL_HD void reg_peak_tree_step(double* v, int* i, int* f, int t, int h) {
    if (t >= h) return;
    const double ov = v[t + h];
    const int oi = i[t + h];
    if (ov > v[t] || (ov == v[t] && oi < i[t])) {
        v[t] = ov;
        i[t] = oi;
    }
    f[t] = f[t] | f[t + h];
}

RL_HD double reg_parabola(double m, double z, double p) {
#pragma clang fp contract(off)
    const double den = (m - 2.0 * z) + p;
    return den == 0.0 ? 0.0 : (0.5 * (m - p)) / den;
}

// thread 0: the pair's fields from the tree's (value, index, flat)
RL_HD void reg_peak_finish(const double* tp, int R, double n, double v, int i, int flat, double* out) {
#pragma clang fp contract(off)
    const int W = 2 * R + 1, nd = W * W;
    if (flat) {
        out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; out[3] = 0.0; out[4] = 1.0;
        return;
    }
    const int iy = i / W, ix = i - iy * W;
    out[2] = v; out[4] = 0.0;
    if (iy == 0 || iy == W - 1 || ix == 0 || ix == W - 1) {
        out[0] = (double)(iy - R); out[1] = (double)(ix - R); out[3] = 1.0;
        return;
    }
    bool ok;
    const double z = reg_ncc(tp, nd, i, n, ok);
    const double ym = reg_ncc(tp, nd, i - W, n, ok), yp = reg_ncc(tp, nd, i + W, n, ok);
    const double xm = reg_ncc(tp, nd, i - 1, n, ok), xp = reg_ncc(tp, nd, i + 1, n, ok);
    out[0] = (double)(iy - R) + reg_parabola(ym, z, yp);
    out[1] = (double)(ix - R) + reg_parabola(xm, z, xp);
    out[3] = 0.0;
}

// thread t's share of the surface [nd]: its displacements' NCC, zeros for a flat pair
RL_HD void reg_peak_surface(const double* tp, int nd, double n, int t, int flat, double* sp) {
    for (int d = t; d < nd; d += kRegThreads) {
        bool ok;
        sp[d] = flat ? 0.0 : reg_ncc(tp, nd, d, n, ok);
    }
}

// The host's rules of an estimate (registration._estimate, coarse = None) on the fields [kPeakFields] of a pair: the first stage
// sets the shift [2] and fields [3] = ncc, at_limit, flat; a refine pass over a pair that was not flat replaces the value and adds
// the offset unless the pass finds the pair flat (at_limit keeps the first stage's answer).
inline void reg_estimate_first(const double* pk, double* shift, double* fields) {
    shift[0] = pk[0]; shift[1] = pk[1];
    fields[0] = pk[2]; fields[1] = pk[3]; fields[2] = pk[4];
}
inline void reg_estimate_refine(const double* pk, double* shift, double* fields) {
#pragma clang fp contract(off)
    if (pk[4] != 0.0) return;
    shift[0] = shift[0] + pk[0];
    shift[1] = shift[1] + pk[1];
    fields[0] = pk[2];
}

// ---- launchers (register_kernels.hip, register_peaks.hip), on stream s.  dtypes: RL_F32 / RL_F64.  All pointers are device pointers.
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t register_sums(int a_dtype, int b_dtype, const RegSumArgs& a, hipStream_t s);
hipError_t register_peaks(const RegPeakArgs& a, hipStream_t s);
// pass 1 (along x): src of src_dtype -> tmp float64; pass 2 (along y): tmp -> dst of dst_dtype; stats [n][2] or nullptr (then
// a.part may be nullptr too; otherwise a.part holds n * blocks * 2 values)
hipError_t shift_images(int src_dtype, int dst_dtype, const ShiftArgs& a, double* tmp, double* stats, hipStream_t s);
#endif

}  // namespace rl
