// bead_kernels.hpp -- the peak finder of the bead measurement (rl_find_peaks, include/rlsted.h): the thread
// bodies of bead_kernels.hip, written as host-compilable functions so that the CPU tests run the very same code phase by phase
// (tests/emu/bead_emu.cpp).  Each body is one thread's share of a phase between two workgroup barriers.
//
// Per image x of ny x nx, taps w[0 .. 2h], radius r, border b >= h + r, every value widened to float64, no contraction:
//   u(y, x) = (...((0.0 + w[0] x(y, x - h)) + w[1] x(y, x - h + 1)) + ...) + w[2h] x(y, x + h)        row pass
//   s(y, x) = the same fold over u(y - h + k, x), k ascending                                           column pass
// D = [b, ny - b) x [b, nx - b).  lo / hi: min / max of the non-nan s over D (exact: order free); t = v > threshold ? v : threshold
// with v = lo + rel (hi - lo).  p in D is a candidate when s(p) >= t, s(q) < s(p) for every q with |q - p|_inf <= r before p in
// row-major order and s(q) <= s(p) for every such q after it (IEEE comparisons: a nan anywhere in the window disqualifies p).
// D is cut into tiles of kBpTY x kBpTX pixels from (b, b); the last row and column of tiles may be partial.
//   RANGE    a workgroup per (image, tile): u on (kBpTY + 2h) x kBpTX, s on the tile, the tile's lo / hi through a halving tree in
//            LDS -> part[image][tile][2].
//   LEVELS   a workgroup per image: the tiles' lo / hi, thread t takes tiles t, t + 256, ..., then the tree; thread 0 forms t.
//   MARK     a workgroup per (image, tile): u on (kBpTY + 2r + 2h) x (kBpTX + 2r), s on (kBpTY + 2r) x (kBpTX + 2r) (the halo of h + r
//            is read from the image: b >= h + r keeps it inside), the rule above per tile pixel, flags in LDS, then one 32-bit word
//            per tile row -> mask[image][y - b][tile column], bit x - x0.
//   COMPACT  a workgroup per image: thread t owns the words [t c, (t + 1) c) of the image's mask in (row, tile column) order -- which
//            is row-major pixel order -- counts their bits, thread 0 forms the exclusive prefix of the 256 counts in order (integers:
//            exact), and every thread walks its words again, bits ascending, writing the candidates whose rank is below cap: (y, x),
//            s(p) recomputed at the pixel by the same folds, x(p).  count[image] = the total.
// No atomics, no floating-point sum whose order depends on the launch: bit-identical from run to run, and an image's result does
// not depend on the other images of the call.
// LDS (RANGE, MARK): u then s, (UH + SH) SW doubles, SW = kBpTX + 2 rr, SH = kBpTY + 2 rr, UH = SH + 2 h, rr = 0 (RANGE) or r
// (MARK): at most (80 + 48) 64 8 = 65536 bytes at h = r = 16.  After the column pass the u region is dead and holds the tree's two
// arrays of 256 doubles (RANGE; u has at least 16 * 32 doubles, exactly that at h = 0) or the 512 flag bytes (MARK).
#pragma once
#include "fft_core.hpp"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rl {

constexpr int kBpThreads = 256;
constexpr int kBpTY = 16;            // tile rows
constexpr int kBpTX = 32;            // tile columns: one 32-bit mask word per tile row
constexpr int kBpMaxH = 16;
constexpr int kBpMaxR = 16;
constexpr int kBpLevels = 3;         // lo, hi, t (RL_PEAK_LEVELS)

struct BpArgs {
    const void* src;             // the images
    int f64;                     // element type: 0 float, 1 double
    const long long* off;        // [n] element offsets (device)
    int n, ny, nx, h, r, b, cap;
    const double* w;             // [2h + 1] taps (device)
    double rel, threshold;
    int nty, ntx;                // tiles over D
    double* part;                // [n][nty ntx][2]: lo, hi of every tile
    double* levels;              // [n][kBpLevels]
    unsigned* mask;              // [n][ny - 2b][ntx]
    int* yx;                     // [n][cap][2]
    double* sv;                  // [n][cap]: s(p)
    double* xv;                  // [n][cap]: x(p)
    long long* count;            // [n]
};

struct BpTile {
    long long img, tile;
    int tx, y0, x0, rr, SW, SH, UH, yl, xl;   // yl / xl: the s region's rows / columns end (exclusive, image coordinates)
    long long base;                           // the image's element offset
};

RL_HD size_t bp_lds_bytes(int h, int rr) {
    const size_t SW = kBpTX + 2 * rr, SH = kBpTY + 2 * rr, UH = SH + 2 * h;
    return (UH + SH) * SW * sizeof(double);
}
RL_HD double bp_load(const void* p, int f64, long long i) { return f64 ? ((const double*)p)[i] : (double)((const float*)p)[i]; }

RL_HD BpTile bp_tile(const BpArgs& p, long long block, int rr) {
    BpTile T;
    const long long nt = (long long)p.nty * p.ntx;
    T.img = block / nt;
    T.tile = block % nt;
    T.tx = (int)(T.tile % p.ntx);
    T.y0 = p.b + (int)(T.tile / p.ntx) * kBpTY;
    T.x0 = p.b + T.tx * kBpTX;
    T.rr = rr;
    T.SW = kBpTX + 2 * rr;
    T.SH = kBpTY + 2 * rr;
    T.UH = T.SH + 2 * p.h;
    T.yl = (T.y0 + kBpTY < p.ny - p.b ? T.y0 + kBpTY : p.ny - p.b) + rr;
    T.xl = (T.x0 + kBpTX < p.nx - p.b ? T.x0 + kBpTX : p.nx - p.b) + rr;
    T.base = p.off[T.img];
    return T;
}

// u(gy, gx) of the image at `base`; the caller keeps gx - h .. gx + h inside the row
RL_HD double bp_u(const BpArgs& p, long long base, int gy, int gx) {
#pragma clang fp contract(off)
    const long long row = base + (long long)gy * p.nx + gx - p.h;
    double u = 0.0;
    for (int j = 0; j <= 2 * p.h; ++j) u = u + p.w[j] * bp_load(p.src, p.f64, row + j);
    return u;
}
// s(y, x) at one pixel: the column fold over u computed by bp_u -- the operations of the tile's two passes
RL_HD double bp_s_point(const BpArgs& p, long long base, int y, int x) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int k = 0; k <= 2 * p.h; ++k) s = s + p.w[k] * bp_u(p, base, y - p.h + k, x);
    return s;
}

// ---- RANGE / MARK: row pass, thread t; U [UH][SW]
RL_HD void bp_row_body(const BpArgs& p, const BpTile& T, int t, double* U) {
    for (int i = t; i < T.UH * T.SW; i += kBpThreads) {
        const int gy = T.y0 - T.rr - p.h + i / T.SW, gx = T.x0 - T.rr + i % T.SW;
        if (gy < T.yl + p.h && gx < T.xl) U[i] = bp_u(p, T.base, gy, gx);
    }
}
// column pass, thread t; S [SH][SW]
RL_HD void bp_col_body(const BpArgs& p, const BpTile& T, int t, const double* U, double* S) {
#pragma clang fp contract(off)
    for (int i = t; i < T.SH * T.SW; i += kBpThreads) {
        const int ry = i / T.SW, rx = i % T.SW;
        if (T.y0 - T.rr + ry < T.yl && T.x0 - T.rr + rx < T.xl) {
            double s = 0.0;
            for (int k = 0; k <= 2 * p.h; ++k) s = s + p.w[k] * U[(ry + k) * T.SW + rx];
            S[i] = s;
        }
    }
}

// ---- RANGE: thread t's lo / hi over its tile pixels in D (rr = 0), into lo[t], hi[t]
RL_HD void bp_range_body(const BpArgs& p, const BpTile& T, int t, const double* S, double* lo, double* hi) {
    double l = HUGE_VAL, g = -HUGE_VAL;
    for (int i = t; i < kBpTY * kBpTX; i += kBpThreads) {
        const int ly = i / kBpTX, lx = i % kBpTX;
        if (T.y0 + ly < p.ny - p.b && T.x0 + lx < p.nx - p.b) {
            const double v = S[ly * T.SW + lx];
            if (v < l) l = v;
            if (v > g) g = v;
        }
    }
    lo[t] = l;
    hi[t] = g;
}
RL_HD void bp_minmax_step(double* lo, double* hi, int t, int h) {
    if (t < h) {
        if (lo[t + h] < lo[t]) lo[t] = lo[t + h];
        if (hi[t + h] > hi[t]) hi[t] = hi[t + h];
    }
}
RL_HD void bp_range_finish(const BpArgs& p, const BpTile& T, const double* lo, const double* hi) {
    double* o = p.part + ((size_t)T.img * p.nty * p.ntx + T.tile) * 2;
    o[0] = lo[0];
    o[1] = hi[0];
}

// ---- LEVELS: workgroup `img`
RL_HD void bp_levels_body(const BpArgs& p, long long img, int t, double* lo, double* hi) {
    const long long nt = (long long)p.nty * p.ntx;
    const double* q = p.part + (size_t)img * nt * 2;
    double l = HUGE_VAL, g = -HUGE_VAL;
    for (long long k = t; k < nt; k += kBpThreads) {
        if (q[2 * k] < l) l = q[2 * k];
        if (q[2 * k + 1] > g) g = q[2 * k + 1];
    }
    lo[t] = l;
    hi[t] = g;
}
RL_HD void bp_levels_finish(const BpArgs& p, long long img, const double* lo, const double* hi) {
#pragma clang fp contract(off)
    const double v = lo[0] + p.rel * (hi[0] - lo[0]);
    double* o = p.levels + (size_t)img * kBpLevels;
    o[0] = lo[0];
    o[1] = hi[0];
    o[2] = v > p.threshold ? v : p.threshold;
}

// ---- MARK: the rule at tile pixel i of thread t's share, flags [kBpTY][kBpTX] bytes
RL_HD bool bp_is_peak(const double* S, int c, int SW, int r, double t) {
    const double sp = S[c];
    if (!(sp >= t)) return false;
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const double q = S[c + dy * SW + dx];
            if (dy < 0 || (dy == 0 && dx < 0)) {
                if (!(q < sp)) return false;
            } else if (!(q <= sp)) {
                return false;
            }
        }
    return true;
}
RL_HD void bp_mark_body(const BpArgs& p, const BpTile& T, int t, const double* S, unsigned char* flags) {
    const double lvl = p.levels[(size_t)T.img * kBpLevels + 2];
    for (int i = t; i < kBpTY * kBpTX; i += kBpThreads) {
        const int ly = i / kBpTX, lx = i % kBpTX;
        bool c = false;
        if (T.y0 + ly < p.ny - p.b && T.x0 + lx < p.nx - p.b) c = bp_is_peak(S, (ly + T.rr) * T.SW + lx + T.rr, T.SW, T.rr, lvl);
        flags[i] = c ? 1 : 0;
    }
}
// thread t < kBpTY: the word of tile row t
RL_HD void bp_word_body(const BpArgs& p, const BpTile& T, int t, const unsigned char* flags) {
    if (t >= kBpTY || T.y0 + t >= p.ny - p.b) return;
    unsigned word = 0;
    for (int c = 0; c < kBpTX; ++c)
        if (flags[t * kBpTX + c]) word |= 1u << c;
    const long long ndy = p.ny - 2 * p.b;
    p.mask[((size_t)T.img * ndy + (T.y0 + t - p.b)) * p.ntx + T.tx] = word;
}

// ---- COMPACT: workgroup `img`; thread t's words [*first, *last)
RL_HD void bp_words_of(const BpArgs& p, int t, long long* first, long long* last) {
    const long long W = (long long)(p.ny - 2 * p.b) * p.ntx, per = (W + kBpThreads - 1) / kBpThreads;
    *first = t * per < W ? t * per : W;
    *last = (t + 1) * per < W ? (t + 1) * per : W;
}
RL_HD long long bp_count_body(const BpArgs& p, long long img, int t) {
    long long a, e, c = 0;
    bp_words_of(p, t, &a, &e);
    const unsigned* m = p.mask + (size_t)img * (p.ny - 2 * p.b) * p.ntx;
    for (long long k = a; k < e; ++k) c += __builtin_popcount(m[k]);
    return c;
}
// thread 0: counts [256] -> exclusive prefix in place; count[img] = the total
RL_HD void bp_scan_body(const BpArgs& p, long long img, long long* counts) {
    long long run = 0;
    for (int k = 0; k < kBpThreads; ++k) {
        const long long c = counts[k];
        counts[k] = run;
        run += c;
    }
    p.count[img] = run;
}
RL_HD void bp_write_body(const BpArgs& p, long long img, int t, long long rank) {
    if (rank >= p.cap) return;
    long long a, e;
    bp_words_of(p, t, &a, &e);
    const unsigned* m = p.mask + (size_t)img * (p.ny - 2 * p.b) * p.ntx;
    const long long base = p.off[img];
    for (long long k = a; k < e; ++k) {
        unsigned word = m[k];
        while (word) {
            const int c = __builtin_ctz(word);
            word &= word - 1;
            const int y = p.b + (int)(k / p.ntx), x = p.b + (int)(k % p.ntx) * kBpTX + c;
            const size_t o = (size_t)img * p.cap + (size_t)rank;
            p.yx[2 * o] = y;
            p.yx[2 * o + 1] = x;
            p.sv[o] = bp_s_point(p, base, y, x);
            p.xv[o] = bp_load(p.src, p.f64, base + (long long)y * p.nx + x);
            if (++rank >= p.cap) return;
        }
    }
}

// ---- launcher (bead_kernels.hip), on stream s: RANGE, LEVELS, MARK, COMPACT for a.n images.  All pointers are device pointers.
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t find_peaks(const BpArgs& a, hipStream_t s);
#endif

}  // namespace rl
