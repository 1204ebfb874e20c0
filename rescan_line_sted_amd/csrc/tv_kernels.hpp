// tv_kernels.hpp -- total-variation regularised Richardson-Lucy (Dey et al., Microsc. Res. Tech. 69, 260, 2006): the multiplicative
// RL-TV step x_new = psi(x) / (1 - lambda div(grad x / |grad x|)) around the plan's own iteration psi.  The workgroup bodies of
// tv_kernels.hip, written as host-compilable templates so that the CPU tests run the very same code (tests/emu/tv_emu.cpp), and the
// launchers.  The arithmetic, to the last bit, is the specification of rl_deconv_set_tv in include/rlsted.h.
//
// Two launches around the iteration (and a third only where the partials are not of the point at hand):
//   WEIGHT  (before psi)  s = (sum x) / n from the frame's partials; w = 1 / (1 - lambda div) of the point x = est -> w
//   APPLY   (after psi)   est = est * w, and the float64 per-workgroup partials of sum est_new -> part (the next step's s)
//   SUM     = APPLY with TV_SUM_ONLY: the partials of sum est alone, nothing stored to est, w not read
//
// WEIGHT works on tiles of kTvRows rows x kTvVecs vectors of W = 16 / sizeof(T) pixels.  A workgroup stages its tile plus a one-pixel
// halo in LDS (rows i0 - 1 .. i0 + kTvRows, columns j0 - 1 .. j0 + kTvVecs W; pixels outside the image are stored as 0 and never
// enter a result: the boundary rules below select 0 instead).  The interior columns sit at a 16-byte aligned LDS offset (W elements
// of left margin, of which the last is the west halo), so that a thread's own vector is one 16-byte LDS read.  Thread t takes vector
// t % kTvVecs of the kTvRowsPerThread consecutive rows of row group t / kTvVecs (a wave is one row group: its lanes read consecutive
// vectors) and walks down them.  Per pixel the seven values x(i,j), (i,j+1), (i+1,j), (i,j-1), (i-1,j), (i-1,j+1), (i+1,j-1) come from
// LDS.  Nothing of the neighbours' unit gradients is stored: a thread keeps the py of the row it has just left and the px of the pixel
// to its left in registers -- the very values the spec's px[i,j-1] and py[i-1,j] name -- and recomputes them, by the same expressions,
// only where they belong to another thread (the first row of its group, the first pixel of its vector).
//
// APPLY has the work split and the order of every sum of accel_kernels.hpp (accel_blocks workgroups of kAccelThreads threads per
// frame, thread / tree / frame order), with the element est_new widened to float64 in place of the products.
#pragma once
#include "accel_kernels.hpp"

#include <cmath>

namespace rl {

constexpr int kTvVecs = 64;                                        // vectors (of W pixels) of a tile row: one per lane of a wave
constexpr int kTvRowsPerThread = 4;                                // rows a thread walks down
constexpr int kTvRows = kAccelThreads / kTvVecs * kTvRowsPerThread;   // rows of a WEIGHT tile
constexpr int kTvLdsRows = kTvRows + 2;

enum TvFlags {
    TV_SUM_ONLY = 1,   // APPLY: partials of sum est only (a point APPLY did not produce, or the step from ones, whose w is 1)
};

template <typename T>
struct TvParams {
    T* est;              // [frames][ny][nx]  WEIGHT: x (read); APPLY: psi(x) in, x_new out
    T* w;                // [frames][ny][nx]  WEIGHT: written; APPLY: read
    double* part;        // [frames][nb]      WEIGHT: partials of sum x (read); APPLY / SUM: partials of sum est_new (written)
    double lambda, eps_rel;
    int ny, nx;
    int nb;              // accel_blocks(ny * nx, sizeof(T))
    int tiles_x;         // WEIGHT: tiles per image row
    int flags;
};

template <typename T>
RL_HD constexpr int tv_tile_cols() { return kTvVecs * (int)(16 / sizeof(T)); }
template <typename T>
RL_HD constexpr int tv_lds_pitch() { return tv_tile_cols<T>() + 2 * (int)(16 / sizeof(T)); }   // W of margin on either side
template <typename T>
RL_HD constexpr int tv_lds_elems() { return kTvLdsRows * tv_lds_pitch<T>(); }

RL_HD int tv_tiles_x(int nx, size_t esize) { const int tc = kTvVecs * (int)(16 / esize); return (nx + tc - 1) / tc; }
RL_HD int tv_tiles_y(int ny) { return (ny + kTvRows - 1) / kTvRows; }

// s = (sum x) / n from a frame's partials [nb] (summed in increasing order)
RL_HD double tv_mean(const double* part, int nb, size_t n) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s = s + part[b];
    return s / (double)n;
}
// eps2 = T((eps_rel s) (eps_rel s)): formed in float64, rounded once
template <typename T>
RL_HD T tv_eps2(double eps_rel, double s) {
#pragma clang fp contract(off)
    const double e = eps_rel * s;
    return (T)(e * e);
}

// rows of a frame start on 16-byte boundaries (then every vector of a tile row is one 16-byte access)
template <typename T>
RL_HD bool tv_rows_aligned(const T* frame, int nx) { return accel_aligned(frame) && ((size_t)nx * sizeof(T)) % 16 == 0; }

// WEIGHT, staging: thread t of the workgroup of tile `tile` of frame f fills its share of the LDS tile
template <typename T>
RL_HD void tv_stage_thread(const TvParams<T>& p, int f, int tile, int t, T* lds) {
    constexpr int W = 16 / sizeof(T), P = tv_lds_pitch<T>();
    const int i0 = tile / p.tiles_x * kTvRows, j0 = tile % p.tiles_x * tv_tile_cols<T>();
    const T* xs = p.est + (size_t)f * p.ny * p.nx;
    const bool vec = tv_rows_aligned(xs, p.nx);
    for (int v = t; v < kTvLdsRows * kTvVecs; v += kAccelThreads) {   // the interior columns, a vector at a time
        const int r = v / kTvVecs, c = v % kTvVecs, i = i0 - 1 + r, j = j0 + c * W;
        T x[W];
        if (i >= 0 && i < p.ny && j < p.nx) {
            accel_load(xs + (size_t)i * p.nx, (size_t)j, (size_t)p.nx, vec, x);
        } else {
            for (int e = 0; e < W; ++e) x[e] = T(0);
        }
        AccelVec<T> a;
        for (int e = 0; e < W; ++e) a.e[e] = x[e];
        *reinterpret_cast<AccelVec<T>*>(lds + r * P + W + c * W) = a;
    }
    if (t < 2 * kTvLdsRows) {   // the west and east halo columns
        const int r = t / 2, east = t % 2, i = i0 - 1 + r, j = east ? j0 + tv_tile_cols<T>() : j0 - 1;
        const bool in = i >= 0 && i < p.ny && j >= 0 && j < p.nx;
        lds[r * P + (east ? W + tv_tile_cols<T>() : W - 1)] = in ? xs[(size_t)i * p.nx + j] : T(0);
    }
}

// one component of the unit gradient: d / sqrt((dx dx + dy dy) + eps2)
template <typename T>
RL_HD T tv_unit(T d, T dx, T dy, T eps2) {
#pragma clang fp contract(off)
    const T q = dx * dx + dy * dy;
    const T m = std::sqrt(q + eps2);
    return d / m;
}

// WEIGHT, thread t: the weights of its vector in each of its rows, from the staged tile
template <typename T>
RL_HD void tv_weight_thread(const TvParams<T>& p, int f, int tile, int t, const T* lds, T eps2) {
#pragma clang fp contract(off)
    constexpr int W = 16 / sizeof(T), P = tv_lds_pitch<T>();
    const int i0 = tile / p.tiles_x * kTvRows, j0 = tile % p.tiles_x * tv_tile_cols<T>();
    const int g = t / kTvVecs, c = t % kTvVecs, ia = i0 + g * kTvRowsPerThread, j = j0 + c * W;
    if (ia >= p.ny || j >= p.nx) return;
    T* ws = p.w + (size_t)f * p.ny * p.nx;
    const bool vec = tv_rows_aligned(ws, p.nx);
    const T lambda = (T)p.lambda;
    T pyn[W];   // py of the row above, per pixel of the vector
    for (int r = 0; r < kTvRowsPerThread; ++r) {
        const int i = ia + r;
        if (i >= p.ny) break;
        const T* row = lds + (i - i0 + 1) * P + W + c * W;   // x(i, j)
        const T *north = row - P, *south = row + P;
        // the thread's window: columns j - 1 .. j + W of the rows i and i + 1 (and, in its first row, i - 1)
        T xc[W + 2], xs[W + 2];
        for (int e = 0; e < W + 2; ++e) {
            xc[e] = row[e - 1];
            xs[e] = south[e - 1];
        }
        const bool last_row = i + 1 >= p.ny;
        if (r == 0) {   // the north neighbours (i - 1, jj) belong to another thread: their dy ends on this row
            for (int e = 0; e < W; ++e) {
                const int jj = j + e, k = e + 1;
                pyn[e] = T(0);
                if (i > 0 && jj < p.nx) {
                    const T xnn = north[k - 1];
                    const T dxn = jj + 1 >= p.nx ? T(0) : north[k] - xnn;
                    const T dyn = xc[k] - xnn;
                    pyn[e] = tv_unit(dyn, dxn, dyn, eps2);
                }
            }
        }
        T out[W];
        T pxw = T(0);
        if (j > 0) {   // the west neighbour (i, j - 1) of the vector's first pixel belongs to another thread: its dx ends on this pixel
            const T xw = xc[0];
            const T dxw = xc[1] - xw;
            const T dyw = last_row ? T(0) : xs[0] - xw;
            pxw = tv_unit(dxw, dxw, dyw, eps2);
        }
        for (int e = 0; e < W; ++e) {
            const int jj = j + e, k = e + 1;   // k: the pixel's index in the window
            if (jj >= p.nx) {
                out[e] = T(0);
                continue;
            }
            const T x = xc[k];
            const T dx = jj + 1 >= p.nx ? T(0) : xc[k + 1] - x;
            const T dy = last_row ? T(0) : xs[k] - x;
            const T px = tv_unit(dx, dx, dy, eps2), py = tv_unit(dy, dx, dy, eps2);
            const T div = (px - pxw) + (py - pyn[e]);
            out[e] = T(1) / (T(1) - lambda * div);
            pxw = px;      // px[i, jj] is the next pixel's px[i, jj + 1 - 1]
            pyn[e] = py;   // py[i, jj] is the next row's py[i + 1 - 1, jj]
        }
        accel_store(ws + (size_t)i * p.nx, (size_t)j, (size_t)p.nx, vec, out);
    }
}

// APPLY / SUM, thread t of workgroup b of frame f: est = est * w over its vectors, returns its sum of est_new
template <typename T>
RL_HD double tv_apply_thread(const TvParams<T>& p, int f, int b, int t) {
#pragma clang fp contract(off)
    constexpr int W = 16 / sizeof(T);
    const size_t n = (size_t)p.ny * p.nx, nvec = (n + W - 1) / W, vpb = (nvec + p.nb - 1) / p.nb;
    const size_t base = (size_t)f * n;
    T* es = p.est + base;
    const bool sum_only = (p.flags & TV_SUM_ONLY) != 0;
    const T* ws = sum_only ? nullptr : p.w + base;
    const bool vec = accel_aligned(es) && (sum_only || accel_aligned(ws));
    double s = 0.0;
    const size_t j1 = ((size_t)b + 1) * vpb < nvec ? ((size_t)b + 1) * vpb : nvec;
    for (size_t j = (size_t)b * vpb + t; j < j1; j += kAccelThreads) {
        const size_t e0 = j * W;
        T xv[W], wv[W];
        accel_load((const T*)es, e0, n, vec, xv);
        if (!sum_only) {
            accel_load(ws, e0, n, vec, wv);
            for (int c = 0; c < W; ++c) xv[c] = xv[c] * wv[c];
            accel_store(es, e0, n, vec, xv);
        }
        for (int c = 0; c < W; ++c)
            if (e0 + c < n) s = s + (double)xv[c];
    }
    return s;
}

// ---- launchers (tv_kernels.hip): frames [0, frames) of the pointers' batch, on stream s.  est, w: [frames][ny][nx] of the plan's
// dtype; part [frames][accel_blocks(ny nx)] float64.
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t tv_weight(int dtype, const void* est, void* w, const double* part, double lambda, double eps_rel, int ny, int nx, int frames,
                     hipStream_t s);
hipError_t tv_apply(int dtype, void* est, const void* w, double* part, int ny, int nx, int frames, int flags, hipStream_t s);
#endif

}  // namespace rl
