// accel_kernels.hpp -- Biggs-Andrews vector extrapolation of the Richardson-Lucy iteration (Biggs & Andrews, Appl. Opt. 36,
// 1766, 1997): the workgroup bodies of accel_kernels.hip, written as host-compilable templates so that the CPU tests run the
// very same code (tests/emu/accel_emu.cpp), and the launchers.
//
// psi(y) is one reference iteration (ref:520-531) applied to y, x_0 = ones.  Per frame, k = 0, 1, ...:
//     x_{k+1} = psi(y_k)                                               y_0 = x_0
//     g_k     = x_{k+1} - y_k
//     a_{k+1} = clamp(sum g_k g_{k-1} / sum g_{k-1} g_{k-1}, 0, 1)     (0 for k = 0, or a denominator that is 0 / not finite)
//     y_{k+1} = max(x_{k+1} + a_{k+1} (x_{k+1} - x_k), 0)
// Two launches around the plan's own iteration:
//   REDUCE      (after psi)        g = est - y (est = x_{k+1}); the two dot products' per-workgroup partials -> part
//   EXTRAPOLATE (before the next)  a from the frame's partials -> alpha; est = y = max(x + a (x - x_prev), 0), x_prev = x
//
// Work split (fixed by the frame size and the element type alone, never by the batch, so that a frame's sums do not depend on
// the frames beside it): a frame of n pixels is nvec = ceil(n / W) vectors of W = 16 / sizeof(T) elements (the last one
// partial), handed out in accel_blocks() equal runs of vpb = ceil(nvec / nb) vectors, one run per workgroup of
// kAccelThreads threads; thread t of workgroup b takes vectors b * vpb + t, + kAccelThreads, ... up to the end of the run.
// Sums are float64 in BOTH element types, products formed in float64 from the stored T values, in this order:
//   thread    s_t = (((0 + p_0) + p_1) + ...) over its vectors in increasing order, the W elements of a vector in order
//   workgroup tree over the kAccelThreads slots: s[t] = s[t] + s[t + h] for t < h, h = kAccelThreads / 2, ..., 1
//   frame     (((0 + part_0) + part_1) + ...) over the workgroups in increasing order
// No float atomics; contraction off (the dot products are specified to the last bit of exactly these sums).
#pragma once
#include "fft_core.hpp"

#include <cstddef>
#include <cstdint>

namespace rl {

constexpr int kAccelThreads = 256;       // threads per workgroup (four waves)
constexpr int kAccelVecsPerThread = 8;   // vectors per thread the work split aims at
constexpr int kAccelMaxBlocks = 256;     // workgroups per frame at most (the extrapolation sums this many partials)

enum AccelFlags {
    ACC_Y_ONES = 1,      // REDUCE: y_k is the start x_0 = ones (the plan's shortcut iteration from ones: no y buffer written)
    ACC_HAVE_PREV = 2,   // REDUCE: g_{k-1} exists (k >= 1); otherwise the partials are 0 and a_{k+1} = 0
    ACC_FRESH = 4,       // EXTRAPOLATE: no history (a set estimate, a change of mode): a = 0, the partials are not read
};

template <typename T>
struct AccelParams {
    T* est;          // [frames][n]  REDUCE: x_{k+1} (read); EXTRAPOLATE: x_k in, y_k out
    T* y;            // [frames][n]  REDUCE: y_k (read); EXTRAPOLATE: y_k (written)
    T* g;            // [frames][n]  REDUCE: g_{k-1} in, g_k out
    T* x;            // [frames][n]  EXTRAPOLATE: x_{k-1} in (only where a != 0), x_k out
    double* part;    // [frames][nb][2]  per-workgroup partials (sum g_k g_{k-1}, sum g_{k-1} g_{k-1})
    double* alpha;   // [frames]  EXTRAPOLATE: a of the point it formed
    size_t n;        // pixels per frame
    int nb;          // workgroups per frame (accel_blocks)
    int flags;
};

RL_HD int accel_width(size_t esize) { return (int)(16 / esize); }
// workgroups per frame for n pixels of esize bytes
RL_HD int accel_blocks(size_t n, size_t esize) {
    const size_t W = 16 / esize, nvec = (n + W - 1) / W, per = (size_t)kAccelThreads * kAccelVecsPerThread;
    const size_t nb = (nvec + per - 1) / per;
    return nb < 1 ? 1 : (nb > (size_t)kAccelMaxBlocks ? kAccelMaxBlocks : (int)nb);
}

template <typename T>
struct alignas(16) AccelVec {
    T e[16 / sizeof(T)];
};

// the frame's W-element vector j of `src` -> v (whole vectors of an aligned frame through one 16-byte access, otherwise element by
// element; elements past the frame read as 0)
template <typename T>
RL_HD void accel_load(const T* src, size_t e0, size_t n, bool vec, T* v) {
    constexpr int W = 16 / sizeof(T);
    if (vec && e0 + W <= n) {
        const AccelVec<T> a = *reinterpret_cast<const AccelVec<T>*>(src + e0);
        for (int c = 0; c < W; ++c) v[c] = a.e[c];
    } else {
        for (int c = 0; c < W; ++c) v[c] = e0 + c < n ? src[e0 + c] : T(0);
    }
}
template <typename T>
RL_HD void accel_store(T* dst, size_t e0, size_t n, bool vec, const T* v) {
    constexpr int W = 16 / sizeof(T);
    if (vec && e0 + W <= n) {
        AccelVec<T> a;
        for (int c = 0; c < W; ++c) a.e[c] = v[c];
        *reinterpret_cast<AccelVec<T>*>(dst + e0) = a;
    } else {
        for (int c = 0; c < W; ++c)
            if (e0 + c < n) dst[e0 + c] = v[c];
    }
}
RL_HD bool accel_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// REDUCE, thread t of workgroup b of frame f: writes g_k over its vectors, returns its two sums
template <typename T>
RL_HD void accel_reduce_thread(const AccelParams<T>& p, int f, int b, int t, double& num, double& den) {
#pragma clang fp contract(off)
    constexpr int W = 16 / sizeof(T);
    const size_t n = p.n, nvec = (n + W - 1) / W, vpb = (nvec + p.nb - 1) / p.nb;
    const size_t base = (size_t)f * n;
    const T* xs = p.est + base;
    const T* ys = p.y + base;
    T* gs = p.g + base;
    const bool ones = (p.flags & ACC_Y_ONES) != 0, prev = (p.flags & ACC_HAVE_PREV) != 0;
    const bool vec = accel_aligned(xs) && accel_aligned(gs) && (ones || accel_aligned(ys));   // (the same for every buffer in a plan)
    double sn = 0.0, sd = 0.0;
    const size_t j1 = ((size_t)b + 1) * vpb < nvec ? ((size_t)b + 1) * vpb : nvec;
    for (size_t j = (size_t)b * vpb + t; j < j1; j += kAccelThreads) {
        const size_t e0 = j * W;
        T xv[W], yv[W], gp[W], gn[W];
        accel_load(xs, e0, n, vec, xv);
        if (ones) {
            for (int c = 0; c < W; ++c) yv[c] = T(1);
        } else {
            accel_load(ys, e0, n, vec, yv);
        }
        if (prev) accel_load((const T*)gs, e0, n, vec, gp);
        for (int c = 0; c < W; ++c) {
            gn[c] = xv[c] - yv[c];
            if (prev && e0 + c < n) {
                const double a = (double)gn[c] * (double)gp[c];
                const double d = (double)gp[c] * (double)gp[c];
                sn = sn + a;
                sd = sd + d;
            }
        }
        accel_store(gs, e0, n, vec, gn);
    }
    num = sn;
    den = sd;
}

// one step of the workgroup tree (every t < h reads slots >= h, which nobody writes in this step)
RL_HD void accel_tree_step(double* s, int t, int h) {
#pragma clang fp contract(off)
    if (t < h) s[t] = s[t] + s[t + h];
}

// a from a frame's partials [nb][2] (summed in increasing order)
RL_HD double accel_alpha(const double* part, int nb) {
#pragma clang fp contract(off)
    double num = 0.0, den = 0.0;
    for (int b = 0; b < nb; ++b) {
        num = num + part[2 * b];
        den = den + part[2 * b + 1];
    }
    if (!(den > 0.0) || !(den <= 1.7976931348623157e308)) return 0.0;   // 0, negative, inf, nan
    const double r = num / den;
    return r > 1.0 ? 1.0 : (r > 0.0 ? r : 0.0);                            // (a nan quotient gives 0)
}

// EXTRAPOLATE, thread t of workgroup b of frame f, with the frame's a
template <typename T>
RL_HD void accel_extrapolate_thread(const AccelParams<T>& p, int f, int b, int t, double alpha) {
#pragma clang fp contract(off)
    constexpr int W = 16 / sizeof(T);
    const size_t n = p.n, nvec = (n + W - 1) / W, vpb = (nvec + p.nb - 1) / p.nb;
    const size_t base = (size_t)f * n;
    T* es = p.est + base;
    T* ys = p.y + base;
    T* xs = p.x + base;
    const bool vec = accel_aligned(es) && accel_aligned(ys) && accel_aligned(xs);
    const T a = (T)alpha;
    const bool move = alpha != 0.0;   // a == 0: y = max(x, 0), x_{k-1} is not read (it may not exist)
    const size_t j1 = ((size_t)b + 1) * vpb < nvec ? ((size_t)b + 1) * vpb : nvec;
    for (size_t j = (size_t)b * vpb + t; j < j1; j += kAccelThreads) {
        const size_t e0 = j * W;
        T xv[W], xp[W], yv[W];
        accel_load((const T*)es, e0, n, vec, xv);
        if (move) accel_load((const T*)xs, e0, n, vec, xp);
        for (int c = 0; c < W; ++c) {
            T v = xv[c];
            if (move) v = xv[c] + a * (xv[c] - xp[c]);
            yv[c] = v > T(0) ? v : T(0);
        }
        accel_store(es, e0, n, vec, yv);
        accel_store(ys, e0, n, vec, yv);
        accel_store(xs, e0, n, vec, xv);
    }
}

// ---- launchers (accel_kernels.hip): frames [0, frames) of the pointers' batch, on stream s.  Buffers are [frames][n] of the
// plan's dtype; part [frames][nb][2], alpha [frames] float64.
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t accel_reduce(int dtype, const void* est, const void* y, void* g, double* part, size_t n, int frames, int flags,
                        hipStream_t s);
hipError_t accel_extrapolate(int dtype, void* est, void* y, void* x, const double* part, double* alpha, size_t n, int frames,
                             int flags, hipStream_t s);
#endif

}  // namespace rl
