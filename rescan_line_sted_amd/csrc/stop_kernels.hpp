// stop_kernels.hpp -- the Poisson I-divergence of a frame's prediction, on the device, and the stopping rule of
// rl_deconv_iterate_until (include/rlsted.h): the workgroup bodies of stop_kernels.hip, written as host-compilable templates so
// that the CPU tests run the very same code (tests/emu/stop_emu.cpp), and the launchers.
//
// D(m || p) = sum m log(m / p) - m + p is what Richardson-Lucy minimises (m the measurement, p = H(estimate)).  Per frame, over its
// V view images -- N = V * ny * nx stored values of the plan's type T, contiguous in the measurement and in the prediction --, each
// value converted to float64 before any arithmetic, the term of a pixel is
//     p > 0           :  ((m > 0 ? m * log(m / p) : 0) - m) + p             log: the float64 device log
//     p <= 0 or nan   :  m > 0 ? 0 : -m       a prediction the plan could not resolve is a neutral pixel, as in rl_ratio
//                                             (DESIGN.md section 3b): a ratio of 1 means m = p, whose term is 0
// Two launches per check:
//   DIVERGENCE  the terms' per-workgroup sums -> part [frames][nb]                  (reads 2 N sizeof(T) bytes per frame)
//   LATCH       D = the frame's partials summed; the rule against the frame's state; a frame that had not stopped before this
//               check gets its estimate copied to the result buffer and D / the iteration count latched
//   (TOTAL      D alone -> out [frames], for rl_deconv_divergence)
//
// Work split of DIVERGENCE (fixed by N and the element type alone, never by the batch, so that a frame's sum does not depend on
// the frames beside it): the split of accel_kernels.hpp on the frame's N values -- nvec = ceil(N / W) vectors of W = 16 / sizeof(T)
// elements (the last one partial), handed out in stop_blocks(N) = accel_blocks(N) equal runs of vpb = ceil(nvec / nb) vectors, one
// run per workgroup of kStopThreads threads; thread t of workgroup b takes vectors b * vpb + t, + kStopThreads, ... up to the end
// of the run, each through one 16-byte load per stream (m and p) where the frame is 16-byte aligned, element by element otherwise.
// Sums are float64 in BOTH element types, in this order:
//   thread    s_t = (((0 + term_0) + term_1) + ...) over its vectors in increasing order, the W elements of a vector in order
//   workgroup tree over the kStopThreads slots: s[t] = s[t] + s[t + h] for t < h, h = kStopThreads / 2, ..., 1
//   frame     (((0 + part_0) + part_1) + ...) over the workgroups in increasing order
// The longest chain of additions a value passes through: ceil(vpb / kStopThreads) * W + log2(kStopThreads) + nb.
// No float atomics; contraction off.
//
// LATCH runs on grid (accel_blocks(ny * nx), frames): every workgroup of a frame sums the same partials in the same order and
// reads the frame's state of the PREVIOUS check (prev); workgroup 0 writes the state of THIS check to the other half of the
// double buffer (next) -- no workgroup reads what another workgroup of the launch writes.
#pragma once
#include "accel_kernels.hpp"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rl {

constexpr int kStopThreads = kAccelThreads;
constexpr int kStopMaxBlocks = kAccelMaxBlocks;

enum StopRule {
    STOP_RULE_DISCREPANCY = 1,   // 2 D / N <= t
    STOP_RULE_RELATIVE = 2,      // a previous check of this run exists and D_prev - D <= t * D_prev
};

// state of one frame after a check (double buffered by check parity)
struct StopFrame {
    double d_latched;   // D at the latched point: the check at which the frame stopped, or the last check so far
    double d_last;      // D of this check (the next check's D_prev)
    int iterations;     // iterations of this run at the latched point
    int stopped;        // a check has met the rule
};

template <typename T>
struct DivParams {
    const T* meas;   // [frames][N]
    const T* pred;   // [frames][N]
    double* part;    // [frames][nb]
    size_t n;        // N: values per frame (all its views)
    int nb;          // workgroups per frame (stop_blocks)
};

template <typename T>
struct LatchParams {
    const T* est;            // [frames][n]
    T* result;               // [frames][n]
    const double* part;      // [frames][nb_part]
    const StopFrame* prev;   // [frames]  state after the previous check (not read when have_prev == 0)
    StopFrame* next;         // [frames]  state after this check
    size_t n;                // pixels of one estimate image
    int nb;                  // workgroups per frame of this launch (accel_blocks(n))
    int nb_part;             // partials per frame (stop_blocks(N))
    int rule;
    int have_prev;           // a previous check of this run exists
    int done;                // iterations of this run so far
    double threshold;
    double count;            // N as a double
};

RL_HD int stop_blocks(size_t n_frame, size_t esize) { return accel_blocks(n_frame, esize); }

RL_HD double stop_term(double m, double p) {
#pragma clang fp contract(off)
    if (p > 0.0) {
        const double a = m > 0.0 ? m * log(m / p) : 0.0;
        return (a - m) + p;
    }
    return m > 0.0 ? 0.0 : -m;
}

// DIVERGENCE, thread t of workgroup b of frame f: the sum of its terms
template <typename T>
RL_HD double stop_divergence_thread(const DivParams<T>& p, int f, int b, int t) {
#pragma clang fp contract(off)
    constexpr int W = 16 / sizeof(T);
    const size_t n = p.n, nvec = (n + W - 1) / W, vpb = (nvec + p.nb - 1) / p.nb;
    const T* ms = p.meas + (size_t)f * n;
    const T* ps = p.pred + (size_t)f * n;
    const bool vec = accel_aligned(ms) && accel_aligned(ps);
    double s = 0.0;
    const size_t j1 = ((size_t)b + 1) * vpb < nvec ? ((size_t)b + 1) * vpb : nvec;
    for (size_t j = (size_t)b * vpb + t; j < j1; j += kStopThreads) {
        const size_t e0 = j * W;
        T mv[W], pv[W];
        accel_load(ms, e0, n, vec, mv);
        accel_load(ps, e0, n, vec, pv);
        for (int c = 0; c < W; ++c)
            if (e0 + c < n) s = s + stop_term((double)mv[c], (double)pv[c]);
    }
    return s;
}

// D from a frame's partials (summed in increasing order)
RL_HD double stop_total(const double* part, int nb) {
#pragma clang fp contract(off)
    double d = 0.0;
    for (int b = 0; b < nb; ++b) d = d + part[b];
    return d;
}

RL_HD bool stop_finite(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }

// does D meet the rule?  (a D -- or, for the relative rule, a D_prev -- that is nan or inf never does)
RL_HD bool stop_rule_met(int rule, double threshold, double count, double d, bool have_prev, double d_prev) {
#pragma clang fp contract(off)
    if (!stop_finite(d)) return false;
    if (rule == STOP_RULE_DISCREPANCY) return 2.0 * d / count <= threshold;
    if (rule == STOP_RULE_RELATIVE) return have_prev && stop_finite(d_prev) && d_prev - d <= threshold * d_prev;
    return false;
}

// LATCH, the decision every workgroup of frame f reaches from D: the frame's state after this check; *copy = the frame had not
// stopped before (its estimate goes to the result buffer)
template <typename T>
RL_HD StopFrame stop_latch_frame(const LatchParams<T>& p, int f, double d, bool* copy) {
    StopFrame s;
    const bool before = p.have_prev && p.prev[f].stopped != 0;
    if (before) {
        s = p.prev[f];
    } else {
        s.d_latched = d;
        s.iterations = p.done;
        s.stopped = stop_rule_met(p.rule, p.threshold, p.count, d, p.have_prev != 0, p.have_prev ? p.prev[f].d_last : 0.0) ? 1 : 0;
    }
    s.d_last = d;
    *copy = !before;
    return s;
}

// LATCH, thread t of workgroup b of frame f: result = est over its vectors (the split of accel_kernels.hpp on the n pixels)
template <typename T>
RL_HD void stop_copy_thread(const LatchParams<T>& p, int f, int b, int t) {
    constexpr int W = 16 / sizeof(T);
    const size_t n = p.n, nvec = (n + W - 1) / W, vpb = (nvec + p.nb - 1) / p.nb;
    const T* es = p.est + (size_t)f * n;
    T* rs = p.result + (size_t)f * n;
    const bool vec = accel_aligned(es) && accel_aligned(rs);
    const size_t j1 = ((size_t)b + 1) * vpb < nvec ? ((size_t)b + 1) * vpb : nvec;
    for (size_t j = (size_t)b * vpb + t; j < j1; j += kStopThreads) {
        T v[W];
        accel_load(es, j * W, n, vec, v);
        accel_store(rs, j * W, n, vec, v);
    }
}

// ---- launchers (stop_kernels.hip): frames [0, frames) of the pointers' batch, on stream s.  meas / pred: [frames][n_frame] of the
// plan's dtype, part [frames][stop_blocks(n_frame)] float64; est / result [frames][n_img]; prev / next [frames].
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t stop_divergence(int dtype, const void* meas, const void* pred, double* part, size_t n_frame, int frames, hipStream_t s);
hipError_t stop_totals(int dtype, const double* part, size_t n_frame, int frames, double* out, hipStream_t s);
hipError_t stop_latch(int dtype, const void* est, void* result, const double* part, const StopFrame* prev, StopFrame* next, size_t n_img,
                      size_t n_frame, int frames, int rule, double threshold, int done, int have_prev, hipStream_t s);
#endif

}  // namespace rl
