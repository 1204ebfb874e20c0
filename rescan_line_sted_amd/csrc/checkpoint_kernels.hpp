// checkpoint_kernels.hpp -- iteration checkpoints of the enqueued sweep (rl_batch_submit_checkpoints, include/rlsted.h): the
// estimate of every frame of a slice cast to its destination and scored against the frame's scaled object, between two iterations
// of the slice's loop.  The workgroup bodies of checkpoint_kernels.hip, written as host-compilable templates so that the CPU tests
// run the very same code (tests/emu/checkpoint_emu.cpp), and the launchers.
//
// Frame f of a launch: x = est[f], T = obj[f], n pixels each, of the plan's element type.  Every value widened to float64 before
// any arithmetic, contraction off; the six sums over the frame's pixels (RL_TRACE_FIELDS):
//     0 sum x     1 sum T     2 sum x*x     3 sum T*T     4 sum x*T     5 sum (x-T)*(x-T)
// Field 5 is formed per pixel from the difference d = x - T, never from fields 2 to 4 (which cancel where x is close to T).
// Two launches:
//   CHECKPOINT  grid (nb, frames): dst[f] = (TO) x where a destination is given; the per-workgroup sums -> part [frames][nb][6]
//               where a trace is asked for (no tree otherwise)
//   TOTALS      one thread per frame: out[f][6] = the frame's partials summed in increasing order
//
// Work split of CHECKPOINT: that of accel_kernels.hpp on the frame's n pixels (fixed by n and the element type T alone, never by
// the launch, so that a frame's numbers depend neither on the frames beside it nor on whether a destination is given) -- nvec =
// ceil(n / W) vectors of W = 16 / sizeof(T) pixels (the last one partial), handed out in accel_blocks(n) equal runs of vpb =
// ceil(nvec / nb) vectors, one run per workgroup of kCheckpointThreads threads; thread t of workgroup b takes vectors b * vpb + t,
// + kCheckpointThreads, ... up to the end of the run.  est and obj come through one 16-byte load per vector where the frame is
// 16-byte aligned, element by element otherwise (accel_load); the destination goes out in 16-byte pieces -- one for TO = T, two
// for float32 -> float64 -- except float64 -> float32, where a vector is two pixels: one 8-byte store (a wave still writes 512
// contiguous bytes).  Sums are float64, in this order:
//   thread    s_t = (((0 + v_0) + v_1) + ...) over its vectors in increasing order, the W pixels of a vector in order
//   workgroup tree over the kCheckpointThreads slots: s[t] = s[t] + s[t + h] for t < h, h = kCheckpointThreads / 2, ..., 1
//   frame     (((0 + part_0) + part_1) + ...) over the workgroups in increasing order
// No float atomics, no LDS beyond the tree: bit-identical from run to run.
#pragma once
#include "accel_kernels.hpp"

#include <cstddef>
#include <cstdint>

namespace rl {

constexpr int kCheckpointThreads = kAccelThreads;
constexpr int kCheckpointFields = 6;   // RL_TRACE_FIELDS

template <typename T, typename TO>
struct CheckpointParams {
    const T* est;    // [frames][n] the estimates
    const T* obj;    // [frames][n] the scaled objects (not read without part)
    TO* dst;         // [frames][n] or nullptr
    double* part;    // [frames][nb][kCheckpointFields] or nullptr: no sums are formed
    size_t n;        // pixels per frame
    int nb;          // workgroups per frame (accel_blocks(n, sizeof(T)))
};

RL_HD int checkpoint_blocks(size_t n, size_t esize) { return accel_blocks(n, esize); }

// W values of type T -> element e0 of a TO frame
template <typename T, typename TO>
RL_HD void checkpoint_store(TO* dst, size_t e0, size_t n, bool vec, const T* v) {
    constexpr int W = 16 / sizeof(T), WO = 16 / sizeof(TO);
    if constexpr (W % WO == 0) {   // TO = T: one piece; float32 -> float64: two
        for (int k = 0; k < W / WO; ++k) {
            TO o[WO];
            for (int c = 0; c < WO; ++c) o[c] = (TO)v[k * WO + c];
            accel_store(dst, e0 + (size_t)k * WO, n, vec, o);
        }
    } else {             // float64 -> float32: the vector's two pixels in one 8-byte store
        struct alignas(8) Half { TO e[W]; };
        if (vec && e0 + W <= n) {
            Half o;
            for (int c = 0; c < W; ++c) o.e[c] = (TO)v[c];
            *reinterpret_cast<Half*>(dst + e0) = o;
        } else {
            for (int c = 0; c < W; ++c)
                if (e0 + c < n) dst[e0 + c] = (TO)v[c];
        }
    }
}

// CHECKPOINT, thread t of workgroup b of frame f: writes the cast estimate over its vectors, returns its six sums (zeros without part)
template <typename T, typename TO>
RL_HD void checkpoint_thread(const CheckpointParams<T, TO>& p, int f, int b, int t, double* s) {
#pragma clang fp contract(off)
    constexpr int W = 16 / sizeof(T);
    const size_t n = p.n, nvec = (n + W - 1) / W, vpb = (nvec + p.nb - 1) / p.nb;
    const size_t base = (size_t)f * n;
    const T* xs = p.est + base;
    const bool sums = p.part != nullptr;
    const T* ts = sums ? p.obj + base : nullptr;
    TO* ds = p.dst ? p.dst + base : nullptr;
    const bool vec_x = accel_aligned(xs), vec_t = accel_aligned(ts);
    const bool vec_d = ((uintptr_t)ds & (sizeof(TO) * W < 16 ? sizeof(TO) * W - 1 : 15u)) == 0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0;
    const size_t j1 = ((size_t)b + 1) * vpb < nvec ? ((size_t)b + 1) * vpb : nvec;
#pragma unroll 4
    for (size_t j = (size_t)b * vpb + t; j < j1; j += kCheckpointThreads) {
        const size_t e0 = j * W;
        T xv[W], tv[W];
        accel_load(xs, e0, n, vec_x, xv);
        if (sums) accel_load(ts, e0, n, vec_t, tv);
        if (ds) checkpoint_store<T, TO>(ds, e0, n, vec_d, xv);
        if (sums)
            for (int c = 0; c < W; ++c)
                if (e0 + c < n) {
                    const double x = (double)xv[c], tr = (double)tv[c];
                    const double xx = x * x, tt = tr * tr, xt = x * tr, d = x - tr;
                    const double dd = d * d;
                    s0 = s0 + x;
                    s1 = s1 + tr;
                    s2 = s2 + xx;
                    s3 = s3 + tt;
                    s4 = s4 + xt;
                    s5 = s5 + dd;
                }
    }
    s[0] = s0;
    s[1] = s1;
    s[2] = s2;
    s[3] = s3;
    s[4] = s4;
    s[5] = s5;
}

// one step of the workgroup tree on the six sums' slots s[field][kCheckpointThreads]
RL_HD void checkpoint_tree_step(double (*s)[kCheckpointThreads], int t, int h) {
#pragma clang fp contract(off)
    if (t < h)
        for (int c = 0; c < kCheckpointFields; ++c) s[c][t] = s[c][t] + s[c][t + h];
}

// thread 0 of workgroup b of frame f, after the tree
RL_HD void checkpoint_write_part(double* part, int nb, int f, int b, const double (*s)[kCheckpointThreads]) {
    double* o = part + ((size_t)f * nb + b) * kCheckpointFields;
    for (int c = 0; c < kCheckpointFields; ++c) o[c] = s[c][0];
}

// TOTALS, frame f: its partials summed in increasing order -> out[f][kCheckpointFields]
RL_HD void checkpoint_total(const double* part, int nb, int f, double* out) {
#pragma clang fp contract(off)
    double* o = out + (size_t)f * kCheckpointFields;
    for (int c = 0; c < kCheckpointFields; ++c) {
        double v = 0.0;
        for (int b = 0; b < nb; ++b) v = v + part[((size_t)f * nb + b) * kCheckpointFields + c];
        o[c] = v;
    }
}

// ---- launchers (checkpoint_kernels.hip): frames [0, frames) of the pointers, on stream s.  est / obj [frames][n] of `dtype`, dst
// [frames][n] of out_dtype or nullptr, part [frames][nb][6] float64 or nullptr, out [frames][6] float64
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t checkpoint_take(int dtype, const void* est, const void* obj, int out_dtype, void* dst, double* part, size_t n, int frames,
                           hipStream_t s);
hipError_t checkpoint_totals(int dtype, const double* part, size_t n, int frames, double* out, hipStream_t s);
#endif

}  // namespace rl
