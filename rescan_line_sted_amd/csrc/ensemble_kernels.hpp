// ensemble_kernels.hpp -- per-pixel statistics over the members of an ensemble of device-resident images (rl_ensemble_stats,
// include/rlsted.h): mean, unbiased variance, squared bias and mean squared error against a scaled truth, and their pixel sums.
// The workgroup bodies of ensemble_kernels.hip, written as host-compilable templates so that the CPU tests run the very same code
// (tests/emu/ensemble_emu.cpp), and the launchers.
//
// Group g of a call is the images at element offsets member_off[group_ptr[g] .. group_ptr[g + 1]) of the source buffer, n >= 1 of
// them, each N contiguous values of type T; its truth, if any, N values of type TT at truth_off[g], times truth_scale[g] = s.
// Per pixel, every value widened to float64 before any arithmetic, the members x_0 ... x_{n-1} in list order:
//     mean = ((((0 + x_0) + x_1) + ...) + x_{n-1}) / n
//     ss   = (((0 + (x_0 - mean)^2) + (x_1 - mean)^2) + ...)        a SECOND pass over the members (never sum x^2 - n mean^2)
//     var  = n > 1 ? ss / (n - 1) : 0
//     st   = s * t                                                   (one rounding)
//     b2   = (mean - st)^2
//     mse  = (((0 + (x_0 - st)^2) + (x_1 - st)^2) + ...) / n
// Without a truth st = b2 = mse = 0.  Two launches:
//   STATS   grid (nb, groups): mean and var -> the float64 maps [groups][N] (either may be absent); the per-workgroup sums of
//           mean, var, b2, mse, st^2 -> part [groups][nb][kEnsembleSums]
//   TOTALS  one thread per group: out[g] = { n, the five sums of the group's partials }
//
// Work split of STATS: that of accel_kernels.hpp on the group's N pixels (fixed by N and the element type T alone, never by the
// call, so that a group's numbers do not depend on the groups beside it) -- nvec = ceil(N / W) vectors of W = 16 / sizeof(T)
// pixels (the last one partial), handed out in accel_blocks(N) equal runs of vpb = ceil(nvec / nb) vectors, one run per workgroup
// of kEnsembleThreads threads; thread t of workgroup b takes vectors b * vpb + t, + kEnsembleThreads, ... up to the end of the run.
// A member's vector comes through one 16-byte load where that member image is 16-byte aligned, element by element otherwise
// (accel_load); the truth and the maps likewise in 16-byte pieces.  A group of up to kEnsembleHold = 16 members is read once: the
// thread keeps the members' vectors in registers between the two passes (a workgroup is alone on its CU at the grids this split
// gives, so the loads in flight per thread are what hides the memory latency); a larger group is read twice.  The arithmetic and
// its order are the same either way.  Sums are float64, in this order:
//   thread    s_t = (((0 + v_0) + v_1) + ...) over its vectors in increasing order, the W pixels of a vector in order
//   workgroup tree over the kEnsembleThreads slots: s[t] = s[t] + s[t + h] for t < h, h = kEnsembleThreads / 2, ..., 1
//   group     (((0 + part_0) + part_1) + ...) over the workgroups in increasing order
// No float atomics, no LDS beyond the tree, contraction off: bit-identical from run to run.
#pragma once
#include "accel_kernels.hpp"

#include <cstddef>
#include <cstdint>

namespace rl {

constexpr int kEnsembleThreads = kAccelThreads;
constexpr int kEnsembleSums = 5;     // mean, var, b2, mse, st^2
constexpr int kEnsembleFields = 6;   // n and the five sums (RL_ENSEMBLE_FIELDS)
constexpr int kEnsembleHold = 16;    // groups of up to this many members are read ONCE: a thread keeps their vectors in registers

template <typename T, typename TT>
struct EnsembleParams {
    const T* src;                  // base of the member images
    const int64_t* member_off;     // element offsets (device)
    const int32_t* group_ptr;      // [groups + 1] into member_off (device)
    const TT* truth;               // base of the truth images, or nullptr
    const int64_t* truth_off;      // [groups] (device; not read without a truth)
    const double* truth_scale;     // [groups]
    double* mean;                  // [groups][n] or nullptr
    double* var;                   // [groups][n] or nullptr
    double* part;                  // [groups][nb][kEnsembleSums]
    size_t n;                      // pixels per image
    int nb;                        // workgroups per group (accel_blocks(n, sizeof(T)))
};

RL_HD int ensemble_blocks(size_t n, size_t esize) { return accel_blocks(n, esize); }

// W values of type TT from element e0 of `src`, widened -> v (elements past n read as 0)
template <typename TT, int W>
RL_HD void ensemble_load_wide(const TT* src, size_t e0, size_t n, bool vec, double* v) {
    constexpr int WT = 16 / sizeof(TT);
    if (W % WT == 0) {
        for (int k = 0; k < W / WT; ++k) {
            TT tmp[WT];
            accel_load(src, e0 + (size_t)k * WT, n, vec, tmp);
            for (int c = 0; c < WT; ++c) v[k * WT + c] = (double)tmp[c];
        }
    } else {
        for (int c = 0; c < W; ++c) v[c] = e0 + c < n ? (double)src[e0 + c] : 0.0;
    }
}

// W float64 values -> element e0 of a map, in 16-byte pieces
template <int W>
RL_HD void ensemble_store_map(double* dst, size_t e0, size_t n, bool vec, const double* v) {
    for (int k = 0; k < W / 2; ++k) accel_store(dst, e0 + 2 * (size_t)k, n, vec, v + 2 * k);
}

// STATS, thread t of workgroup b of group g: writes the maps over its vectors, returns its five sums
template <typename T, typename TT>
RL_HD void ensemble_thread(const EnsembleParams<T, TT>& p, int g, int b, int t, double* s) {
#pragma clang fp contract(off)
    constexpr int W = 16 / sizeof(T);
    const size_t n = p.n, nvec = (n + W - 1) / W, vpb = (nvec + p.nb - 1) / p.nb;
    const int m0 = p.group_ptr[g], m1 = p.group_ptr[g + 1];
    const double cnt = (double)(m1 - m0), cnt1 = cnt - 1.0;
    const bool have_t = p.truth != nullptr;
    const TT* ts = have_t ? p.truth + p.truth_off[g] : nullptr;
    const double scale = have_t ? p.truth_scale[g] : 0.0;
    const bool vec_t = accel_aligned(ts);
    double* mean_g = p.mean ? p.mean + (size_t)g * n : nullptr;
    double* var_g = p.var ? p.var + (size_t)g * n : nullptr;
    const bool vec_m = accel_aligned(mean_g), vec_v = accel_aligned(var_g);
    double s_mean = 0.0, s_var = 0.0, s_b2 = 0.0, s_mse = 0.0, s_tt = 0.0;
    const size_t j1 = ((size_t)b + 1) * vpb < nvec ? ((size_t)b + 1) * vpb : nvec;
    for (size_t j = (size_t)b * vpb + t; j < j1; j += kEnsembleThreads) {
        const size_t e0 = j * W;
        double mean[W], ss[W], se[W], st[W], var[W];
        for (int c = 0; c < W; ++c) mean[c] = ss[c] = se[c] = st[c] = 0.0;
        if (have_t) {
            ensemble_load_wide<TT, W>(ts, e0, n, vec_t, st);
            for (int c = 0; c < W; ++c) st[c] = scale * st[c];
        }
        if (m1 - m0 <= kEnsembleHold) {
            // the members' vectors stay in registers between the two passes: kEnsembleHold loads issued back to back (slots past
            // the group reload its last member and are not used), then the same sums in the same order
            const int cn = m1 - m0;
            T x[kEnsembleHold][W];
#pragma unroll
            for (int k = 0; k < kEnsembleHold; ++k) {
                const T* xs = p.src + p.member_off[m0 + (k < cn ? k : cn - 1)];
                accel_load(xs, e0, n, accel_aligned(xs), x[k]);
            }
#pragma unroll
            for (int k = 0; k < kEnsembleHold; ++k)
                if (k < cn) {
#pragma unroll
                    for (int c = 0; c < W; ++c) mean[c] = mean[c] + (double)x[k][c];
                }
            for (int c = 0; c < W; ++c) mean[c] = mean[c] / cnt;
#pragma unroll
            for (int k = 0; k < kEnsembleHold; ++k)
                if (k < cn) {
#pragma unroll
                    for (int c = 0; c < W; ++c) {
                        const double d = (double)x[k][c] - mean[c];
                        ss[c] = ss[c] + d * d;
                        if (have_t) {
                            const double e = (double)x[k][c] - st[c];
                            se[c] = se[c] + e * e;
                        }
                    }
                }
        } else {
#pragma unroll 4
            for (int m = m0; m < m1; ++m) {
                const T* xs = p.src + p.member_off[m];
                T x[W];
                accel_load(xs, e0, n, accel_aligned(xs), x);
                for (int c = 0; c < W; ++c) mean[c] = mean[c] + (double)x[c];
            }
            for (int c = 0; c < W; ++c) mean[c] = mean[c] / cnt;
#pragma unroll 4
            for (int m = m0; m < m1; ++m) {
                const T* xs = p.src + p.member_off[m];
                T x[W];
                accel_load(xs, e0, n, accel_aligned(xs), x);
                for (int c = 0; c < W; ++c) {
                    const double d = (double)x[c] - mean[c];
                    ss[c] = ss[c] + d * d;
                    if (have_t) {
                        const double e = (double)x[c] - st[c];
                        se[c] = se[c] + e * e;
                    }
                }
            }
        }
        for (int c = 0; c < W; ++c) {
            var[c] = cnt1 > 0.0 ? ss[c] / cnt1 : 0.0;
            if (e0 + c < n) {
                s_mean = s_mean + mean[c];
                s_var = s_var + var[c];
                if (have_t) {
                    const double bias = mean[c] - st[c];
                    s_b2 = s_b2 + bias * bias;
                    s_mse = s_mse + se[c] / cnt;
                    s_tt = s_tt + st[c] * st[c];
                }
            }
        }
        if (mean_g) ensemble_store_map<W>(mean_g, e0, n, vec_m, mean);
        if (var_g) ensemble_store_map<W>(var_g, e0, n, vec_v, var);
    }
    s[0] = s_mean;
    s[1] = s_var;
    s[2] = s_b2;
    s[3] = s_mse;
    s[4] = s_tt;
}

// one step of the workgroup tree on the five sums' slots s[sum][kEnsembleThreads]
RL_HD void ensemble_tree_step(double (*s)[kEnsembleThreads], int t, int h) {
#pragma clang fp contract(off)
    if (t < h)
        for (int c = 0; c < kEnsembleSums; ++c) s[c][t] = s[c][t] + s[c][t + h];
}

// thread 0 of workgroup b of group g, after the tree
RL_HD void ensemble_write_part(double* part, int nb, int g, int b, const double (*s)[kEnsembleThreads]) {
    double* o = part + ((size_t)g * nb + b) * kEnsembleSums;
    for (int c = 0; c < kEnsembleSums; ++c) o[c] = s[c][0];
}

// TOTALS, group g: its partials summed in increasing order -> out[g][kEnsembleFields]
RL_HD void ensemble_total(const double* part, const int32_t* group_ptr, int nb, int g, double* out) {
#pragma clang fp contract(off)
    double* o = out + (size_t)g * kEnsembleFields;
    o[0] = (double)(group_ptr[g + 1] - group_ptr[g]);
    for (int c = 0; c < kEnsembleSums; ++c) {
        double v = 0.0;
        for (int b = 0; b < nb; ++b) v = v + part[((size_t)g * nb + b) * kEnsembleSums + c];
        o[1 + c] = v;
    }
}

// ---- launchers (ensemble_kernels.hip): groups [g0, g0 + groups) of the tables, on stream s; dtypes RL_F32 / RL_F64 of the source
// and the truth buffer (truth may be nullptr); mean / var / part / out are indexed by the absolute group
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t ensemble_stats(int src_dtype, int truth_dtype, const void* src, const int64_t* member_off, const int32_t* group_ptr,
                          const void* truth, const int64_t* truth_off, const double* truth_scale, double* mean, double* var,
                          double* part, size_t n, int g0, int groups, hipStream_t s);
hipError_t ensemble_totals(int src_dtype, const double* part, const int32_t* group_ptr, size_t n, int groups, double* out,
                           hipStream_t s);
#endif

}  // namespace rl
