// calib_kernels.hpp -- camera calibration (rl_calib_*, rl_repair_pixels, include/rlsted.h): the thread bodies
// of calib_kernels.hip, written as host-compilable templates so that the CPU tests run the very same code (tests/emu/calib_emu.cpp),
// the host's defect list, and the launchers.
//
// ACCUMULATE  raw (TR: u8, u16, i16, f32), n_frames sensor frames of src_ny x src_pitch elements -> per pixel of the window
//   (y0, x0) + ny x nx the two running sums S = sum x and Q = sum x^2.
//     integer TR: S int64, Q uint64, exact.  At most kCalibMaxFrames = 65535 frames in all, so that F Q and S^2 stay below 2^64.
//     f32:        S, Q float64:  S = S + (double)x;  Q = Q + (double)x * (double)x, frame after frame, no contraction (the product
//                 of two widened floats is exact in float64).
//   Work split: the window is ny * ceil(nx / 8) vectors of W = 8 adjacent pixels, ONE vector per thread, 256 threads per workgroup;
//   a thread loops over its frames with 16 accumulators in registers and reads one unaligned run per frame (tile_load_run: 16 bytes
//   of u16) where the vector is whole, element loads at a partial row end: nothing outside the window is read.  Integer types: when
//   the window alone gives fewer than kCalibTargetGroups workgroups, the frames of the call are split over the grid's y axis in
//   `parts` runs of fpp = ceil(n_frames / parts) frames (at least kCalibMinFramesPerPart each) and every part adds its sums to the
//   accumulators with 64-bit integer atomics; integer addition is associative, so the result is the same bits in any split and any
//   order.  With parts == 1 (always for f32) the thread owns its pixels: acc = acc + local, no atomics.
// FINALIZE  one pixel per thread, float64:
//     integer:  mean = (double)S / (double)F;  N = F Q - S^2 in uint64 (exact, >= 0);  var = F > 1 ? (double)N / (double)(F (F - 1)) : 0
//     f32:      mean = S / F;  var = F > 1 ? (Q - S mean) / (F - 1) : 0, no contraction
// REPAIR  img [n_images][ny][nx] (T: f32, f64) in place, one thread per (image, listed defect).  The host lists every defect that can
//   be repaired with its ring radius r and a bit per position of its (2 r + 1)^2 window, row-major, set where the neighbour is
//   inside the image and not a defect (repair_list).  The c candidates are ranked by re-reading: rank(i) = the number of candidates
//   j that sort before i (smaller, or equal with j before i; nan last); the replacement is the candidate of rank (c - 1) / 2 for odd
//   c, ((double)v[c/2 - 1] + (double)v[c/2]) * 0.5 rounded once to T for even c.  The kernel reads only pixels that are NOT defects
//   and writes only pixels that ARE: in place is free of races by construction.  No per-thread arrays, no LDS, no scratch.
#pragma once
#include "tile_kernels.hpp"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace rl {

constexpr int kCalibThreads = 256;          // four waves
constexpr int kCalibW = 8;                  // pixels per thread
constexpr int kCalibMaxFrames = 65535;      // integer accumulators: F Q and S^2 below 2^64
constexpr int kCalibTargetGroups = 1024;    // workgroups a launch aims at (four per CU)
constexpr int kCalibMinFramesPerPart = 8;   // a part of the frame split is at least this long
constexpr int kRepairMaxRadius = 3;         // (2 * 3 + 1)^2 = 49 window positions: one 64-bit word

template <typename TR> struct CalibAcc { typedef long long S; typedef unsigned long long Q; static constexpr bool integer = true; };
template <> struct CalibAcc<float> { typedef double S; typedef double Q; static constexpr bool integer = false; };

RL_HD size_t calib_vectors(int ny, int nx) { return (size_t)ny * (size_t)((nx + kCalibW - 1) / kCalibW); }
RL_HD int calib_groups(size_t nvec) { return (int)((nvec + kCalibThreads - 1) / kCalibThreads); }
// parts of the frame split of an integer accumulate: 1 where the window fills the device or the call is short
RL_HD int calib_parts(int groups, int n_frames, bool integer) {
    if (!integer || groups >= kCalibTargetGroups) return 1;
    int parts = (kCalibTargetGroups + groups - 1) / groups;
    const int most = n_frames / kCalibMinFramesPerPart;
    if (parts > most) parts = most;
    return parts < 1 ? 1 : parts;
}
// may n_frames more be added to an accumulator that holds `frames`?
RL_HD bool calib_frames_ok(bool integer, long long frames, int n_frames) {
    return n_frames >= 1 && frames >= 0 && (!integer || frames + (long long)n_frames <= (long long)kCalibMaxFrames);
}

template <typename TR>
struct CalibParams {
    const TR* raw;                         // n_frames x src_ny x src_pitch
    typename CalibAcc<TR>::S* sum;         // [ny][nx]
    typename CalibAcc<TR>::Q* sumsq;       // [ny][nx]
    size_t src_elems;                      // src_ny * src_pitch
    int src_pitch, y0, x0, ny, nx, cpr, n_frames, parts, fpp;
};

template <typename TR>
inline CalibParams<TR> calib_params(const void* raw, void* sum, void* sumsq, int src_ny, int src_pitch, int y0, int x0, int ny, int nx,
                                    int n_frames, int parts) {
    CalibParams<TR> p;
    p.raw = (const TR*)raw;
    p.sum = (typename CalibAcc<TR>::S*)sum;
    p.sumsq = (typename CalibAcc<TR>::Q*)sumsq;
    p.src_elems = (size_t)src_ny * (size_t)src_pitch;
    p.src_pitch = src_pitch; p.y0 = y0; p.x0 = x0; p.ny = ny; p.nx = nx;
    p.cpr = (nx + kCalibW - 1) / kCalibW;
    p.n_frames = n_frames;
    p.parts = parts;
    p.fpp = (n_frames + parts - 1) / parts;
    return p;
}

// acc += v: the thread's own pixel (plain) or, in a frame split, a pixel it shares with the other parts (64-bit integer atomic)
RL_HD void calib_add(long long* acc, long long v, bool shared) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (shared) {
        atomicAdd((unsigned long long*)acc, (unsigned long long)v);   // (two's complement: the same bits as the signed sum)
        return;
    }
#endif
    *acc = *acc + v;
}
RL_HD void calib_add(unsigned long long* acc, unsigned long long v, bool shared) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (shared) {
        atomicAdd(acc, v);
        return;
    }
#endif
    *acc = *acc + v;
}
RL_HD void calib_add(double* acc, double v, bool) { *acc = v; }   // (f32 raw: the thread continued from the stored sum)

// ACCUMULATE, thread t of workgroup b of part `part`
template <typename TR>
RL_HD void calib_accumulate_thread(const CalibParams<TR>& p, int b, int t, int part) {
#pragma clang fp contract(off)
    constexpr int W = kCalibW;
    typedef typename CalibAcc<TR>::S S;
    typedef typename CalibAcc<TR>::Q Q;
    const size_t j = (size_t)b * kCalibThreads + (size_t)t;
    if (j >= (size_t)p.ny * (size_t)p.cpr) return;
    const int f0 = part * p.fpp, f1 = f0 + p.fpp < p.n_frames ? f0 + p.fpp : p.n_frames;
    if (f0 >= f1) return;
    size_t y;
    int c;
    tile_divmod(j, p.cpr, y, c);
    const int x0 = c * W;
    const bool whole = x0 + W <= p.nx;
    const size_t pix = y * (size_t)p.nx + (size_t)x0;
    S s[W];
    Q q[W];
    for (int e = 0; e < W; ++e) {
        s[e] = S(0);
        q[e] = Q(0);
    }
    if (!CalibAcc<TR>::integer)   // the order is the definition: go on from the stored sums
        for (int e = 0; e < W; ++e)
            if (x0 + e < p.nx) {
                s[e] = p.sum[pix + e];
                q[e] = p.sumsq[pix + e];
            }
    const TR* src = p.raw + (size_t)f0 * p.src_elems + ((size_t)p.y0 + y) * (size_t)p.src_pitch + (size_t)p.x0 + (size_t)x0;
    for (int f = f0; f < f1; ++f, src += p.src_elems) {
        TR in[W];
        if (whole) {
            tile_load_run<TR, W>(src, in);
        } else {
            for (int e = 0; e < W; ++e) in[e] = x0 + e < p.nx ? src[e] : TR(0);
        }
        for (int e = 0; e < W; ++e) {
            const S x = (S)in[e];
            const S xx = x * x;
            s[e] = s[e] + x;
            q[e] = q[e] + (Q)xx;
        }
    }
    const bool shared = p.parts > 1;
    for (int e = 0; e < W; ++e)
        if (x0 + e < p.nx) {
            calib_add(p.sum + pix + e, s[e], shared);
            calib_add(p.sumsq + pix + e, q[e], shared);
        }
}

// FINALIZE, pixel i
RL_HD void calib_finalize_int(const long long* sum, const unsigned long long* sumsq, long long frames, size_t i, double* mean, double* var) {
#pragma clang fp contract(off)
    const long long S = sum[i];
    const unsigned long long F = (unsigned long long)frames, Q = sumsq[i], N = F * Q - (unsigned long long)S * (unsigned long long)S;
    if (mean) mean[i] = (double)S / (double)frames;
    if (var) var[i] = frames > 1 ? (double)N / (double)(F * (F - 1)) : 0.0;
}
RL_HD void calib_finalize_f32(const double* sum, const double* sumsq, long long frames, size_t i, double* mean, double* var) {
#pragma clang fp contract(off)
    const double S = sum[i], Q = sumsq[i], F = (double)frames;
    const double m = S / F;
    if (mean) mean[i] = m;
    if (var) {
        const double sm = S * m;
        const double num = Q - sm;
        var[i] = frames > 1 ? num / (F - 1.0) : 0.0;
    }
}

// ---- repair ----------------------------------------------------------------------------------------------------------------------
struct RepairEntry {
    int32_t pixel;                 // y * nx + x of the defect
    int32_t r;                     // its ring radius, 1 .. kRepairMaxRadius
    unsigned long long bits;       // bit (dy + r) * (2 r + 1) + (dx + r): the neighbour is inside the image and not a defect
};

// The defects of mask [ny][nx] (nonzero = defect) that have a good pixel within `radius`, in row-major order, each with the first
// ring r = 1 .. radius that holds one; *defects: all defects, *unrepaired: those without.
inline void repair_list(const unsigned char* mask, int ny, int nx, int radius, std::vector<RepairEntry>& list, long long* defects,
                        long long* unrepaired) {
    list.clear();
    long long n_def = 0, n_un = 0;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            if (!mask[(size_t)y * nx + x]) continue;
            ++n_def;
            bool found = false;
            for (int r = 1; r <= radius && !found; ++r) {
                unsigned long long bits = 0;
                const int w = 2 * r + 1;
                for (int dy = -r; dy <= r; ++dy)
                    for (int dx = -r; dx <= r; ++dx) {
                        const int yy = y + dy, xx = x + dx;
                        if (yy < 0 || yy >= ny || xx < 0 || xx >= nx || mask[(size_t)yy * nx + xx]) continue;
                        bits |= 1ull << ((dy + r) * w + (dx + r));
                    }
                if (bits) {
                    RepairEntry e;
                    e.pixel = (int32_t)((size_t)y * nx + x);
                    e.r = r;
                    e.bits = bits;
                    list.push_back(e);
                    found = true;
                }
            }
            if (!found) ++n_un;
        }
    if (defects) *defects = n_def;
    if (unrepaired) *unrepaired = n_un;
}

// does candidate (a, ia) sort before candidate (b, ib)?  Ascending, nan last, equal values in row-major order
template <typename T>
RL_HD bool repair_before(T a, int ia, T b, int ib) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an == bn ? ia < ib : bn;
    return a < b || (a == b && ia < ib);
}

// REPAIR, listed defect `entry` of image img [ny * nx]
template <typename T>
RL_HD void repair_thread(T* img, int nx, const RepairEntry& entry) {
#pragma clang fp contract(off)
    const int r = entry.r, w = 2 * r + 1, n = w * w;
    const unsigned long long bits = entry.bits;
    int c = 0;
    for (int i = 0; i < n; ++i) c += (int)((bits >> i) & 1ull);
    if (c == 0) return;
    const int k_lo = (c - 1) / 2, k_hi = c / 2;
    const ptrdiff_t win = (ptrdiff_t)entry.pixel - (ptrdiff_t)r * nx - r;    // (only the positions of set bits are touched)
    T lo = T(0), hi = T(0);
    for (int i = 0, iy = 0, ix = 0; i < n; ++i) {
        if ((bits >> i) & 1ull) {
            const T v = img[win + (ptrdiff_t)iy * nx + ix];
            int rank = 0;
            for (int j = 0, jy = 0, jx = 0; j < n; ++j) {
                if (j != i && ((bits >> j) & 1ull)) rank += repair_before(img[win + (ptrdiff_t)jy * nx + jx], j, v, i) ? 1 : 0;
                if (++jx == w) {
                    jx = 0;
                    ++jy;
                }
            }
            if (rank == k_lo) lo = v;
            if (rank == k_hi) hi = v;
        }
        if (++ix == w) {
            ix = 0;
            ++iy;
        }
    }
    if (k_lo == k_hi) {
        img[entry.pixel] = lo;
    } else {
        const double s = (double)lo + (double)hi;
        img[entry.pixel] = (T)(s * 0.5);
    }
}

// ---- launchers (calib_kernels.hip), on stream s.  All pointers are device pointers.
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t calib_accumulate(int raw_dtype, const void* raw, void* sum, void* sumsq, int src_ny, int src_pitch, int y0, int x0, int ny,
                            int nx, int n_frames, hipStream_t s);
hipError_t calib_finalize(int raw_dtype, const void* sum, const void* sumsq, long long frames, size_t n_pix, double* mean, double* var,
                          hipStream_t s);
hipError_t repair(int dtype, void* img, int n_images, size_t n_pix, int nx, const RepairEntry* list, int n_list, hipStream_t s);
#endif

}  // namespace rl
