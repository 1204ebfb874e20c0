// xcorr_kernels.hpp -- the coarse FFT cross-correlation stage of the registration (rl_register_xcorr, include/rlsted.h; DESIGN.md
// section 4k): the thread bodies of xcorr_kernels.hip, written as host-compilable templates so that the CPU tests run the very same
// code under the emulated execution model (tests/emu/xcorr_emu.cpp).  The transforms are the Stockham passes of fft_core.hpp on the
// FftCfgs of fft_configs.hpp (the row geometry of a length, which is also its column geometry up to L = 1152); nothing here is a
// second FFT.  Which instantiation a launch gets: kernel_variants.hpp (RL_XCORR_LENGTHS, for_each_xcorr, select_xcorr).
//
// Per pair (A, B) of ny x nx images and a radius R, with Ly / Lx the smallest supported lengths >= ny + R / nx + R:
//   STATS  one workgroup of 256 threads per (pair, image).  With n = ny nx and x_i the image's elements in row-major order, widened
//          to float64: thread t: s_t = ((0.0 + x_t) + x_{t+256}) + ... in increasing order; the 256 values through the halving tree
//          (s_t = s_t + s_{t+h} for t < h, h = 128, 64, ... 1); mean = s_0 / n.  The centred value is a_i = (float)(x_i - mean), the
//          energy E = sum a_i^2 with e_t = fma(a, a, e_t) over the same elements in the same order and the same tree, in float64.
//   ROW    one transform per (pair, image row y): z[x] = a[y][x] 2^-ka + i b[y][x] 2^-kb for x < nx, 0 beyond, forward transform of
//          length Lx, spectrum row stored to spec[pair][y][Lx].  2^ka <= sqrt(E_a) < 2^(ka + 1) and kb likewise (xc_norm_exp): the two
//          images enter the packed transform with norms in [1, 2), so that the rounding error of the one does not drown the other
//          (tests/xcorr_reference.py, the bound); scaling by a power of two is exact, and PEAK scales back by 2^(ka + kb) in float64.
//   COL    one work item per (pair, q), q = 0 .. Lx / 2: the columns c0 = q and c1 = (Lx - q) mod Lx of spec, rows >= ny zero, both
//          through the forward transform of length Ly.  With Z0 = column c0 at ky and Z1 = column c1 at -ky:
//              A' = Z0 + conj(Z1)   B' = (Z0 - conj(Z1)) / i   X(ky) = conj(A') B' * 0.25 / (Ly Lx)
//          (A' / 2 and B' / 2 are the spectra of a and b), inverse transform of X along the column, and of the result only the rows
//          dy in [-R, R] are stored: rows[pair][dy + R][c0], and the conjugate at [c1] (the row spectrum of a real surface).
//   INV    one inverse transform of length Lx per (pair, dy); the real parts at dx in [-R, R] are C(d): corr[pair][dy + R][dx + R].
//   PEAK   one workgroup of 256 threads per pair: v(d) = (double)C(d) / ((ny - |dy|)(nx - |dx|)), C(d) = corr 2^ka 2^kb.  Thread t owns
//          the window rows t, t + 256, ...: per row, over the columns in increasing order from 0.0, s = s + v, q = q + v v, and the first
//          maximum of the row (v > best).  Thread 0 then walks the rows in increasing order: S = S + s_row, Q = Q + q_row, the first
//          maximum (row maximum > best).  E_a <= 0 or E_b <= 0 (or nan): d = (0, 0), v = 0.
// No atomics, every sum in a fixed order: results are bit-identical from run to run, and a pair's numbers do not depend on the other
// pairs of a call.  Nothing outside an image is read: the padding is formed in LDS.
// Work split of the transform kernels: a transform takes T threads (FftCfg::T); a workgroup holds G whole transforms in thread
// order (XcGroup: 256 / T for the sub-wave geometries, 4 waves for T = 64, one transform for the workgroup-synchronous L = 1152).
// Work items past the end are computed on the last item and not stored, so that every barrier is met by every thread.
// LDS: G * LdsSlots<Cfg> complex floats (ROW, INV), twice that (COL); 4 (2 R + 1) doubles (PEAK).
#pragma once
#include "accel_kernels.hpp"
#include "fft_configs.hpp"

#include <cstddef>
#include <cstdint>

namespace rl {

constexpr int kXcFields = 7;         // dy, dx, v, E_a, E_b, sum v, sum v^2 (RL_XCORR_FIELDS)
constexpr int kXcThreads = 256;      // STATS and PEAK workgroups
constexpr int kXcMaxL = 1152;        // the largest length served (the longer ones have their own column geometry)
enum XcStage { XC_ROW = 0, XC_COL = 1, XC_INV = 2 };

struct XcArgs {
    const void* a;               // reference images
    const void* b;               // moving images
    int a_f64, b_f64;            // element types: 0 float, 1 double
    const long long* a_off;      // [pairs] element offsets (device)
    const long long* b_off;
    int pairs, ny, nx, R, Ly, Lx;
    double* stats;               // [pairs][4]: mean a, mean b, E_a, E_b
    cx<float>* spec;             // [pairs][ny][Lx]
    cx<float>* rows;             // [pairs][2 R + 1][Lx]
    float* corr;                 // [pairs][2 R + 1][2 R + 1]
    double* peaks;               // [pairs][kXcFields]
    float* surf;                 // [pairs][2 R + 1][2 R + 1], or nullptr
    const cx<float>* tw_y;       // per-pass twiddles of Ly / Lx (fft_core.hpp PassTw)
    const cx<float>* tw_x;
};

template <class Cfg>
struct XcGroup {
    static constexpr int T = Cfg::T;
    static constexpr int G = T > 64 ? 1 : (T == 64 ? 4 : kXcThreads / T);   // whole transforms per workgroup
    static constexpr int THREADS = G * T;
    static constexpr int SLOTS = LdsSlots<Cfg>::value;                      // complex values of one transform's LDS
    static_assert(T > 64 || THREADS % 64 == 0, "whole waves");
};
template <class Cfg>
using XcView = LdsView<float, 1, LdsGather<Cfg::L>::value, LdsPadShift<Cfg::L>::value>;
template <class Cfg>
RL_HD size_t xc_lds_bytes(int stage) { return (size_t)(stage == XC_COL ? 2 : 1) * XcGroup<Cfg>::G * XcGroup<Cfg>::SLOTS * sizeof(cx<float>); }
RL_HD size_t xc_peak_lds_bytes(int R) { return (size_t)4 * (2 * R + 1) * sizeof(double); }
template <class Cfg>
RL_HD long long xc_items(const XcArgs& p, int stage) {
    return (long long)p.pairs * (stage == XC_ROW ? p.ny : stage == XC_COL ? p.Lx / 2 + 1 : 2 * p.R + 1);
}
template <class Cfg>
RL_HD long long xc_blocks(const XcArgs& p, int stage) { return (xc_items<Cfg>(p, stage) + XcGroup<Cfg>::G - 1) / XcGroup<Cfg>::G; }

RL_HD double xc_load(const void* p, int f64, long long i) { return f64 ? ((const double*)p)[i] : (double)((const float*)p)[i]; }
RL_HD float xc_centre(double x, double mean) { return (float)(x - mean); }
// k with 2^k <= sqrt(E) < 2^(k + 1) for a normal positive E, else 0; and 2^k as a double (|k| <= 512)
RL_HD int xc_norm_exp(double E) {
    if (!(E > 0.0)) return 0;
    unsigned long long bits;
    __builtin_memcpy(&bits, &E, sizeof bits);
    const int be = (int)((bits >> 52) & 0x7ff);
    if (be == 0 || be == 0x7ff) return 0;
    const int ex = be - 1023;
    return ex >= 0 ? ex / 2 : -((1 - ex) / 2);
}
RL_HD double xc_pow2(int k) {
    const unsigned long long bits = (unsigned long long)(1023 + k) << 52;
    double d;
    __builtin_memcpy(&d, &bits, sizeof d);
    return d;
}

// f(element index, value) for every value thread t holds after the LAST pass of a transform (fft_core.hpp run_passes)
template <class Cfg, bool INV, class F>
RL_HD void xc_outputs(const cx<float>* v, cx<float> tl, int t, F&& f) {
    using PL = PassInfo<Cfg, INV, Cfg::NP - 1>;
#pragma unroll
    for (int nb = 0; nb < PL::NBM; ++nb) {
        const int j = t + nb * Cfg::T;
        if (j < PL::NBF) {
#pragma unroll
            for (int r = 0; r < PL::R; ++r) f(j + r * PL::NBF, v[nb * PL::R + r]);
        }
    }
    if constexpr (PL::TAIL) f((64 + (t & 7)) + bitrev3(t >> 3) * PL::NBF, tl);
}

// ---- STATS: workgroup `block` = 2 * pair + image; sm: kXcThreads doubles
template <class Sync>
RL_HD void xc_stats_body(const XcArgs& p, int t, long long block, double* sm, Sync& sync) {
#pragma clang fp contract(off)
    const long long pair = block / 2;
    const int which = (int)(block % 2);
    const void* img = which ? p.b : p.a;
    const int f64 = which ? p.b_f64 : p.a_f64;
    const long long off = (which ? p.b_off : p.a_off)[pair], n = (long long)p.ny * p.nx;
    double s = 0.0;
    for (long long i = t; i < n; i += kXcThreads) s = s + xc_load(img, f64, off + i);
    sm[t] = s;
    sync.wg();
    for (int h = kXcThreads / 2; h > 0; h >>= 1) {
        accel_tree_step(sm, t, h);
        sync.wg();
    }
    const double mean = sm[0] / (double)n;
    sync.wg();
    double e = 0.0;
    for (long long i = t; i < n; i += kXcThreads) {
        const double a = (double)xc_centre(xc_load(img, f64, off + i), mean);
        e = __builtin_fma(a, a, e);
    }
    sm[t] = e;
    sync.wg();
    for (int h = kXcThreads / 2; h > 0; h >>= 1) {
        accel_tree_step(sm, t, h);
        sync.wg();
    }
    if (t == 0) {
        p.stats[pair * 4 + which] = mean;
        p.stats[pair * 4 + 2 + which] = sm[0];
    }
}

// ---- ROW: Cfg of length Lx
template <class Cfg, class Sync>
RL_HD void xc_row_body(const XcArgs& p, int tid, long long block, cx<float>* lds, Sync& sync) {
    using GR = XcGroup<Cfg>;
    constexpr int T = Cfg::T, L = Cfg::L;
    const int grp = tid / T, t = tid % T;
    const long long items = xc_items<Cfg>(p, XC_ROW);
    long long item = block * GR::G + grp;
    const bool live = item < items;
    if (!live) item = items - 1;
    const long long pair = item / p.ny;
    const int y = (int)(item % p.ny);
    XcView<Cfg> view{lds + grp * GR::SLOTS};
    const double ma = p.stats[pair * 4], mb = p.stats[pair * 4 + 1];
    const double fa = xc_pow2(-xc_norm_exp(p.stats[pair * 4 + 2])), fb = xc_pow2(-xc_norm_exp(p.stats[pair * 4 + 3]));
    const long long ao = p.a_off[pair] + (long long)y * p.nx, bo = p.b_off[pair] + (long long)y * p.nx;
    for (int x = t; x < L; x += T)
        view.at(x) = x < p.nx ? mk<float>((float)((xc_load(p.a, p.a_f64, ao + x) - ma) * fa), (float)((xc_load(p.b, p.b_f64, bo + x) - mb) * fb))
                              : mk<float>(0.0f, 0.0f);
    fft_sync<Cfg>(sync);
    cx<float> v[CfgRegs<Cfg>::VMAX];
    cx<float> tl = mk<float>(0.0f, 0.0f);
    run_passes<Cfg, false, 0, false>(v, tl, t, view, p.tw_x, sync);
    cx<float>* out = p.spec + ((size_t)pair * p.ny + y) * L;
    xc_outputs<Cfg, false>(v, tl, t, [&](int e, cx<float> z) {
        if (live) out[e] = z;
    });
}

// ---- COL: Cfg of length Ly
template <class Cfg, class Sync>
RL_HD void xc_col_body(const XcArgs& p, int tid, long long block, cx<float>* lds, Sync& sync) {
    using GR = XcGroup<Cfg>;
    constexpr int T = Cfg::T, L = Cfg::L;
    const int grp = tid / T, t = tid % T;
    const int nq = p.Lx / 2 + 1;
    const long long items = xc_items<Cfg>(p, XC_COL);
    long long item = block * GR::G + grp;
    const bool live = item < items;
    if (!live) item = items - 1;
    const long long pair = item / nq;
    const int c0 = (int)(item % nq), c1 = (p.Lx - c0) % p.Lx;
    XcView<Cfg> view0{lds + (2 * grp) * GR::SLOTS}, view1{lds + (2 * grp + 1) * GR::SLOTS};
    const cx<float>* s = p.spec + (size_t)pair * p.ny * p.Lx;
    for (int y = t; y < L; y += T) {
        view0.at(y) = y < p.ny ? s[(size_t)y * p.Lx + c0] : mk<float>(0.0f, 0.0f);
        view1.at(y) = y < p.ny ? s[(size_t)y * p.Lx + c1] : mk<float>(0.0f, 0.0f);
    }
    fft_sync<Cfg>(sync);
    cx<float> v[CfgRegs<Cfg>::VMAX];
    cx<float> tl = mk<float>(0.0f, 0.0f);
    run_passes<Cfg, false, 0, false>(v, tl, t, view0, p.tw_y, sync);
    fft_sync<Cfg>(sync);   // the last pass has been read by every thread: back to natural order
    xc_outputs<Cfg, false>(v, tl, t, [&](int e, cx<float> z) { view0.at(e) = z; });
    run_passes<Cfg, false, 0, false>(v, tl, t, view1, p.tw_y, sync);
    fft_sync<Cfg>(sync);
    xc_outputs<Cfg, false>(v, tl, t, [&](int e, cx<float> z) { view1.at(e) = z; });
    fft_sync<Cfg>(sync);
    const float sc = 0.25f / ((float)L * (float)p.Lx);
    for (int k = t; k < L; k += T) {
        const cx<float> z0 = view0.at(k), z1 = view1.at((L - k) % L);
        const cx<float> A = mk<float>(z0.re + z1.re, z0.im - z1.im);      // Z0 + conj(Z1)
        const cx<float> B = mk<float>(z0.im + z1.im, z1.re - z0.re);      // (Z0 - conj(Z1)) / i
        view0.at(k) = mk<float>((A.re * B.re + A.im * B.im) * sc, (A.re * B.im - A.im * B.re) * sc);   // conj(A) B
    }
    fft_sync<Cfg>(sync);
    run_passes<Cfg, true, 0, false>(v, tl, t, view0, p.tw_y, sync);
    const int R = p.R, W = 2 * R + 1, Lx = p.Lx;
    cx<float>* o = p.rows + (size_t)pair * W * Lx;
    xc_outputs<Cfg, true>(v, tl, t, [&](int e, cx<float> z) {
        const int w = e <= R ? e + R : e - L + R;       // dy = e or e - Ly
        if (!live || w < 0) return;
        o[(size_t)w * Lx + c0] = z;
        if (c1 != c0) o[(size_t)w * Lx + c1] = mk<float>(z.re, -z.im);
    });
}

// ---- INV: Cfg of length Lx
template <class Cfg, class Sync>
RL_HD void xc_inv_body(const XcArgs& p, int tid, long long block, cx<float>* lds, Sync& sync) {
    using GR = XcGroup<Cfg>;
    constexpr int T = Cfg::T, L = Cfg::L;
    const int grp = tid / T, t = tid % T;
    const long long items = xc_items<Cfg>(p, XC_INV);
    long long item = block * GR::G + grp;
    const bool live = item < items;
    if (!live) item = items - 1;
    XcView<Cfg> view{lds + grp * GR::SLOTS};
    const cx<float>* row = p.rows + (size_t)item * L;           // item = pair * W + w
    for (int x = t; x < L; x += T) view.at(x) = row[x];
    fft_sync<Cfg>(sync);
    cx<float> v[CfgRegs<Cfg>::VMAX];
    cx<float> tl = mk<float>(0.0f, 0.0f);
    run_passes<Cfg, true, 0, false>(v, tl, t, view, p.tw_x, sync);
    const int R = p.R, W = 2 * R + 1;
    float* o = p.corr + (size_t)item * W;
    xc_outputs<Cfg, true>(v, tl, t, [&](int e, cx<float> z) {
        const int c = e <= R ? e + R : e - L + R;       // dx = e or e - Lx
        if (live && c >= 0) o[c] = z.re;
    });
}

// ---- PEAK: workgroup `pair`; sm: 4 (2 R + 1) doubles
template <class Sync>
RL_HD void xc_peak_body(const XcArgs& p, int t, long long pair, double* sm, Sync& sync) {
#pragma clang fp contract(off)
    const int R = p.R, W = 2 * R + 1;
    const float* c = p.corr + (size_t)pair * W * W;
    float* surf = p.surf ? p.surf + (size_t)pair * W * W : nullptr;
    double *rs = sm, *rq = sm + W, *rm = sm + 2 * W, *ra = sm + 3 * W;
    const double ka = xc_pow2(xc_norm_exp(p.stats[pair * 4 + 2])), kb = xc_pow2(xc_norm_exp(p.stats[pair * 4 + 3]));
    for (int w = t; w < W; w += kXcThreads) {
        const int ady = w < R ? R - w : w - R;
        double s = 0.0, q = 0.0, best = 0.0;
        int arg = 0;
        for (int x = 0; x < W; ++x) {
            const int adx = x < R ? R - x : x - R;
            const double v = (double)c[(size_t)w * W + x] * ka * kb / ((double)(p.ny - ady) * (double)(p.nx - adx));
            s = s + v;
            q = q + v * v;
            if (x == 0 || v > best) {
                best = v;
                arg = x;
            }
            if (surf) surf[(size_t)w * W + x] = (float)v;
        }
        rs[w] = s; rq[w] = q; rm[w] = best; ra[w] = (double)arg;
    }
    sync.wg();
    if (t != 0) return;
    double S = 0.0, Q = 0.0, best = 0.0;
    int bw = 0;
    for (int w = 0; w < W; ++w) {
        S = S + rs[w];
        Q = Q + rq[w];
        if (w == 0 || rm[w] > best) {
            best = rm[w];
            bw = w;
        }
    }
    const double ea = p.stats[pair * 4 + 2], eb = p.stats[pair * 4 + 3];
    const bool flat = !(ea > 0.0) || !(eb > 0.0);
    double* o = p.peaks + (size_t)pair * kXcFields;
    o[0] = flat ? 0.0 : (double)(bw - R);
    o[1] = flat ? 0.0 : ra[bw] - (double)R;
    o[2] = flat ? 0.0 : best;
    o[3] = ea; o[4] = eb; o[5] = S; o[6] = Q;
}

// ---- launcher (xcorr_kernels.hip), on stream s: STATS, ROW, COL, INV, PEAK for a.pairs pairs.  All pointers are device pointers.
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t xcorr_pairs(const XcArgs& a, hipStream_t s);
#endif

}  // namespace rl
