// Host emulator of rl_find_peaks (rescan_line_sted_amd/csrc/bead_kernels.hpp, bead_kernels.hip): the very same thread bodies at the
// launcher's geometry, run phase by phase -- every thread of a workgroup finishes a phase before any thread starts the next, which is
// what the kernels' barriers guarantee -- with the LDS of every workgroup a heap block of exactly the kernel's byte count, poisoned
// with nan bit patterns before use.  TEST INFRASTRUCTURE ONLY -- built by tests/test_beads_cpu.py with g++ (-ffp-contract=off), as a
// shared library and, with -DBEAD_EMU_MAIN, as a stand-alone program for the sanitizers; never loaded by the product.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/bead_kernels.hpp"

using namespace rl;

namespace {

template <typename T>
struct Exact {                       // a heap block of exactly `count` elements
    T* p;
    explicit Exact(size_t count) : p((T*)std::malloc(count ? count * sizeof(T) : 1)) {}
    ~Exact() { std::free(p); }
    Exact(const Exact&) = delete;
};

void poison(void* p, size_t bytes) { std::memset(p, 0xff, bytes); }

void run_range(const BpArgs& a) {
    const long long blocks = (long long)a.n * a.nty * a.ntx;
    const size_t bytes = bp_lds_bytes(a.h, 0);
    for (long long blk = 0; blk < blocks; ++blk) {
        const BpTile T = bp_tile(a, blk, 0);
        Exact<double> lds(bytes / sizeof(double));
        poison(lds.p, bytes);
        double* U = lds.p;
        double* S = lds.p + T.UH * T.SW;
        for (int t = 0; t < kBpThreads; ++t) bp_row_body(a, T, t, U);
        for (int t = 0; t < kBpThreads; ++t) bp_col_body(a, T, t, U, S);
        double *lo = U, *hi = U + kBpThreads;
        for (int t = 0; t < kBpThreads; ++t) bp_range_body(a, T, t, S, lo, hi);
        for (int h = kBpThreads / 2; h > 0; h >>= 1)
            for (int t = 0; t < kBpThreads; ++t) bp_minmax_step(lo, hi, t, h);
        bp_range_finish(a, T, lo, hi);
    }
}

void run_levels(const BpArgs& a) {
    Exact<double> lo(kBpThreads), hi(kBpThreads);
    for (long long img = 0; img < a.n; ++img) {
        poison(lo.p, kBpThreads * sizeof(double));
        poison(hi.p, kBpThreads * sizeof(double));
        for (int t = 0; t < kBpThreads; ++t) bp_levels_body(a, img, t, lo.p, hi.p);
        for (int h = kBpThreads / 2; h > 0; h >>= 1)
            for (int t = 0; t < kBpThreads; ++t) bp_minmax_step(lo.p, hi.p, t, h);
        bp_levels_finish(a, img, lo.p, hi.p);
    }
}

void run_mark(const BpArgs& a) {
    const long long blocks = (long long)a.n * a.nty * a.ntx;
    const size_t bytes = bp_lds_bytes(a.h, a.r);
    for (long long blk = 0; blk < blocks; ++blk) {
        const BpTile T = bp_tile(a, blk, a.r);
        Exact<double> lds(bytes / sizeof(double));
        poison(lds.p, bytes);
        double* U = lds.p;
        double* S = lds.p + T.UH * T.SW;
        for (int t = 0; t < kBpThreads; ++t) bp_row_body(a, T, t, U);
        for (int t = 0; t < kBpThreads; ++t) bp_col_body(a, T, t, U, S);
        unsigned char* flags = reinterpret_cast<unsigned char*>(U);
        for (int t = 0; t < kBpThreads; ++t) bp_mark_body(a, T, t, S, flags);
        for (int t = 0; t < kBpThreads; ++t) bp_word_body(a, T, t, flags);
    }
}

void run_compact(const BpArgs& a) {
    Exact<long long> counts(kBpThreads);
    for (long long img = 0; img < a.n; ++img) {
        for (int t = 0; t < kBpThreads; ++t) counts.p[t] = bp_count_body(a, img, t);
        bp_scan_body(a, img, counts.p);
        for (int t = 0; t < kBpThreads; ++t) bp_write_body(a, img, t, counts.p[t]);
    }
}

}  // namespace

extern "C" {
// rl_find_peaks on host arrays: src at element offsets off [n]; taps [2h + 1]; yx [n][cap][2], sv / xv [n][cap], count [n], levels
// [n][3], written as the device writes them (entries past min(count, cap) untouched).  -1 on the arguments rl_find_peaks refuses.
int emu_find_peaks(const void* src, int f64, const long long* off, int n, int ny, int nx, const double* taps, int h, int r, int b, double rel,
                   double threshold, int cap, int* yx, double* sv, double* xv, long long* count, double* levels) {
    if (n < 1 || h < 0 || h > kBpMaxH || r < 1 || r > kBpMaxR || b < h + r || ny < 2 * b + 1 || nx < 2 * b + 1 || cap < 1) return -1;
    BpArgs a;
    a.src = src; a.f64 = f64; a.off = off; a.n = n; a.ny = ny; a.nx = nx; a.h = h; a.r = r; a.b = b; a.cap = cap;
    a.w = taps; a.rel = rel; a.threshold = threshold;
    a.nty = (ny - 2 * b + kBpTY - 1) / kBpTY;
    a.ntx = (nx - 2 * b + kBpTX - 1) / kBpTX;
    Exact<double> part((size_t)n * a.nty * a.ntx * 2);
    Exact<unsigned> mask((size_t)n * (ny - 2 * b) * a.ntx);
    poison(part.p, (size_t)n * a.nty * a.ntx * 2 * sizeof(double));
    poison(mask.p, (size_t)n * (ny - 2 * b) * a.ntx * sizeof(unsigned));
    a.part = part.p; a.mask = mask.p; a.levels = levels; a.count = count; a.yx = yx; a.sv = sv; a.xv = xv;
    run_range(a);
    run_levels(a);
    run_mark(a);
    run_compact(a);
    return 0;
}
// the kernel geometry the tests build their images around
int emu_tile(int axis) { return axis == 0 ? kBpTY : kBpTX; }
int emu_lds_bytes(int h, int r) { return (int)bp_lds_bytes(h, r); }
}

#ifdef BEAD_EMU_MAIN
// The stand-alone program of the sanitizer run: images, taps, outputs, partials and masks are heap blocks of EXACTLY their byte
// counts and the LDS exactly the kernel's, so a read or a write past any of them is the sanitizer's to find.  The candidates are
// held to a plain loop over the definition written here.  Prints "ok <cases>".
namespace {
unsigned g_state = 2463534242u;
long long g_found = 0, g_overflowed = 0;      // candidates seen, images whose count exceeded cap
double next_unit() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 17;
    g_state ^= g_state << 5;
    return (double)(g_state >> 8) / 16777216.0;
}

// the definition, pixel by pixel
double plain_s(const double* x, int nx, const double* w, int h, int y, int c) {
    double s = 0.0;
    for (int k = 0; k <= 2 * h; ++k) {
        double u = 0.0;
        for (int j = 0; j <= 2 * h; ++j) u = u + w[j] * x[(size_t)(y - h + k) * nx + c - h + j];
        s = s + w[k] * u;
    }
    return s;
}

template <typename T>
int peaks_case(int n, int ny, int nx, int h, int r, int b, int cap, long* done) {
    const size_t n_pix = (size_t)ny * nx;
    Exact<T> img(n * n_pix);
    Exact<double> wide(n_pix), taps(2 * h + 1);
    Exact<long long> off(n);
    double tsum = 0.0;
    for (int k = 0; k <= 2 * h; ++k) tsum += taps.p[k] = std::exp(-0.5 * (k - h) * (k - h) / 2.0);
    for (int k = 0; k <= 2 * h; ++k) taps.p[k] /= tsum;
    for (size_t i = 0; i < n * n_pix; ++i) img.p[i] = (T)(std::floor(next_unit() * 8.0) + (i % 97 == 5 ? 40.0 : 0.0));
    for (int i = 0; i < n; ++i) off.p[i] = (long long)((n - 1 - i) * n_pix);
    Exact<int> yx((size_t)n * cap * 2);
    Exact<double> sv((size_t)n * cap), xv((size_t)n * cap), levels((size_t)n * 3);
    Exact<long long> count(n);
    if (emu_find_peaks(img.p, sizeof(T) == 8, off.p, n, ny, nx, taps.p, h, r, b, 0.3, 0.0, cap, yx.p, sv.p, xv.p, count.p, levels.p)) return 1;
    for (int i = 0; i < n; ++i) {
        for (size_t k = 0; k < n_pix; ++k) wide.p[k] = (double)img.p[off.p[i] + k];
        const double t = levels.p[3 * i + 2];
        long long k = 0;
        for (int y = b; y < ny - b; ++y)
            for (int x = b; x < nx - b; ++x) {
                const double sp = plain_s(wide.p, nx, taps.p, h, y, x);
                bool c = sp >= t;
                for (int dy = -r; dy <= r && c; ++dy)
                    for (int dx = -r; dx <= r && c; ++dx) {
                        if (!dy && !dx) continue;
                        const double q = plain_s(wide.p, nx, taps.p, h, y + dy, x + dx);
                        c = (dy < 0 || (dy == 0 && dx < 0)) ? q < sp : q <= sp;
                    }
                if (!c) continue;
                if (k < cap) {
                    const size_t o = (size_t)i * cap + k;
                    if (yx.p[2 * o] != y || yx.p[2 * o + 1] != x || sv.p[o] != sp || xv.p[o] != wide.p[(size_t)y * nx + x]) {
                        std::printf("image %d candidate %lld: (%d, %d) %.17g, expected (%d, %d) %.17g\n", i, k, yx.p[2 * o], yx.p[2 * o + 1], sv.p[o], y, x, sp);
                        return 1;
                    }
                }
                ++k;
            }
        g_found += k;
        g_overflowed += k > cap;
        if (k != count.p[i]) {
            std::printf("image %d: count %lld, expected %lld\n", i, count.p[i], k);
            return 1;
        }
    }
    ++*done;
    return 0;
}
}  // namespace

int main() {
    long done = 0;
    if (peaks_case<float>(3, 2 * kBpTY + 5 + 2 * 7, 2 * kBpTX + 3 + 2 * 7, 4, 3, 7, 64, &done)) return 1;
    if (peaks_case<double>(2, 2 * kBpTY + 1 + 2 * 5, kBpTX + 9 + 2 * 5, 2, 2, 5, 3, &done)) return 1;
    if (peaks_case<double>(1, 2 * 32 + 1, 2 * 32 + 1, 16, 16, 32, 8, &done)) return 1;      // the largest LDS, a domain of one pixel
    if (peaks_case<float>(2, 2 * 1 + 20, 2 * 1 + 40, 0, 1, 1, 500, &done)) return 1;
    if (g_found < 20 || g_overflowed < 2) {        // the cases must exercise the candidates and the cap
        std::printf("found %lld, overflowed %lld\n", g_found, g_overflowed);
        return 1;
    }
    std::printf("ok %ld\n", done);
    return 0;
}
#endif
