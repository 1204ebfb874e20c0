// Host emulator of the registration kernels (rescan_line_sted_amd/csrc/register_kernels.hpp, register_kernels.hip): the very same
// thread bodies, run thread by thread over the launch grids -- (pair, band, pass) workgroups of kRegThreads threads that stage a
// column block into an "LDS" array, meet at the barrier and walk it with their sums kept across the blocks; the totals in the
// kernel's order; the shift's two passes, tile by tile, with the workgroup tree and the totals of its statistics -- with the
// launchers' own parameters and the product's own taps (shift_taps).  TEST INFRASTRUCTURE ONLY -- built by
// tests/test_register_cpu.py with g++ (-ffp-contract=off), as a shared library and, with -DREGISTER_EMU_MAIN, as a stand-alone
// program for the sanitizers; never loaded by the product.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/register_kernels.hpp"

using namespace rl;

namespace {

template <typename TA, typename TB>
void sums_run(const RegSumArgs& a) {
    const RegGeom& g = a.g;
    const RegSumParams<TA, TB> p = reg_sum_params<TA, TB>(a);
    std::vector<double> lds(reg_lds_doubles(g));        // exactly the launch's dynamic LDS
    std::vector<double> acc((size_t)kRegThreads * kRegFields), row((size_t)kRegThreads * 2);
    for (int pair = 0; pair < a.pairs; ++pair)
        for (int band = 0; band < g.bands; ++band)
            for (int pass = 0; pass < g.passes; ++pass) {
                std::fill(acc.begin(), acc.end(), 0.0);
                std::fill(row.begin(), row.end(), 0.0);
                for (int tile = 0; tile < g.ntx; ++tile) {
                    for (int t = 0; t < kRegThreads; ++t) reg_stage<TA, TB>(p, pair, band, tile, t, lds.data());
                    for (int t = 0; t < kRegThreads; ++t) reg_walk(g, band, tile, pass, t, lds.data(), &acc[(size_t)t * kRegFields], &row[(size_t)t * 2]);
                }
                for (int t = 0; t < kRegThreads; ++t) reg_store(g, p.part, pair, band, pass, t, &acc[(size_t)t * kRegFields], &row[(size_t)t * 2]);
            }
    const int per = g.nd * kRegFields + 2;
    for (size_t id = 0; id < (size_t)a.pairs * per; ++id) a.tot[id] = reg_total(g, a.part + (id / per) * reg_part_doubles(g), (int)(id % per));
}

template <typename TS, typename TD, int AXIS, bool FINAL>
void pass_run(const ShiftArgs& a) {
    const ShiftParams<TS, TD> p = shift_params<TS, TD>(a);
    const int nb = p.nby * p.nbx;
    std::vector<double> lds(kShiftLds), sm[kShiftFields];
    for (auto& s : sm) s.resize(kRegThreads);
    for (size_t block = 0; block < (size_t)a.n * nb; ++block) {
        const size_t i = block / nb;
        const int by = (int)(block % nb) / p.nbx, bx = (int)(block % nb) % p.nbx;
        for (int t = 0; t < kRegThreads; ++t) shift_stage<TS, TD, AXIS>(p, i, by, bx, t, lds.data());
        for (int t = 0; t < kRegThreads; ++t) {
            double sums[kShiftFields];
            shift_compute<TS, TD, AXIS, FINAL>(p, i, by, bx, t, lds.data(), sums);
            for (int f = 0; f < kShiftFields; ++f) sm[f][t] = sums[f];
        }
        if (!FINAL || !p.part) continue;
        for (int h = kRegThreads / 2; h > 0; h >>= 1)
            for (int f = 0; f < kShiftFields; ++f)
                for (int t = 0; t < kRegThreads; ++t) accel_tree_step(sm[f].data(), t, h);
        for (int f = 0; f < kShiftFields; ++f) p.part[block * kShiftFields + f] = sm[f][0];
    }
}

}  // namespace

extern "C" {
// dtypes: 0 f32, 1 f64.  a / b: host arrays, offsets in elements.  sums_out [pairs][(2R+1)^2][3], ref_out [pairs][2].  The
// caller has checked the arguments as rl_register_sums does.  geom_out: NULL or 6 ints TY, G, h, passes, bands, LDS doubles.
int emu_register_sums(const void* a, int a_dtype, const long long* a_off, const void* b, int b_dtype, const long long* b_off, int pairs,
                      int ny, int nx, int R, int M, double* sums_out, double* ref_out, int* geom_out) {
    if (R < 1 || R > kRegMaxR || M < R || ny - 2 * M < 8 || nx - 2 * M < 8 || pairs < 1) return -1;
    const RegGeom g = reg_geom(ny, nx, R, M);
    if (geom_out) {
        geom_out[0] = g.TY; geom_out[1] = g.G; geom_out[2] = g.h; geom_out[3] = g.passes; geom_out[4] = g.bands; geom_out[5] = (int)reg_lds_doubles(g);
    }
    const int per = g.nd * kRegFields + 2;
    std::vector<double> part((size_t)pairs * reg_part_doubles(g), NAN), tot((size_t)pairs * per);
    RegSumArgs s;
    s.a = a; s.b = b; s.a_off = a_off; s.b_off = b_off; s.part = part.data(); s.tot = tot.data(); s.pairs = pairs; s.g = g;
    if (a_dtype == 0) {
        if (b_dtype == 0) sums_run<float, float>(s); else sums_run<float, double>(s);
    } else {
        if (b_dtype == 0) sums_run<double, float>(s); else sums_run<double, double>(s);
    }
    for (int i = 0; i < pairs; ++i) {
        std::memcpy(sums_out + (size_t)i * g.nd * kRegFields, tot.data() + (size_t)i * per, sizeof(double) * g.nd * kRegFields);
        ref_out[2 * i] = tot[(size_t)i * per + g.nd * kRegFields];
        ref_out[2 * i + 1] = tot[(size_t)i * per + g.nd * kRegFields + 1];
    }
    return 0;
}

// src [n][ny][nx] -> dst [n][ny][nx]; shifts [n][2]; stats NULL or [n][2]
int emu_shift_images(const void* src, int src_dtype, int n, int ny, int nx, const double* shifts, int order, double floor, void* dst,
                     int dst_dtype, double* stats) {
    if (n < 1 || ny < 1 || nx < 1 || (order != 1 && order != 3)) return -1;
    std::vector<ShiftImage> table((size_t)n);
    for (int i = 0; i < n; ++i) {
        shift_taps(shifts[2 * i], order, ny, table[i].gy, &table[i].oy, &table[i].nty);
        shift_taps(shifts[2 * i + 1], order, nx, table[i].gx, &table[i].ox, &table[i].ntx);
    }
    const int nb = shift_blocks_y(ny) * shift_blocks_x(nx);
    std::vector<double> tmp((size_t)n * ny * nx), part((size_t)n * nb * kShiftFields);
    ShiftArgs x;
    x.src = src; x.dst = tmp.data(); x.img = table.data(); x.part = nullptr; x.n = n; x.ny = ny; x.nx = nx; x.floor = floor;
    if (src_dtype == 0) pass_run<float, double, 1, false>(x); else pass_run<double, double, 1, false>(x);
    ShiftArgs y = x;
    y.src = tmp.data(); y.dst = dst; y.part = stats ? part.data() : nullptr;
    if (dst_dtype == 0) pass_run<double, float, 0, true>(y); else pass_run<double, double, 0, true>(y);
    if (stats)
        for (size_t id = 0; id < (size_t)n * kShiftFields; ++id)
            stats[id] = ingest_total(part.data() + (id / kShiftFields) * nb * kShiftFields, nb, kShiftFields, (int)(id % kShiftFields));
    return 0;
}
}

#ifdef REGISTER_EMU_MAIN
// The stand-alone program of the sanitizer run: the images, the destination and the outputs are heap blocks of EXACTLY their byte
// counts (the last pair's images end with their buffers), and the "LDS" arrays are exactly the launches' sizes, so a read or a
// write past any of them is the sanitizer's to find.  Results are held to plain loops written here.  Prints "ok <sums> <shifts>".
namespace {
unsigned g_state = 2463534242u;
double next_unit() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 17;
    g_state ^= g_state << 5;
    return (double)(g_state >> 8) / 16777216.0;
}
template <typename T>
struct Exact {
    T* p;
    size_t n;
    explicit Exact(size_t count) : p((T*)std::malloc(count * sizeof(T))), n(count) {}
    ~Exact() { std::free(p); }
    Exact(const Exact&) = delete;
};

template <typename TA, typename TB>
int sums_case(int ny, int nx, int R, int M, long* done) {
    const int pairs = 3, W = 2 * R + 1;
    Exact<TA> a((size_t)2 * ny * nx);
    Exact<TB> b((size_t)pairs * ny * nx);
    for (size_t i = 0; i < a.n; ++i) a.p[i] = (TA)(next_unit() * 100.0);
    for (size_t i = 0; i < b.n; ++i) b.p[i] = (TB)(next_unit() * 100.0);
    const long long a_off[3] = {0, (long long)ny * nx, 0}, b_off[3] = {2LL * ny * nx, 0, (long long)ny * nx};
    Exact<double> sums((size_t)pairs * W * W * 3), ref((size_t)pairs * 2);
    if (emu_register_sums(a.p, sizeof(TA) == 4 ? 0 : 1, a_off, b.p, sizeof(TB) == 4 ? 0 : 1, b_off, pairs, ny, nx, R, M, sums.p, ref.p, nullptr)) return 1;
    for (int i = 0; i < pairs; ++i)
        for (int d = 0; d < W * W; ++d) {
            const int dy = d / W - R, dx = d % W - R;
            long double sb = 0, sbb = 0, sab = 0, mag = 0;
            for (int y = M; y < ny - M; ++y)
                for (int x = M; x < nx - M; ++x) {
                    const long double av = a.p[a_off[i] + (size_t)y * nx + x], bv = b.p[b_off[i] + (size_t)(y + dy) * nx + x + dx];
                    sb += bv; sbb += bv * bv; sab += av * bv; mag += 1e4L;
                }
            const double* s = sums.p + ((size_t)i * W * W + d) * 3;
            const long double tol = mag * 1e-12L;
            if (fabsl(s[0] - sb) > tol || fabsl(s[1] - sbb) > tol || fabsl(s[2] - sab) > tol) {
                std::printf("sums %d x %d R %d pair %d d %d: %.17g %.17g %.17g\n", ny, nx, R, i, d, s[0], s[1], s[2]);
                return 1;
            }
        }
    ++*done;
    return 0;
}

template <typename TS, typename TD>
int shift_case(int ny, int nx, int order, long* done) {
    const int n = 3;
    Exact<TS> src((size_t)n * ny * nx);
    Exact<TD> dst(src.n);
    for (size_t i = 0; i < src.n; ++i) src.p[i] = (TS)(next_unit() * 50.0);
    const double shifts[6] = {2.0, -3.0, -(double)ny - 3.0, 2.0 * nx + 1.0, order == 1 ? 0.0 : 0.37, order == 1 ? 1.0 : -40.6};
    Exact<double> stats((size_t)n * 2);
    if (emu_shift_images(src.p, sizeof(TS) == 4 ? 0 : 1, n, ny, nx, shifts, order, 1.0, dst.p, sizeof(TD) == 4 ? 0 : 1, stats.p)) return 1;
    for (int i = 0; i < n; ++i) {
        double raised = 0;
        const bool whole = shifts[2 * i] == std::floor(shifts[2 * i]) && shifts[2 * i + 1] == std::floor(shifts[2 * i + 1]);
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const TD got = dst.p[((size_t)i * ny + y) * nx + x];
                if (!(got >= (TD)1.0) || !(got <= (TD)200.0)) return 1;      // the floor; a spline of values in 0 .. 50 stays far below 200
                if (whole) {                                                 // the displaced pixel (order 3: up to rounding)
                    const int p = ny > 1 ? 2 * (ny - 1) : 1, q = nx > 1 ? 2 * (nx - 1) : 1;
                    int yy = (int)(((long long)y + (long long)shifts[2 * i]) % p + p) % p, xx = (int)(((long long)x + (long long)shifts[2 * i + 1]) % q + q) % q;
                    yy = ny == 1 ? 0 : (yy >= ny ? p - yy : yy);
                    xx = nx == 1 ? 0 : (xx >= nx ? q - xx : xx);
                    const double v = (double)src.p[((size_t)i * ny + yy) * nx + xx], want = v < 1.0 ? 1.0 : v;
                    if (v < 1.0 - 1e-9) raised += 1;
                    if (order == 1 ? (double)got != (double)(TD)want : std::fabs((double)got - want) > 1e-4) {
                        std::printf("shift %d x %d order %d image %d (%d, %d): %.17g, want %.17g\n", ny, nx, order, i, y, x, (double)got, want);
                        return 1;
                    }
                }
            }
        if (whole && order == 1 && stats.p[2 * i] != raised) return 1;
    }
    ++*done;
    return 0;
}
}  // namespace

int main() {
    long sums = 0, shifts = 0;
    const int cases[][4] = {{37, 53, 2, 2}, {24, 41, 1, 3}, {40, 56, 6, 6}, {72, 48, 6, 8}, {30, 45, 9, 10}, {73, 74, 32, 32}};
    for (const auto& c : cases)
        if (sums_case<float, float>(c[0], c[1], c[2], c[3], &sums) || sums_case<float, double>(c[0], c[1], c[2], c[3], &sums) ||
            sums_case<double, float>(c[0], c[1], c[2], c[3], &sums) || sums_case<double, double>(c[0], c[1], c[2], c[3], &sums))
            return 1;
    const int shapes[][2] = {{37, 53}, {1, 70}, {33, 1}, {64, 65}};
    for (const auto& sh : shapes)
        for (int order : {1, 3})
            if (shift_case<float, float>(sh[0], sh[1], order, &shifts) || shift_case<float, double>(sh[0], sh[1], order, &shifts) ||
                shift_case<double, float>(sh[0], sh[1], order, &shifts) || shift_case<double, double>(sh[0], sh[1], order, &shifts))
                return 1;
    std::printf("ok %ld %ld\n", sums, shifts);
    return 0;
}
#endif
