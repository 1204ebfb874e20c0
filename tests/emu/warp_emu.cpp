// Host emulator of the affine kernels (rescan_line_sted_amd/csrc/affine_kernels.hpp, affine_kernels.hip): the very same thread
// bodies, run thread by thread over the launch grids -- the prefilter through the shift's own passes with the product's prefilter
// taps (warp_prefilter_taps), the evaluation tile by tile with the footprint staged in an "LDS" array of exactly kWarpLds doubles or
// read directly, the workgroup tree and the totals of its statistics; the affine sums run by run with the tree in batches of nine
// fields and the totals in the kernel's order.  TEST INFRASTRUCTURE ONLY -- built by tests/test_affine_cpu.py with g++
// (-ffp-contract=off), as a shared library and, with -DWARP_EMU_MAIN, as a stand-alone program for the sanitizers; never loaded by the
// product.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/affine_kernels.hpp"

using namespace rl;

namespace {

template <typename TS, typename TD, int AXIS, bool FINAL>
void pass_run(const ShiftArgs& a) {
    const ShiftParams<TS, TD> p = shift_params<TS, TD>(a);
    const int nb = p.nby * p.nbx;
    std::vector<double> lds(kShiftLds);
    for (size_t block = 0; block < (size_t)a.n * nb; ++block) {
        const size_t i = block / nb;
        const int by = (int)(block % nb) / p.nbx, bx = (int)(block % nb) % p.nbx;
        for (int t = 0; t < kRegThreads; ++t) shift_stage<TS, TD, AXIS>(p, i, by, bx, t, lds.data());
        for (int t = 0; t < kRegThreads; ++t) {
            double sums[kShiftFields];
            shift_compute<TS, TD, AXIS, FINAL>(p, i, by, bx, t, lds.data(), sums);
        }
    }
}

// the tiles of k_warp_eval; staged_out counts the tiles that went through the "LDS"
template <typename TS, typename TD, int ORDER>
void eval_run(const WarpArgs& a, long* staged_out) {
    const WarpParams<TS, TD> p = warp_params<TS, TD>(a);
    const int nb = p.nby * p.nbx;
    std::vector<double> lds(kWarpLds), sm[kWarpFields];
    for (auto& s : sm) s.resize(kRegThreads);
    for (size_t block = 0; block < (size_t)a.n * nb; ++block) {
        const size_t i = block / nb;
        const int by = (int)(block % nb) / p.nbx, bx = (int)(block % nb) % p.nbx;
        const TS* s = p.src + i * (size_t)p.sy * p.sx;
        const WarpBox box = warp_box<ORDER>(p.xf + i * kWarpXf, p.oy, p.ox, by, bx, p.direct);
        if (box.staged) {
            std::fill(lds.begin(), lds.end(), NAN);
            for (int t = 0; t < kRegThreads; ++t) warp_stage<TS>(s, p.sy, p.sx, box, t, lds.data());
            ++*staged_out;
        }
        for (int t = 0; t < kRegThreads; ++t) {
            double sums[kWarpFields];
            if (box.staged) {
                const WarpFetchLds fetch{lds.data(), box.y0, box.x0, box.cols};
                warp_compute<TS, TD, ORDER>(p, i, by, bx, t, fetch, sums);
            } else {
                const WarpFetchGlobal<TS> fetch{s, p.sy, p.sx};
                warp_compute<TS, TD, ORDER>(p, i, by, bx, t, fetch, sums);
            }
            for (int f = 0; f < kWarpFields; ++f) sm[f][t] = sums[f];
        }
        if (!p.part) continue;
        for (int h = kRegThreads / 2; h > 0; h >>= 1)
            for (int f = 0; f < kWarpFields; ++f)
                for (int t = 0; t < kRegThreads; ++t) accel_tree_step(sm[f].data(), t, h);
        for (int f = 0; f < kWarpFields; ++f) p.part[block * kWarpFields + f] = sm[f][0];
    }
}

template <typename TA, typename TW>
void aff_run(const AffArgs& a) {
    const AffParams<TA, TW> p = aff_params<TA, TW>(a);
    const AffGeom& g = a.g;
    std::vector<double> acc((size_t)kRegThreads * kAffFields), sm((size_t)kAffBatch * kRegThreads);
    for (int pair = 0; pair < a.pairs; ++pair)
        for (unsigned b = 0; b < g.nb; ++b) {
            for (int t = 0; t < kRegThreads; ++t) aff_accumulate<TA, TW>(p, pair, b, t, &acc[(size_t)t * kAffFields]);
            double* out = a.part + ((size_t)pair * g.nb + b) * kAffFields;
            for (int f0 = 0; f0 < kAffFields; f0 += kAffBatch) {
                for (int t = 0; t < kRegThreads; ++t)
                    for (int f = 0; f < kAffBatch; ++f) sm[(size_t)f * kRegThreads + t] = acc[(size_t)t * kAffFields + f0 + f];
                for (int h = kRegThreads / 2; h > 0; h >>= 1)
                    for (int f = 0; f < kAffBatch; ++f)
                        for (int t = 0; t < kRegThreads; ++t) accel_tree_step(&sm[(size_t)f * kRegThreads], t, h);
                for (int f = 0; f < kAffBatch; ++f) out[f0 + f] = sm[(size_t)f * kRegThreads];
            }
        }
    for (size_t id = 0; id < (size_t)a.pairs * kAffFields; ++id)
        a.tot[id] = ingest_total(a.part + (id / kAffFields) * g.nb * kAffFields, (int)g.nb, kAffFields, (int)(id % kAffFields));
}

}  // namespace

extern "C" {
// dtypes: 0 f32, 1 f64.  src [n][sy][sx] -> dst [n][oy][ox]; xf [n][6]; stats NULL or [n][2]; direct: 1 stages no tile; staged_out:
// NULL or the number of tiles that were staged.  The caller has checked the arguments as rl_warp_images does.
int emu_warp_images(const void* src, int src_dtype, int n, int sy, int sx, const double* xf, int order, double floor, void* dst, int dst_dtype,
                    int oy, int ox, double* stats, int direct, long* staged_out) {
    if (n < 1 || sy < 1 || sx < 1 || oy < 1 || ox < 1 || (order != 1 && order != 3)) return -1;
    const int nb = warp_blocks_y(oy) * warp_blocks_x(ox);
    std::vector<double> coef, part((size_t)n * nb * kWarpFields);
    long staged = 0;
    WarpArgs a;
    a.src = src; a.dst = dst; a.xf = xf; a.part = stats ? part.data() : nullptr;
    a.n = n; a.sy = sy; a.sx = sx; a.oy = oy; a.ox = ox; a.order = order; a.direct = direct; a.floor = floor;
    if (order == 3) {
        std::vector<ShiftImage> table((size_t)n);
        warp_prefilter_taps(sy, table[0].gy, &table[0].oy, &table[0].nty);
        warp_prefilter_taps(sx, table[0].gx, &table[0].ox, &table[0].ntx);
        for (int k = 1; k < n; ++k) table[k] = table[0];
        std::vector<double> tmp((size_t)n * sy * sx);
        coef.resize((size_t)n * sy * sx);
        ShiftArgs x;
        x.src = src; x.dst = tmp.data(); x.img = table.data(); x.part = nullptr; x.n = n; x.ny = sy; x.nx = sx; x.floor = -HUGE_VAL;
        if (src_dtype == 0) pass_run<float, double, 1, false>(x); else pass_run<double, double, 1, false>(x);
        ShiftArgs y = x;
        y.src = tmp.data(); y.dst = coef.data();
        pass_run<double, double, 0, true>(y);
        a.src = coef.data();
        if (dst_dtype == 0) eval_run<double, float, 3>(a, &staged); else eval_run<double, double, 3>(a, &staged);
    } else if (src_dtype == 0) {
        if (dst_dtype == 0) eval_run<float, float, 1>(a, &staged); else eval_run<float, double, 1>(a, &staged);
    } else {
        if (dst_dtype == 0) eval_run<double, float, 1>(a, &staged); else eval_run<double, double, 1>(a, &staged);
    }
    if (stats)
        for (size_t id = 0; id < (size_t)n * kWarpFields; ++id)
            stats[id] = ingest_total(part.data() + (id / kWarpFields) * nb * kWarpFields, nb, kWarpFields, (int)(id % kWarpFields));
    if (staged_out) *staged_out = staged;
    return 0;
}

// a / w: host arrays, offsets in elements.  sums_out [pairs][45].  geom_out: NULL or 2 ints nb, run.
int emu_affine_sums(const void* a, int a_dtype, const long long* a_off, const void* w, int w_dtype, const long long* w_off, int pairs, int ny,
                    int nx, int M, double* sums_out, int* geom_out) {
    if (M < 1 || ny - 2 * M < 8 || nx - 2 * M < 8 || pairs < 1) return -1;
    const AffGeom g = aff_geom(ny, nx, M);
    if (geom_out) {
        geom_out[0] = (int)g.nb; geom_out[1] = (int)g.run;
    }
    std::vector<double> part((size_t)pairs * g.nb * kAffFields, NAN);
    AffArgs s;
    s.a = a; s.w = w; s.a_off = a_off; s.w_off = w_off; s.part = part.data(); s.tot = sums_out; s.pairs = pairs; s.g = g;
    if (a_dtype == 0) {
        if (w_dtype == 0) aff_run<float, float>(s); else aff_run<float, double>(s);
    } else {
        if (w_dtype == 0) aff_run<double, float>(s); else aff_run<double, double>(s);
    }
    return 0;
}
}

#ifdef WARP_EMU_MAIN
// The stand-alone program of the sanitizer run: the images, the destination and the outputs are heap blocks of EXACTLY their byte
// counts (the last pair's images end with their buffers), and the "LDS" arrays are exactly the launches' sizes, so a read or a write
// past any of them is the sanitizer's to find.  Results are held to plain loops written here.  Prints "ok <warps> <sums>".
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

// three images: a rotation about the centre, an integer translation far outside, 2 x binning; both paths, the same bits
template <typename TS, typename TD>
int warp_case(int sy, int sx, int oy, int ox, int order, long* done) {
    const int n = 3;
    Exact<TS> src((size_t)n * sy * sx);
    Exact<TD> dst((size_t)n * oy * ox), again(dst.n);
    for (size_t i = 0; i < src.n; ++i) src.p[i] = (TS)(next_unit() * 50.0);
    const double c = std::cos(0.3), s = std::sin(0.3), cy = 0.5 * (sy - 1), cx = 0.5 * (sx - 1);
    const double xf[18] = {c, -s, s, c, cy - c * cy + s * cx, cx - s * cy - c * cx, 1.0, 0.0, 0.0, 1.0, -10003.0, 20001.0, 2.0, 0.0, 0.0, 2.0, 0.5, 0.5};
    Exact<double> stats((size_t)n * 2), stats2((size_t)n * 2);
    long staged = 0, none = 0;
    if (emu_warp_images(src.p, sizeof(TS) == 4 ? 0 : 1, n, sy, sx, xf, order, 1.0, dst.p, sizeof(TD) == 4 ? 0 : 1, oy, ox, stats.p, 0, &staged)) return 1;
    if (emu_warp_images(src.p, sizeof(TS) == 4 ? 0 : 1, n, sy, sx, xf, order, 1.0, again.p, sizeof(TD) == 4 ? 0 : 1, oy, ox, stats2.p, 1, &none)) return 1;
    if (staged == 0 || none != 0 || std::memcmp(dst.p, again.p, dst.n * sizeof(TD)) || std::memcmp(stats.p, stats2.p, stats.n * sizeof(double))) {
        std::printf("warp %d x %d -> %d x %d order %d: the paths differ (staged %ld, %ld)\n", sy, sx, oy, ox, order, staged, none);
        return 1;
    }
    double raised = 0;
    for (int y = 0; y < oy; ++y)
        for (int x = 0; x < ox; ++x) {
            for (int i = 0; i < n; ++i) {
                const TD got = dst.p[((size_t)i * oy + y) * ox + x];
                if (!(got >= (TD)1.0) || !(got <= (TD)200.0)) return 1;          // the floor; a spline of values in 0 .. 50 stays far below 200
            }
            const int p = sy > 1 ? 2 * (sy - 1) : 1, q = sx > 1 ? 2 * (sx - 1) : 1;   // image 1: the displaced pixel (order 3: up to rounding)
            int yy = (int)((((long long)y - 10003) % p + p) % p), xx = (int)((((long long)x + 20001) % q + q) % q);
            yy = sy == 1 ? 0 : (yy >= sy ? p - yy : yy);
            xx = sx == 1 ? 0 : (xx >= sx ? q - xx : xx);
            const double v = (double)src.p[((size_t)sy + yy) * sx + xx], want = v < 1.0 ? 1.0 : v;
            if (v < 1.0 - 1e-9) raised += 1;
            const double got = (double)dst.p[((size_t)oy + y) * ox + x];
            if (order == 1 ? got != (double)(TD)want : std::fabs(got - want) > 1e-4) {
                std::printf("warp %d x %d order %d (%d, %d): %.17g, want %.17g\n", sy, sx, order, y, x, got, want);
                return 1;
            }
        }
    if (order == 1 && stats.p[2] != raised) return 1;
    ++*done;
    return 0;
}

template <typename TA, typename TW>
int sums_case(int ny, int nx, int M, long* done) {
    const int pairs = 3;
    Exact<TA> a((size_t)2 * ny * nx);
    Exact<TW> w((size_t)pairs * ny * nx);
    for (size_t i = 0; i < a.n; ++i) a.p[i] = (TA)(next_unit() * 100.0);
    for (size_t i = 0; i < w.n; ++i) w.p[i] = (TW)(next_unit() * 100.0);
    const long long a_off[3] = {0, (long long)ny * nx, 0}, w_off[3] = {2LL * ny * nx, 0, (long long)ny * nx};
    Exact<double> sums((size_t)pairs * kAffFields);
    if (emu_affine_sums(a.p, sizeof(TA) == 4 ? 0 : 1, a_off, w.p, sizeof(TW) == 4 ? 0 : 1, w_off, pairs, ny, nx, M, sums.p, nullptr)) return 1;
    for (int i = 0; i < pairs; ++i) {
        long double want[kAffFields] = {0}, mag[kAffFields] = {0};
        for (int y = M; y < ny - M; ++y)
            for (int x = M; x < nx - M; ++x) {
                const TW* W = w.p + w_off[i] + (size_t)y * nx + x;
                const double av = a.p[a_off[i] + (size_t)y * nx + x];
                const double gy = 0.5 * ((double)W[nx] - (double)W[-nx]), gx = 0.5 * ((double)W[1] - (double)W[-1]);
                const double yc = y - 0.5 * (ny - 1), xc = x - 0.5 * (nx - 1);
                const double phi[8] = {gy, gx, gy * yc, gy * xc, gx * yc, gx * xc, (double)W[0], 1.0};
                int f = 0;
                for (int j = 0; j < 8; ++j)
                    for (int k = j; k < 8; ++k, ++f) {
                        want[f] += (long double)phi[j] * phi[k];
                        mag[f] += fabsl((long double)phi[j] * phi[k]);
                    }
                for (int j = 0; j < 8; ++j) {
                    want[36 + j] += (long double)phi[j] * av;
                    mag[36 + j] += fabsl((long double)phi[j] * av);
                }
                want[44] += (long double)av * av;
                mag[44] += (long double)av * av;
            }
        for (int f = 0; f < kAffFields; ++f)
            if (fabsl(sums.p[(size_t)i * kAffFields + f] - want[f]) > mag[f] * 1e-12L) {
                std::printf("sums %d x %d M %d pair %d field %d: %.17g\n", ny, nx, M, i, f, sums.p[(size_t)i * kAffFields + f]);
                return 1;
            }
    }
    ++*done;
    return 0;
}
}  // namespace

int main() {
    long warps = 0, sums = 0;
    const int shapes[][4] = {{37, 53, 41, 29}, {1, 17, 5, 9}, {5, 7, 40, 33}, {1, 1, 3, 3}, {70, 66, 35, 33}};
    for (const auto& sh : shapes)
        for (int order : {1, 3})
            if (warp_case<float, float>(sh[0], sh[1], sh[2], sh[3], order, &warps) || warp_case<float, double>(sh[0], sh[1], sh[2], sh[3], order, &warps) ||
                warp_case<double, float>(sh[0], sh[1], sh[2], sh[3], order, &warps) || warp_case<double, double>(sh[0], sh[1], sh[2], sh[3], order, &warps))
                return 1;
    const int cases[][3] = {{10, 10, 1}, {37, 53, 4}, {48, 64, 4}, {100, 120, 2}};
    for (const auto& c : cases)
        if (sums_case<float, float>(c[0], c[1], c[2], &sums) || sums_case<float, double>(c[0], c[1], c[2], &sums) ||
            sums_case<double, float>(c[0], c[1], c[2], &sums) || sums_case<double, double>(c[0], c[1], c[2], &sums))
            return 1;
    std::printf("ok %ld %ld\n", warps, sums);
    return 0;
}
#endif
