// Host emulator of the coarse registration stage (rescan_line_sted_amd/csrc/xcorr_kernels.hpp, xcorr_kernels.hip): the very same
// thread bodies under the emulated execution model of emu_common.hpp -- one OS thread per GPU thread, pthread barriers for the
// workgroup and the wavefront, the cross-lane exchanges of the L = 576 tails through the wavefront's exchange array -- over the
// launch grids of xcorr_pairs, chosen through the same walk of the variant table (kernel_variants.hpp for_each_xcorr), with the
// product's own twiddle tables and "LDS" blocks of EXACTLY the launcher's byte counts, poisoned before every workgroup.
// TEST INFRASTRUCTURE ONLY -- built by tests/test_xcorr_cpu.py with g++ (-ffp-contract=off), as a shared library and, with
// -DXCORR_EMU_MAIN, as a stand-alone program for the sanitizers; never loaded by the product.
#include "emu_common.hpp"

#include "../../rescan_line_sted_amd/csrc/xcorr_kernels.hpp"

namespace {

// a grid of `blocks` workgroups of `nthreads` threads; lds: exactly lds_bytes, its own heap block
template <class Body>
void xc_run_grid(long long blocks, int nthreads, size_t lds_bytes, Body body) {
    unsigned char* lds = (unsigned char*)std::malloc(lds_bytes ? lds_bytes : 1);
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, nthreads);
    const int nwaves = (nthreads + 63) / 64;
    std::vector<pthread_barrier_t> wbar(nwaves);
    std::vector<double> xchg((size_t)nwaves * 64);
    for (int w = 0; w < nwaves; ++w) pthread_barrier_init(&wbar[w], nullptr, (w + 1) * 64 <= nthreads ? 64 : nthreads - w * 64);
    for (long long b = 0; b < blocks; ++b) {
        std::memset(lds, 0xff, lds_bytes);
        std::vector<std::thread> th;
        th.reserve(nthreads);
        for (int tid = 0; tid < nthreads; ++tid)
            th.emplace_back([&, tid]() {
                EmuSync s{&bar, &wbar[tid / 64], &xchg[(size_t)(tid / 64) * 64], tid % 64};
                body(tid, b, lds, s);
            });
        for (auto& t : th) t.join();
    }
    pthread_barrier_destroy(&bar);
    for (auto& b : wbar) pthread_barrier_destroy(&b);
    std::free(lds);
}

std::vector<cx<float>> xc_twiddles(int L) {
    std::vector<cx<float>> tw;
    for_each_xcorr([&](auto v) {
        using V = decltype(v);
        if (V::L != L || V::STAGE != 0) return false;
        tw = twiddles_of<typename CfgFor<V::L>::Cfg, float>();
        return true;
    });
    return tw;
}

// what xcorr_kernels.hip's launch_stage does; false: no such row
bool run_stage(int L, int stage, const XcArgs& a, int* threads, long long* lds_out) {
    return for_each_xcorr([&](auto v) {
        using V = decltype(v);
        if (!(V::key() == XcKey{L, stage})) return false;
        using Cfg = typename CfgFor<V::L>::Cfg;
        const size_t lds = xc_lds_bytes<Cfg>(V::STAGE);
        if (threads) *threads = XcGroup<Cfg>::THREADS;
        if (lds_out) *lds_out = (long long)lds;
        xc_run_grid(xc_blocks<Cfg>(a, V::STAGE), XcGroup<Cfg>::THREADS, lds, [&](int tid, long long b, unsigned char* l, EmuSync& s) {
            cx<float>* lds_c = reinterpret_cast<cx<float>*>(l);
            if constexpr (V::STAGE == XC_ROW) xc_row_body<Cfg>(a, tid, b, lds_c, s);
            else if constexpr (V::STAGE == XC_COL) xc_col_body<Cfg>(a, tid, b, lds_c, s);
            else xc_inv_body<Cfg>(a, tid, b, lds_c, s);
        });
        return true;
    });
}

}  // namespace

extern "C" {
// the smallest served length >= n, 0: none (kernel_variants.hpp select_xcorr)
int emu_xcorr_length(long long n) { return select_xcorr(n); }

// dtypes: 0 f32, 1 f64.  a / b: host arrays, offsets in elements.  peaks_out [pairs][7]; surface_out NULL or [pairs][W][W] float;
// c_out NULL or [pairs][W][W] double = C(d) as PEAK forms it (corr 2^ka 2^kb); stats_out NULL or [pairs][4]; geom_out NULL or 8 ints:
// Ly, Lx, threads and LDS bytes of ROW, COL, INV.  The caller has checked the arguments as rl_register_xcorr does.
int emu_register_xcorr(const void* a, int a_dtype, const long long* a_off, const void* b, int b_dtype, const long long* b_off, int pairs,
                       int ny, int nx, int R, double* peaks_out, float* surface_out, double* c_out, double* stats_out, int* geom_out) {
    if (pairs < 1 || ny < 1 || nx < 1 || R < 1 || R > (ny < nx ? ny : nx) / 2) return -1;
    const int Ly = select_xcorr((long long)ny + R), Lx = select_xcorr((long long)nx + R);
    if (!Ly || !Lx) return -1;
    const size_t W = 2 * (size_t)R + 1;
    const std::vector<cx<float>> twy = xc_twiddles(Ly), twx = xc_twiddles(Lx);
    std::vector<double> stats((size_t)pairs * 4, NAN);
    std::vector<cx<float>> spec((size_t)pairs * ny * Lx), rows((size_t)pairs * W * Lx);
    std::vector<float> corr((size_t)pairs * W * W);
    std::memset(spec.data(), 0xff, spec.size() * sizeof(cx<float>));
    std::memset(rows.data(), 0xff, rows.size() * sizeof(cx<float>));
    std::memset(corr.data(), 0xff, corr.size() * sizeof(float));
    XcArgs p;
    p.a = a; p.b = b; p.a_f64 = a_dtype; p.b_f64 = b_dtype; p.a_off = a_off; p.b_off = b_off;
    p.pairs = pairs; p.ny = ny; p.nx = nx; p.R = R; p.Ly = Ly; p.Lx = Lx;
    p.stats = stats.data(); p.spec = spec.data(); p.rows = rows.data(); p.corr = corr.data(); p.peaks = peaks_out; p.surf = surface_out;
    p.tw_y = twy.data(); p.tw_x = twx.data();
    xc_run_grid(2LL * pairs, kXcThreads, kXcThreads * sizeof(double),
                [&](int tid, long long blk, unsigned char* l, EmuSync& s) { xc_stats_body(p, tid, blk, reinterpret_cast<double*>(l), s); });
    int th[3] = {0, 0, 0};
    long long lds[3] = {0, 0, 0};
    if (!run_stage(Lx, XC_ROW, p, &th[0], &lds[0]) || !run_stage(Ly, XC_COL, p, &th[1], &lds[1]) || !run_stage(Lx, XC_INV, p, &th[2], &lds[2])) return -1;
    xc_run_grid(pairs, kXcThreads, xc_peak_lds_bytes(R),
                [&](int tid, long long blk, unsigned char* l, EmuSync& s) { xc_peak_body(p, tid, blk, reinterpret_cast<double*>(l), s); });
    if (geom_out) {
        geom_out[0] = Ly; geom_out[1] = Lx;
        for (int k = 0; k < 3; ++k) {
            geom_out[2 + 2 * k] = th[k];
            geom_out[3 + 2 * k] = (int)lds[k];
        }
    }
    if (stats_out) std::memcpy(stats_out, stats.data(), stats.size() * sizeof(double));
    if (c_out)
        for (int i = 0; i < pairs; ++i) {
            const double ka = xc_pow2(xc_norm_exp(stats[(size_t)i * 4 + 2])), kb = xc_pow2(xc_norm_exp(stats[(size_t)i * 4 + 3]));
            for (size_t k = 0; k < W * W; ++k) c_out[(size_t)i * W * W + k] = (double)corr[(size_t)i * W * W + k] * ka * kb;
        }
    return 0;
}

// PEAK alone on a given window: corr [W][W] float, stats [4] (means, E_a, E_b) -> peaks_out [7], surface_out NULL or [W][W]
int emu_xcorr_peak(const float* corr, const double* stats, int ny, int nx, int R, double* peaks_out, float* surface_out) {
    XcArgs p = {};
    p.pairs = 1; p.ny = ny; p.nx = nx; p.R = R;
    p.stats = const_cast<double*>(stats); p.corr = const_cast<float*>(corr); p.peaks = peaks_out; p.surf = surface_out;
    xc_run_grid(1, kXcThreads, xc_peak_lds_bytes(R),
                [&](int tid, long long blk, unsigned char* l, EmuSync& s) { xc_peak_body(p, tid, blk, reinterpret_cast<double*>(l), s); });
    return 0;
}
}

#ifdef XCORR_EMU_MAIN
// The stand-alone program of the sanitizer run: the images and the outputs are heap blocks of EXACTLY their byte counts (the last
// pair's images end with their buffers, at odd element offsets), and the "LDS" blocks are exactly the launches' sizes, so a read or
// a write past any of them is the sanitizer's to find.  Results are held to plain loops written here.  Prints "ok <cases>".
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
int xcorr_case(int ny, int nx, int R, long* done) {
    const int pairs = 3, W = 2 * R + 1;
    const size_t n = (size_t)ny * nx;
    Exact<TA> a(2 * n + 1);
    Exact<TB> b((size_t)pairs * n + 3);
    for (size_t i = 0; i < a.n; ++i) a.p[i] = (TA)(next_unit() * 100.0);
    for (size_t i = 0; i < b.n; ++i) b.p[i] = (TB)(next_unit() * 100.0);
    const long long a_off[3] = {1, (long long)n + 1, 1}, b_off[3] = {2LL * (long long)n + 3, 3, (long long)n + 3};
    // pair 0's moving image: its reference displaced by (R, -R + 1), so that there is a peak to find
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const int ys = y - R, xs = x + R - 1;
            if (ys >= 0 && ys < ny && xs >= 0 && xs < nx) b.p[b_off[0] + (size_t)y * nx + x] = (TB)a.p[a_off[0] + (size_t)ys * nx + xs];
        }
    Exact<double> peaks((size_t)pairs * 7), c((size_t)pairs * W * W);
    Exact<float> surf((size_t)pairs * W * W);
    if (emu_register_xcorr(a.p, sizeof(TA) == 4 ? 0 : 1, a_off, b.p, sizeof(TB) == 4 ? 0 : 1, b_off, pairs, ny, nx, R, peaks.p, surf.p, c.p, nullptr, nullptr))
        return 1;
    for (int i = 0; i < pairs; ++i) {
        long double ma = 0, mb = 0, ea = 0, eb = 0;
        for (size_t k = 0; k < n; ++k) { ma += a.p[a_off[i] + k]; mb += b.p[b_off[i] + k]; }
        ma /= n; mb /= n;
        for (size_t k = 0; k < n; ++k) {
            const long double u = a.p[a_off[i] + k] - ma, v = b.p[b_off[i] + k] - mb;
            ea += u * u; eb += v * v;
        }
        const long double tol = 1e-4L * sqrtl(ea * eb);
        for (int dy = -R; dy <= R; ++dy)
            for (int dx = -R; dx <= R; ++dx) {
                long double s = 0;
                for (int y = 0; y < ny; ++y)
                    for (int x = 0; x < nx; ++x)
                        if (y + dy >= 0 && y + dy < ny && x + dx >= 0 && x + dx < nx)
                            s += (a.p[a_off[i] + (size_t)y * nx + x] - ma) * (b.p[b_off[i] + (size_t)(y + dy) * nx + x + dx] - mb);
                const double got = c.p[((size_t)i * W + dy + R) * W + dx + R];
                if (!(fabsl(got - s) <= tol)) {
                    std::printf("xcorr %d x %d R %d pair %d d (%d, %d): %.9g, want %.9Lg\n", ny, nx, R, i, dy, dx, got, s);
                    return 1;
                }
            }
    }
    if (peaks.p[0] != (double)R || peaks.p[1] != (double)(-R + 1)) {
        std::printf("xcorr %d x %d R %d: peak (%g, %g)\n", ny, nx, R, peaks.p[0], peaks.p[1]);
        return 1;
    }
    ++*done;
    return 0;
}
}  // namespace

int main() {
    long done = 0;
    const int cases[][3] = {{24, 40, 8}, {56, 48, 8}, {37, 51, 6}};
    for (const auto& c : cases)
        if (xcorr_case<float, float>(c[0], c[1], c[2], &done) || xcorr_case<double, float>(c[0], c[1], c[2], &done) ||
            xcorr_case<float, double>(c[0], c[1], c[2], &done) || xcorr_case<double, double>(c[0], c[1], c[2], &done))
            return 1;
    // the 16-lane geometry, 256, the wave-private length with cross-lane tails and the workgroup-synchronous one, on thin images
    if (xcorr_case<float, double>(100, 20, 10, &done) || xcorr_case<double, float>(20, 200, 9, &done) ||
        xcorr_case<double, double>(20, 560, 10, &done) || xcorr_case<float, float>(570, 20, 10, &done))
        return 1;
    std::printf("ok %ld\n", done);
    return 0;
}
#endif
