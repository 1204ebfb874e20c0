// Shared by the host emulators (emu.cpp, long_emu.cpp, long_outer_emu.cpp): the stand-ins for the GPU's execution model.  One OS thread per
// GPU thread, a pthread barrier for __syncthreads(), a per-wavefront barrier and exchange array for the cross-lane
// operations, LDS poisoned with NaN bit patterns before every workgroup.  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <pthread.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/kernel_variants.hpp"
#include "../../rescan_line_sted_amd/csrc/outer_lds.hpp"

using namespace rl;

struct EmuSync {
    pthread_barrier_t* bar;        // whole workgroup
    pthread_barrier_t* wave_bar;   // the 64 threads of this thread's wavefront
    double* xchg;                  // 64 slots shared by the wavefront (cross-lane shuffles)
    int lane;
    void wg() const { pthread_barrier_wait(bar); }
    void wave() const { pthread_barrier_wait(wave_bar); }
    template <int MASK>
    double shfl_xor(double v) const {
        xchg[lane] = v;
        pthread_barrier_wait(wave_bar);
        const double o = xchg[lane ^ MASK];
        pthread_barrier_wait(wave_bar);
        return o;
    }
    template <int MASK>
    float shfl_xor(float v) const { return (float)shfl_xor<MASK>((double)v); }
    // radix-2 exchange stage (DevSync::bfly): MASK bit clear -> x + partner, set -> partner - x
    template <int MASK, typename T>
    void bfly(cx<T>& x, int l) const {
        const T pr = shfl_xor<MASK>(x.re), pi = shfl_xor<MASK>(x.im);
        if (l & MASK) x = mk<T>(pr - x.re, pi - x.im);
        else x = mk<T>(x.re + pr, x.im + pi);
    }
};

template <class Body>
static void run_grid(int gx, int gy, int nthreads, size_t lds_bytes, Body body) {
    std::vector<unsigned char> lds(lds_bytes + 64);
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, nthreads);
    const int nwaves = (nthreads + 63) / 64;
    std::vector<pthread_barrier_t> wbar(nwaves);
    std::vector<double> xchg((size_t)nwaves * 64);
    for (int w = 0; w < nwaves; ++w) {
        const int n = (w + 1) * 64 <= nthreads ? 64 : nthreads - w * 64;
        pthread_barrier_init(&wbar[w], nullptr, n);
    }
    for (int by = 0; by < gy; ++by)
        for (int bx = 0; bx < gx; ++bx) {
            std::memset(lds.data(), 0xff, lds.size());   // poison: NaNs if read before written
            std::vector<std::thread> th;
            th.reserve(nthreads);
            for (int tid = 0; tid < nthreads; ++tid)
                th.emplace_back([&, tid]() {
                    EmuSync s{&bar, &wbar[tid / 64], &xchg[(size_t)(tid / 64) * 64], tid % 64};
                    body(tid, bx, by, lds.data(), s);
                });
            for (auto& t : th) t.join();
        }
    pthread_barrier_destroy(&bar);
    for (auto& b : wbar) pthread_barrier_destroy(&b);
}

template <class Cfg, typename T>
static std::vector<cx<T>> twiddles_of() {   // the per-pass table the device plan uploads for one geometry
    constexpr int n = PassTw<Cfg, false, 0>::TOTAL;
    std::vector<double> h(2 * (size_t)(n > 0 ? n : 1), 0.0);
    if (n > 0) fill_pass_twiddles<Cfg>(h.data());
    std::vector<cx<T>> tw(n > 0 ? n : 1);
    for (size_t i = 0; i < tw.size(); ++i) tw[i] = mk<T>((T)h[2 * i], (T)h[2 * i + 1]);
    return tw;
}

// ---- the variants of kernel_variants.hpp on the host: what the kernel of a row runs (the bodies fft_kernels.hip's k_colconv,
// k_colconv_outer and k_rowpass call for the same template arguments), and a row as a line of text
template <int L, int C, class V, typename T>
static void colconv_variant(V, const ColParams<T>& p, int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
    using KCfg = typename ColCfgFor<L>::type;
    if constexpr (WavePrivate<KCfg>::value) colconv_wave_body<KCfg, C, V::MODE, T, V::REALP, V::NYC, V::CT>(p, tid, bx, by, reinterpret_cast<cx<T>*>(lds), s);
    else colconv_body<KCfg, C, T>(p, tid, bx, by, reinterpret_cast<cx<T>*>(lds), s);
}
template <int L, class V, typename T>
static void outer_variant(V, const ColParams<T>& p, int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
    using OC = OuterCol<L>;
    static_assert(sizeof(T) == 4 || V::MODE == COL_PER_IMAGE, "float64: the whole pass only");
    if constexpr (sizeof(T) == 4)
        colconv_outer_body<typename OC::Core, OC::M, V::C, float, V::REALP, V::MODE, (V::MODE == COL_PER_IMAGE ? OC::PARK : 0),
                           (V::MODE == COL_PER_IMAGE ? OC::TWLDS : OC::TWLDS_SPLIT), V::NYC>(p, tid, bx, by, reinterpret_cast<cx<float>*>(lds), s);
    else
        colconv_outer_body<typename OC::Core, OC::M, V::C, double, V::REALP, COL_PER_IMAGE, OC::PARK64, 0, V::NYC>(p, tid, bx, by, reinterpret_cast<cx<double>*>(lds), s);
}
template <int L, int Q, class V, typename T>
static void rowpass_variant(V, const RowParams<T>& p, int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
    using KCfg = typename CfgFor<L>::Cfg;
    if constexpr (kRowLean<KCfg, V::MODE, V::ONEV, V::PRESUM>) rowlean_body<KCfg, Q, V::MODE, T, V::NXC, V::SUBC>(p, tid, bx, by, reinterpret_cast<cx<T>*>(lds), s);
    else rowpass_body<KCfg, Q, V::MODE, V::ONEV, T, V::PRESUM>(p, tid, bx, by, reinterpret_cast<cx<T>*>(lds), s);
}

template <typename T>
static const char* tname() { return sizeof(T) == 4 ? "f32" : "f64"; }
template <class... A>
static std::string fmt_line(const char* f, A... a) {
    char buf[160];
    std::snprintf(buf, sizeof buf, f, a...);
    return buf;
}
template <int L, typename T>
static std::string line_of(const ColKey& k) { return fmt_line("k_colconv L=%d T=%s MODE=%d REALP=%d NYC=%d CT=%d\n", L, tname<T>(), k.mode, k.realp, k.nyc, k.ct); }
template <int L, typename T>
static std::string line_of(const OuterKey& k) { return fmt_line("k_colconv_outer L=%d C=%d REALP=%d MODE=%d T=%s NYC=%d\n", L, k.c, k.realp, k.mode, tname<T>(), k.nyc); }
template <int L, typename T>
static std::string line_of(const RowKey& k) { return fmt_line("k_rowpass L=%d T=%s MODE=%d ONEV=%d PRESUM=%d NXC=%d SUBC=%d\n", L, tname<T>(), k.mode, k.onev, k.presum, k.nxc, k.subc); }
template <int L, typename T>
static std::string line_of(const PairKey& k) { return fmt_line("k_rowpair L=%d T=%s MODE=%d NXC=%d SUBC=%d\n", L, tname<T>(), k.mode, k.nxc, k.subc); }
// every row that exists for (L, T, Special), one per line.  The column family is the one launch_col takes for the type.
template <int L, typename T, class Special>
static void list_variants(std::string& out, bool col, bool row) {
    if (col && !kOuterCol<L, T>) for_each_colconv<L, Special>([&](auto v) { out += line_of<L, T>(v.key()); return false; });
    if (col) for_each_outer<L, T, Special>([&](auto v) { out += line_of<L, T>(v.key()); return false; });
    if (row) for_each_rowpass<L, Special>([&](auto v) { out += line_of<L, T>(v.key()); return false; });
    if (row) for_each_rowpair<L, Special>([&](auto v) { out += line_of<L, T>(v.key()); return false; });
}
static int copy_out(const std::string& s, char* buf, int cap) {   // returns the length of the text (truncated to cap - 1)
    std::snprintf(buf, (size_t)cap, "%s", s.c_str());
    return (int)s.size();
}
