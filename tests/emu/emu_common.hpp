// Shared by the host emulators (emu.cpp, long_emu.cpp, long_outer_emu.cpp): the stand-ins for the GPU's execution model.  One OS thread per
// GPU thread, a pthread barrier for __syncthreads(), a per-wavefront barrier and exchange array for the cross-lane
// operations, LDS poisoned with NaN bit patterns before every workgroup.  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <pthread.h>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/conv_kernels.hpp"
#include "../../rescan_line_sted_amd/csrc/fft_configs.hpp"

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
