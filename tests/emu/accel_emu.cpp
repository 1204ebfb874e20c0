// Host emulator of the Biggs-Andrews kernels (rescan_line_sted_amd/csrc/accel_kernels.hpp): the very same thread bodies, run
// thread by thread and workgroup by workgroup.  The threads of a launch touch disjoint elements and meet only in the workgroup
// tree, which runs here step by step as the device runs it between barriers.  TEST INFRASTRUCTURE ONLY -- built by
// tests/test_accel_cpu.py with g++ (-ffp-contract=off) and never loaded by the product.
#include <vector>

#include "../../rescan_line_sted_amd/csrc/accel_kernels.hpp"

using namespace rl;

namespace {

template <typename T>
void reduce(T* est, T* y, T* g, double* part, size_t n, int frames, int flags) {
    AccelParams<T> p{};
    p.est = est; p.y = y; p.g = g; p.part = part; p.n = n; p.flags = flags;
    p.nb = accel_blocks(n, sizeof(T));
    std::vector<double> sn(kAccelThreads), sd(kAccelThreads);
    for (int f = 0; f < frames; ++f)
        for (int b = 0; b < p.nb; ++b) {
            for (int t = 0; t < kAccelThreads; ++t) accel_reduce_thread<T>(p, f, b, t, sn[t], sd[t]);
            double* out = part + ((size_t)f * p.nb + b) * 2;
            if (!(flags & ACC_HAVE_PREV)) {
                out[0] = out[1] = 0.0;
                continue;
            }
            for (int h = kAccelThreads / 2; h > 0; h >>= 1)
                for (int t = 0; t < kAccelThreads; ++t) {
                    accel_tree_step(sn.data(), t, h);
                    accel_tree_step(sd.data(), t, h);
                }
            out[0] = sn[0];
            out[1] = sd[0];
        }
}

template <typename T>
void extrapolate(T* est, T* y, T* x, const double* part, double* alpha, size_t n, int frames, int flags) {
    AccelParams<T> p{};
    p.est = est; p.y = y; p.x = x; p.n = n; p.flags = flags;
    p.nb = accel_blocks(n, sizeof(T));
    for (int f = 0; f < frames; ++f) {
        const double a = (flags & ACC_FRESH) ? 0.0 : accel_alpha(part + (size_t)f * p.nb * 2, p.nb);
        alpha[f] = a;
        for (int b = 0; b < p.nb; ++b)
            for (int t = 0; t < kAccelThreads; ++t) accel_extrapolate_thread<T>(p, f, b, t, a);
    }
}

}  // namespace

extern "C" {
int emu_accel_blocks(size_t n, size_t esize) { return accel_blocks(n, esize); }
int emu_accel_threads() { return kAccelThreads; }
double emu_accel_alpha(const double* part, int nb) { return accel_alpha(part, nb); }
void emu_accel_reduce_f64(double* est, double* y, double* g, double* part, size_t n, int frames, int flags) {
    reduce<double>(est, y, g, part, n, frames, flags);
}
void emu_accel_reduce_f32(float* est, float* y, float* g, double* part, size_t n, int frames, int flags) {
    reduce<float>(est, y, g, part, n, frames, flags);
}
void emu_accel_extrapolate_f64(double* est, double* y, double* x, const double* part, double* alpha, size_t n, int frames, int flags) {
    extrapolate<double>(est, y, x, part, alpha, n, frames, flags);
}
void emu_accel_extrapolate_f32(float* est, float* y, float* x, const double* part, double* alpha, size_t n, int frames, int flags) {
    extrapolate<float>(est, y, x, part, alpha, n, frames, flags);
}
}
