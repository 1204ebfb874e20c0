// Host emulator of the divergence and stopping-rule kernels (rescan_line_sted_amd/csrc/stop_kernels.hpp): the very same thread
// bodies, run thread by thread and workgroup by workgroup; the workgroup tree runs step by step as the device runs it between
// barriers, and every workgroup of a LATCH launch decides for itself, as on the device.  TEST INFRASTRUCTURE ONLY -- built by
// tests/test_stop_cpu.py with g++ (-ffp-contract=off) and never loaded by the product.
#include <vector>

#include "../../rescan_line_sted_amd/csrc/stop_kernels.hpp"

using namespace rl;

namespace {

template <typename T>
void divergence(const T* meas, const T* pred, double* part, size_t n, int frames) {
    DivParams<T> p{};
    p.meas = meas; p.pred = pred; p.part = part; p.n = n;
    p.nb = stop_blocks(n, sizeof(T));
    std::vector<double> s(kStopThreads);
    for (int f = 0; f < frames; ++f)
        for (int b = 0; b < p.nb; ++b) {
            for (int t = 0; t < kStopThreads; ++t) s[t] = stop_divergence_thread<T>(p, f, b, t);
            for (int h = kStopThreads / 2; h > 0; h >>= 1)
                for (int t = 0; t < kStopThreads; ++t) accel_tree_step(s.data(), t, h);
            part[(size_t)f * p.nb + b] = s[0];
        }
}

// returns the number of workgroups whose decision differed from workgroup 0's (0 on a correct kernel)
template <typename T>
int latch(const T* est, T* result, const double* part, const StopFrame* prev, StopFrame* next, size_t n_img, size_t n_frame, int frames,
          int rule, double threshold, int done, int have_prev) {
    LatchParams<T> p{};
    p.est = est; p.result = result; p.part = part; p.prev = prev; p.next = next; p.n = n_img;
    p.nb = accel_blocks(n_img, sizeof(T));
    p.nb_part = stop_blocks(n_frame, sizeof(T));
    p.rule = rule; p.have_prev = have_prev; p.done = done; p.threshold = threshold; p.count = (double)n_frame;
    int differ = 0;
    for (int f = 0; f < frames; ++f) {
        bool copy0 = false;
        for (int b = 0; b < p.nb; ++b) {
            bool copy;
            const StopFrame s = stop_latch_frame<T>(p, f, stop_total(part + (size_t)f * p.nb_part, p.nb_part), &copy);
            if (b == 0) {
                next[f] = s;
                copy0 = copy;
            } else if (copy != copy0) {
                ++differ;
            }
            if (copy)
                for (int t = 0; t < kStopThreads; ++t) stop_copy_thread<T>(p, f, b, t);
        }
    }
    return differ;
}

}  // namespace

extern "C" {
int emu_stop_blocks(size_t n, size_t esize) { return stop_blocks(n, esize); }
int emu_stop_threads() { return kStopThreads; }
int emu_stop_state_bytes() { return (int)sizeof(StopFrame); }
double emu_stop_term(double m, double p) { return stop_term(m, p); }
double emu_stop_total(const double* part, int nb) { return stop_total(part, nb); }
int emu_stop_rule_met(int rule, double threshold, double count, double d, int have_prev, double d_prev) {
    return stop_rule_met(rule, threshold, count, d, have_prev != 0, d_prev) ? 1 : 0;
}
void emu_stop_divergence_f64(const double* meas, const double* pred, double* part, size_t n, int frames) {
    divergence<double>(meas, pred, part, n, frames);
}
void emu_stop_divergence_f32(const float* meas, const float* pred, double* part, size_t n, int frames) {
    divergence<float>(meas, pred, part, n, frames);
}
int emu_stop_latch_f64(const double* est, double* result, const double* part, const void* prev, void* next, size_t n_img, size_t n_frame,
                       int frames, int rule, double threshold, int done, int have_prev) {
    return latch<double>(est, result, part, (const StopFrame*)prev, (StopFrame*)next, n_img, n_frame, frames, rule, threshold, done, have_prev);
}
int emu_stop_latch_f32(const float* est, float* result, const double* part, const void* prev, void* next, size_t n_img, size_t n_frame,
                       int frames, int rule, double threshold, int done, int have_prev) {
    return latch<float>(est, result, part, (const StopFrame*)prev, (StopFrame*)next, n_img, n_frame, frames, rule, threshold, done, have_prev);
}
}
