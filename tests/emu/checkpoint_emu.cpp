// Host emulator of the iteration checkpoints (rescan_line_sted_amd/csrc/checkpoint_kernels.hpp, checkpoint_kernels.hip): the very
// same thread bodies, run thread by thread and workgroup by workgroup over the launch grid; the workgroup tree runs step by step as
// the device runs it between barriers.  TEST INFRASTRUCTURE ONLY -- built by tests/test_checkpoint_cpu.py with g++
// (-ffp-contract=off), as a shared library and, with -DCHECKPOINT_EMU_MAIN, as a stand-alone program for the sanitizers; never
// loaded by the product.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/checkpoint_kernels.hpp"

using namespace rl;

namespace {

// k_checkpoint on grid (nb, frames), then k_checkpoint_totals where a trace is asked for
template <typename T, typename TO>
int take(const T* est, const T* obj, TO* dst, size_t n, int frames, double* part, double* out) {
    CheckpointParams<T, TO> p{};
    p.est = est; p.obj = obj; p.dst = dst; p.part = part; p.n = n;
    p.nb = checkpoint_blocks(n, sizeof(T));
    std::vector<double> slots((size_t)kCheckpointFields * kCheckpointThreads);
    double (*s)[kCheckpointThreads] = reinterpret_cast<double (*)[kCheckpointThreads]>(slots.data());
    for (int f = 0; f < frames; ++f)
        for (int b = 0; b < p.nb; ++b) {
            for (int t = 0; t < kCheckpointThreads; ++t) {
                double v[kCheckpointFields];
                checkpoint_thread<T, TO>(p, f, b, t, v);
                for (int c = 0; c < kCheckpointFields; ++c) s[c][t] = v[c];
            }
            if (!part) continue;
            for (int h = kCheckpointThreads / 2; h > 0; h >>= 1)
                for (int t = 0; t < kCheckpointThreads; ++t) checkpoint_tree_step(s, t, h);
            checkpoint_write_part(part, p.nb, f, b, s);
        }
    if (part && out)
        for (int f = 0; f < frames; ++f) checkpoint_total(part, p.nb, f, out);
    return p.nb;
}

}  // namespace

extern "C" {
int emu_checkpoint_threads() { return kCheckpointThreads; }
int emu_checkpoint_fields() { return kCheckpointFields; }
int emu_checkpoint_blocks(size_t n, size_t esize) { return checkpoint_blocks(n, esize); }
// est / obj [frames][n] of dtype (0 f32, 1 f64); dst [frames][n] of out_dtype or NULL; part [frames][nb][6] or NULL (no sums: obj is
// not read, out is not written); out [frames][6].  Returns the workgroups per frame.
int emu_checkpoint(const void* est, const void* obj, int dtype, void* dst, int out_dtype, size_t n, int frames, double* part,
                   double* out) {
    const bool of = dst ? out_dtype == 0 : dtype == 0;
    if (dtype == 0)
        return of ? take((const float*)est, (const float*)obj, (float*)dst, n, frames, part, out)
                  : take((const float*)est, (const float*)obj, (double*)dst, n, frames, part, out);
    return of ? take((const double*)est, (const double*)obj, (float*)dst, n, frames, part, out)
              : take((const double*)est, (const double*)obj, (double*)dst, n, frames, part, out);
}
}

#ifdef CHECKPOINT_EMU_MAIN
// The stand-alone program of the sanitizer run: three frames at odd and even element offsets in exactly-sized buffers (a read or a
// write past a frame is the sanitizer's to find), every pair of source and destination type, with and without destination and
// trace; the sums are held to a plain double loop loosely, the cast to the plain cast exactly.  Prints "ok <calls>" and returns 0,
// or says what failed.
template <typename T, typename TO>
int run_case(size_t n, int shift, long* calls) {
    unsigned state = 4242u + (unsigned)n;
    auto next = [&state]() {
        state = state * 1664525u + 1013904223u;
        return (double)(state >> 20) / 4096.0;
    };
    const int F = 3;
    std::vector<T> est(shift + F * n), obj(shift + F * n);
    for (auto& x : est) x = (T)next();
    for (auto& x : obj) x = (T)next();
    const int nb = checkpoint_blocks(n, sizeof(T));
    for (int variant = 0; variant < 3; ++variant) {   // 0: destination and trace, 1: trace only, 2: destination only
        std::vector<TO> dst(variant == 1 ? 0 : shift + F * n, (TO)-1);
        std::vector<double> part(variant == 2 ? 0 : (size_t)F * nb * kCheckpointFields, -1.0), out((size_t)F * kCheckpointFields, -1.0);
        emu_checkpoint(est.data() + shift, variant == 2 ? nullptr : obj.data() + shift, sizeof(T) == 4 ? 0 : 1,
                       variant == 1 ? nullptr : dst.data() + shift, sizeof(TO) == 4 ? 0 : 1, n, F, variant == 2 ? nullptr : part.data(),
                       out.data());
        ++*calls;
        for (int f = 0; f < F; ++f) {
            double want[6] = {0, 0, 0, 0, 0, 0};
            for (size_t i = 0; i < n; ++i) {
                const double x = (double)est[shift + f * n + i], t = (double)obj[shift + f * n + i];
                want[0] += x; want[1] += t; want[2] += x * x; want[3] += t * t; want[4] += x * t; want[5] += (x - t) * (x - t);
                if (variant != 1 && dst[shift + f * n + i] != (TO)est[shift + f * n + i]) {
                    std::printf("n %zu shift %d frame %d pixel %zu: cast %.17g, want %.17g\n", n, shift, f, i, (double)dst[shift + f * n + i],
                                (double)(TO)est[shift + f * n + i]);
                    return 1;
                }
            }
            for (int c = 0; c < 6; ++c) {
                const double got = out[(size_t)f * 6 + c];
                if (variant == 2 ? got != -1.0 : !(std::fabs(got - want[c]) <= 1e-9 * (1.0 + std::fabs(want[c])))) {
                    std::printf("n %zu shift %d variant %d frame %d field %d: %.17g, want %.17g\n", n, shift, variant, f, c, got, want[c]);
                    return 1;
                }
            }
        }
        for (int i = 0; i < shift && variant != 1; ++i)
            if (dst[i] != (TO)-1) {
                std::printf("n %zu shift %d: wrote in front of the destination\n", n, shift);
                return 1;
            }
    }
    return 0;
}

int main() {
    const size_t ns[] = {1, 3, 5, 1023, 8193, 8197};
    long calls = 0;
    for (size_t n : ns)
        for (int shift = 0; shift < 4; ++shift)
            if (run_case<float, float>(n, shift, &calls) || run_case<float, double>(n, shift, &calls) ||
                run_case<double, float>(n, shift, &calls) || run_case<double, double>(n, shift, &calls))
                return 1;
    std::printf("ok %ld\n", calls);
    return 0;
}
#endif
