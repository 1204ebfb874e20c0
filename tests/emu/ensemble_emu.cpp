// Host emulator of the ensemble statistics (rescan_line_sted_amd/csrc/ensemble_kernels.hpp, ensemble_kernels.hip): the very same
// thread bodies, run thread by thread and workgroup by workgroup over the launch grid; the workgroup tree runs step by step as the
// device runs it between barriers.  TEST INFRASTRUCTURE ONLY -- built by tests/test_ensemble_cpu.py with g++ (-ffp-contract=off),
// as a shared library and, with -DENSEMBLE_EMU_MAIN, as a stand-alone program for the sanitizers; never loaded by the product.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/ensemble_kernels.hpp"

using namespace rl;

namespace {

// k_ensemble_stats on grid (nb, groups), then k_ensemble_totals
template <typename T, typename TT>
int stats(const T* src, const int64_t* member_off, const int32_t* group_ptr, int groups, const TT* truth, const int64_t* truth_off,
          const double* truth_scale, size_t n, double* mean, double* var, double* out) {
    EnsembleParams<T, TT> p{};
    p.src = src; p.member_off = member_off; p.group_ptr = group_ptr; p.truth = truth; p.truth_off = truth_off;
    p.truth_scale = truth_scale; p.mean = mean; p.var = var; p.n = n;
    p.nb = ensemble_blocks(n, sizeof(T));
    std::vector<double> part((size_t)groups * p.nb * kEnsembleSums, -1.0);
    p.part = part.data();
    std::vector<double> slots((size_t)kEnsembleSums * kEnsembleThreads);
    double (*s)[kEnsembleThreads] = reinterpret_cast<double (*)[kEnsembleThreads]>(slots.data());
    for (int g = 0; g < groups; ++g)
        for (int b = 0; b < p.nb; ++b) {
            for (int t = 0; t < kEnsembleThreads; ++t) {
                double v[kEnsembleSums];
                ensemble_thread<T, TT>(p, g, b, t, v);
                for (int c = 0; c < kEnsembleSums; ++c) s[c][t] = v[c];
            }
            for (int h = kEnsembleThreads / 2; h > 0; h >>= 1)
                for (int t = 0; t < kEnsembleThreads; ++t) ensemble_tree_step(s, t, h);
            ensemble_write_part(p.part, p.nb, g, b, s);
        }
    for (int g = 0; g < groups; ++g) ensemble_total(p.part, group_ptr, p.nb, g, out);
    return p.nb;
}

}  // namespace

extern "C" {
int emu_ensemble_threads() { return kEnsembleThreads; }
int emu_ensemble_sums() { return kEnsembleSums; }
int emu_ensemble_blocks(size_t n, size_t esize) { return ensemble_blocks(n, esize); }
// src / truth: element type by dtype (0 f32, 1 f64); truth may be NULL, truth_scale may not when truth is set; mean / var [groups][n]
// or NULL; out [groups][6].  Returns the workgroups per group.
int emu_ensemble_stats(const void* src, int src_dtype, const int64_t* member_off, const int32_t* group_ptr, int groups,
                       const void* truth, int truth_dtype, const int64_t* truth_off, const double* truth_scale, size_t n,
                       double* mean, double* var, double* out) {
    const bool tf = truth && truth_dtype == 0;
    if (src_dtype == 0)
        return tf ? stats((const float*)src, member_off, group_ptr, groups, (const float*)truth, truth_off, truth_scale, n, mean, var, out)
                  : stats((const float*)src, member_off, group_ptr, groups, (const double*)truth, truth_off, truth_scale, n, mean, var, out);
    return tf ? stats((const double*)src, member_off, group_ptr, groups, (const float*)truth, truth_off, truth_scale, n, mean, var, out)
              : stats((const double*)src, member_off, group_ptr, groups, (const double*)truth, truth_off, truth_scale, n, mean, var, out);
}
}

#ifdef ENSEMBLE_EMU_MAIN
// The stand-alone program of the sanitizer run: groups of different sizes at odd offsets, exactly-sized buffers (a read or a write
// past an image is the sanitizer's to find), f32 and f64 sources and truths, with and without maps and truth; the sums are held to
// a plain double loop loosely.  Prints "ok <calls> <groups>" and returns 0, or says what failed.
template <typename T, typename TT>
int run_case(size_t n, int shift, long* groups_done) {
    unsigned state = 777u + (unsigned)n;
    auto next = [&state]() {
        state = state * 1664525u + 1013904223u;
        return (double)(state >> 20) / 4096.0;
    };
    const int sizes[] = {1, 2, 3, 16, 17};
    const int G = 5;
    std::vector<int64_t> off;
    std::vector<int32_t> gp(1, 0);
    size_t images = 0;
    for (int g = 0; g < G; ++g) {
        for (int m = 0; m < sizes[g]; ++m) off.push_back((int64_t)(shift + (images + m) * n));
        images += sizes[g];
        gp.push_back((int32_t)off.size());
    }
    off[5] = off[0];   // a member listed in two groups
    std::vector<T> src(shift + images * n);
    for (auto& x : src) x = (T)next();
    std::vector<TT> truth(shift + G * n);
    for (auto& x : truth) x = (TT)next();
    std::vector<int64_t> toff(G);
    std::vector<double> scale(G);
    for (int g = 0; g < G; ++g) {
        toff[g] = (int64_t)(shift + g * n);
        scale[g] = 0.5 + 0.25 * g;
    }
    for (int variant = 0; variant < 3; ++variant) {   // 0: truth and maps, 1: no truth, 2: no maps
        std::vector<double> mean(G * n, -1.0), var(G * n, -1.0), out((size_t)G * kEnsembleFields, -1.0);
        emu_ensemble_stats(src.data(), sizeof(T) == 4 ? 0 : 1, off.data(), gp.data(), G, variant == 1 ? nullptr : truth.data(),
                           sizeof(TT) == 4 ? 0 : 1, toff.data(), scale.data(), n, variant == 2 ? nullptr : mean.data(),
                           variant == 2 ? nullptr : var.data(), out.data());
        for (int g = 0; g < G; ++g) {
            const int cnt = gp[g + 1] - gp[g];
            double sm = 0.0, sv = 0.0, sb = 0.0, se = 0.0;
            for (size_t i = 0; i < n; ++i) {
                double m = 0.0, ss = 0.0, e2 = 0.0;
                for (int k = gp[g]; k < gp[g + 1]; ++k) m += (double)src[off[k] + i];
                m /= cnt;
                const double st = variant == 1 ? 0.0 : scale[g] * (double)truth[toff[g] + i];
                for (int k = gp[g]; k < gp[g + 1]; ++k) {
                    ss += ((double)src[off[k] + i] - m) * ((double)src[off[k] + i] - m);
                    e2 += ((double)src[off[k] + i] - st) * ((double)src[off[k] + i] - st);
                }
                const double v = cnt > 1 ? ss / (cnt - 1) : 0.0;
                if (variant != 2 && (std::fabs(mean[g * n + i] - m) > 1e-12 * (1.0 + std::fabs(m)) || std::fabs(var[g * n + i] - v) > 1e-9 * (1.0 + v))) {
                    std::printf("n %zu group %d pixel %zu: maps %.17g %.17g, want %.17g %.17g\n", n, g, i, mean[g * n + i], var[g * n + i], m, v);
                    return 1;
                }
                sm += m;
                sv += v;
                if (variant != 1) {
                    sb += (m - st) * (m - st);
                    se += e2 / cnt;
                }
            }
            const double* o = &out[(size_t)g * kEnsembleFields];
            const double want[5] = {(double)cnt, sm, sv, sb, se};
            for (int f = 0; f < 5; ++f)
                if (!(std::fabs(o[f] - want[f]) <= 1e-9 * (1.0 + std::fabs(want[f])))) {
                    std::printf("n %zu variant %d group %d field %d: %.17g, want %.17g\n", n, variant, g, f, o[f], want[f]);
                    return 1;
                }
            if (cnt == 1 && o[2] != 0.0) {
                std::printf("n %zu group %d: variance of one member %.17g\n", n, g, o[2]);
                return 1;
            }
            ++*groups_done;
        }
    }
    return 0;
}

int main() {
    const size_t ns[] = {1, 3, 5, 1023, 8193, 8197};
    long calls = 0, groups = 0;
    for (size_t n : ns)
        for (int shift = 0; shift < 2; ++shift) {
            if (run_case<float, double>(n, shift, &groups) || run_case<double, double>(n, shift, &groups) ||
                run_case<float, float>(n, 2 * shift + 1, &groups) || run_case<double, float>(n, shift, &groups))
                return 1;
            calls += 12;
        }
    std::printf("ok %ld %ld\n", calls, groups);
    return 0;
}
#endif
