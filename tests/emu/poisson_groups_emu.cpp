// Host emulation of the frame-group Poisson kernel (rescan_line_sted_amd/csrc/poisson_kernels.hpp poisson_groups_body: the text
// k_poisson_groups compiles) and a check of the sampler header's pieces (philox_poisson.hpp ptrs_rate / ptrs_slow / ptrs_candidate /
// ptrs_squeeze / ptrs_accept) against the sampler as it was before it was split.  TEST INFRASTRUCTURE ONLY; driven by
// tests/test_poisson_groups_cpu.py.
#include <atomic>

#include "emu_common.hpp"
#include "../../rescan_line_sted_amd/csrc/poisson_kernels.hpp"

// ---- the reference: philox_poisson_fast, philox_ptrs_attempt and philox_poisson word for word as they stood before the split
// (they use the generator, u53 and the polynomial functions of the header, which the split did not touch)
namespace before_split {

RL_HD bool philox_poisson_fast(double lam, uint64_t seed, uint32_t image, uint32_t pixel, double* out) {
    RL_FP_STRICT
    if (!(lam > 0.0)) {
        *out = 0.0;
        return true;
    }
    if (lam < 10.0) return false;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const double slam = __builtin_sqrt(lam);
    const double b = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * b;
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    const Philox4 o = philox4x32_10(pixel, image, 0u, 0x504F4953u, k0, k1);
    const double U = u53(o.x[0], o.x[1]) - 0.5;
    const double V = u53(o.x[2], o.x[3]);
    const double us = 0.5 - (U < 0.0 ? -U : U);
    const double k = __builtin_floor((2.0 * a / us + b) * U + lam + 0.43);
    *out = k;
    return us >= 0.07 && V <= vr;
}

RL_HD bool philox_ptrs_attempt(double lam, uint32_t k0, uint32_t k1, uint32_t image, uint32_t pixel, uint32_t blk, double* kout) {
    RL_FP_STRICT
    const double slam = __builtin_sqrt(lam);
    const double b = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * b;
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    const Philox4 o = philox4x32_10(pixel, image, blk, 0x504F4953u, k0, k1);
    const double U = u53(o.x[0], o.x[1]) - 0.5;
    const double V = u53(o.x[2], o.x[3]);
    const double us = 0.5 - (U < 0.0 ? -U : U);
    const double k = __builtin_floor((2.0 * a / us + b) * U + lam + 0.43);
    *kout = k;
    if (us >= 0.07 && V <= vr) return true;                      // ~87 % of attempts leave here
    if (k < 0.0 || (us < 0.013 && V > us)) return false;
    if (!(V > 0.0)) return true;
    // slow path: the logarithms are evaluated only here (same values as if hoisted)
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
    const double loglam = det_log(lam);
    const double lhs = (det_log(V) + det_log(invalpha)) - det_log(a / (us * us) + b);
    const double rhs = (k * loglam - lam) - det_logfact(k);
    return lhs <= rhs;
}

RL_HD double philox_poisson(double lam, uint64_t seed, uint32_t image, uint32_t pixel) {
    RL_FP_STRICT
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (!(lam > 0.0)) return 0.0;
    if (lam < 10.0) {
        const double enlam = det_exp(-lam);
        double X = 0.0, prod = 1.0;
        for (uint32_t blk = 0; blk < kPoissonMaxBlocks; ++blk) {
            const Philox4 o = philox4x32_10(pixel, image, blk, 0x504F4953u, k0, k1);
            prod = prod * u53(o.x[0], o.x[1]);
            if (!(prod > enlam)) return X;
            X = X + 1.0;
            prod = prod * u53(o.x[2], o.x[3]);
            if (!(prod > enlam)) return X;
            X = X + 1.0;
        }
        return X;
    }
    double k = 0.0;
    for (uint32_t blk = 0; blk < kPoissonMaxBlocks; ++blk)
        if (before_split::philox_ptrs_attempt(lam, k0, k1, image, pixel, blk, &k)) return k;
    return k < 0.0 ? 0.0 : k;
}

}  // namespace before_split

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// Every rate x blocks [0, blocks): mismatch[0] philox_poisson, [1] philox_poisson_fast, [2] philox_ptrs_attempt, [3] the pieces
// with the rate-only values computed once per rate (what the kernel does), each against before_split.  slow_reached: attempts
// that went as far as the logarithm test, so that a caller knows the cases exercise it.
extern "C" void pg_check_pieces(const double* lams, int n, unsigned long long seed, int blocks, long long* mismatch, long long* slow_reached) {
    const int nt = 8;
    std::vector<std::thread> th;
    std::vector<long long> part((size_t)nt * 5, 0);
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t]() {
            long long* m = &part[(size_t)t * 5];
            const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
            for (int i = t; i < n; i += nt) {
                const double lam = lams[i];
                const uint32_t pixel = (uint32_t)i * 2654435761u + 17u, image = (uint32_t)(i % 7);
                if (!same_bits(philox_poisson(lam, seed, image, pixel), before_split::philox_poisson(lam, seed, image, pixel))) ++m[0];
                double ka = -1.0, kb = -1.0;
                const bool fa = philox_poisson_fast(lam, seed, image, pixel, &ka), fb = before_split::philox_poisson_fast(lam, seed, image, pixel, &kb);
                if (fa != fb || !same_bits(ka, kb)) ++m[1];
                if (!(lam >= 10.0)) continue;
                const PtrsRate r = ptrs_rate(lam);
                const PtrsSlow sl = ptrs_slow(r);
                for (int blk = 0; blk < blocks; ++blk) {
                    const bool want = before_split::philox_ptrs_attempt(lam, k0, k1, image, pixel, (uint32_t)blk, &kb);
                    const bool got = philox_ptrs_attempt(lam, k0, k1, image, pixel, (uint32_t)blk, &ka);
                    if (got != want || !same_bits(ka, kb)) ++m[2];
                    const PtrsCandidate c = ptrs_candidate(r, ptrs_block(k0, k1, image, pixel, (uint32_t)blk));
                    bool slow = false;
                    const bool acc = ptrs_accept(r, c, [&]() {
                        slow = true;
                        return sl;
                    });
                    if (acc != want || !same_bits(c.k, kb) || (ptrs_squeeze(r, c) && !want)) ++m[3];
                    if (blk == 0 && (ptrs_squeeze(r, c) != fb)) ++m[3];
                    if (slow) ++m[4];
                }
            }
        });
    for (auto& t : th) t.join();
    for (int j = 0; j < 4; ++j) mismatch[j] = 0;
    *slow_reached = 0;
    for (int t = 0; t < nt; ++t) {
        for (int j = 0; j < 4; ++j) mismatch[j] += part[(size_t)t * 5 + j];
        *slow_reached += part[(size_t)t * 5 + 4];
    }
}

// ---- the kernel body.  The sync object: EmuSync and the atomic add on an LDS counter that EmuSync lacks.
struct PoissonEmuSync : EmuSync {
    unsigned lds_add(unsigned* p, unsigned v) const { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
};
// An element that counts how often it was assigned: the body's stores are `noisy[i] = (T)(value)`.
template <typename F>
struct Counted {
    F v;
    int writes;
    Counted() = default;
    explicit Counted(double d) : v((F)d), writes(0) {}
    explicit operator double() const { return (double)v; }
    Counted& operator=(const Counted& o) {
        v = o.v;
        __atomic_fetch_add(&writes, 1, __ATOMIC_RELAXED);
        return *this;
    }
};

template <typename F>
static void run_groups(const F* noiseless, size_t n_rates, F* noisy, int* writes, unsigned n_pix, unsigned frames, const PoissonKeys& keys, int grid) {
    using T = Counted<F>;
    const size_t total = (size_t)frames * keys.V * n_pix;
    std::vector<T> in(n_rates), out(total);
    for (size_t i = 0; i < n_rates; ++i) in[i].v = noiseless[i];
    for (size_t i = 0; i < total; ++i) {
        out[i].v = noisy[i];   // (the caller's poison)
        out[i].writes = 0;
    }
    const PoissonGroupParams<T> p{in.data(), out.data(), n_pix, frames, keys};
    run_grid(grid, 1, kPoissonGroupPix, kPoissonGroupLds, [&](int tid, int bx, int, unsigned char* lds, EmuSync& s) {
        PoissonEmuSync ps;
        static_cast<EmuSync&>(ps) = s;
        poisson_groups_body<T>(p, (unsigned)tid, (unsigned)bx, (unsigned)grid, lds, ps);
    });
    for (size_t i = 0; i < total; ++i) {
        noisy[i] = out[i].v;
        writes[i] = out[i].writes;
    }
}

// noiseless: n_rate_images images of n_pix rates; noisy [frames][V][n_pix] and writes likewise; grid <= 0: one workgroup per item
extern "C" int pg_run(int is_f64, const void* noiseless, unsigned n_rate_images, void* noisy, int* writes, unsigned n_pix, unsigned frames, unsigned V,
                      unsigned long long seed0, unsigned image0, const unsigned long long* frame_seeds, const unsigned* frame_ids,
                      const unsigned* rate_frame, int grid) {
    const PoissonKeys keys{seed0, image0, V, frame_seeds, frame_ids, rate_frame};
    const int items = (int)poisson_group_items(n_pix, frames, V);
    if (grid <= 0 || grid > items) grid = items;
    if (is_f64) run_groups<double>((const double*)noiseless, (size_t)n_rate_images * n_pix, (double*)noisy, writes, n_pix, frames, keys, grid);
    else run_groups<float>((const float*)noiseless, (size_t)n_rate_images * n_pix, (float*)noisy, writes, n_pix, frames, keys, grid);
    return items;
}

// the same launch drawn value by value with philox_poisson() as it was before the split
template <typename F>
static void ref_groups(const F* noiseless, F* out, unsigned n_pix, unsigned frames, const PoissonKeys& keys) {
    for (unsigned f = 0; f < frames; ++f)
        for (unsigned v = 0; v < keys.V; ++v) {
            const unsigned img = f * keys.V + v;
            const F* rates = keys.image_rates(noiseless, img, n_pix);
            for (unsigned pix = 0; pix < n_pix; ++pix)
                out[(size_t)img * n_pix + pix] = (F)(before_split::philox_poisson((double)rates[pix], keys.seed(img), keys.image(img), pix) + 1e-9);
        }
}
extern "C" void pg_ref(int is_f64, const void* noiseless, void* out, unsigned n_pix, unsigned frames, unsigned V, unsigned long long seed0,
                       unsigned image0, const unsigned long long* frame_seeds, const unsigned* frame_ids, const unsigned* rate_frame) {
    const PoissonKeys keys{seed0, image0, V, frame_seeds, frame_ids, rate_frame};
    if (is_f64) ref_groups<double>((const double*)noiseless, (double*)out, n_pix, frames, keys);
    else ref_groups<float>((const float*)noiseless, (float*)out, n_pix, frames, keys);
}
extern "C" int pg_lds_bytes() { return (int)kPoissonGroupLds; }
