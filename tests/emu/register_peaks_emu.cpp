// Host emulator of k_register_peaks (rescan_line_sted_amd/csrc/register_kernels.hpp PEAKS, register_peaks.hip): the very same
// thread bodies, run thread by thread -- a workgroup of kRegThreads threads per pair scans its displacements, the "LDS" arrays meet
// the tree step by step, thread 0 finishes, every thread writes its share of the surface -- and rl_register_estimate's order of
// stages composed from the emulated sums and shift of register_emu.cpp with the product's own rules (reg_estimate_first,
// reg_estimate_refine).  TEST INFRASTRUCTURE ONLY -- built by tests/test_register_peaks_cpu.py with g++ (-ffp-contract=off), as a
// shared library and, with -DPEAKS_EMU_MAIN, as a stand-alone program for the sanitizers; never loaded by the product.
#include "register_emu.cpp"

namespace {

void peaks_run(const RegPeakArgs& a) {
    const int nd = (2 * a.R + 1) * (2 * a.R + 1);
    std::vector<double> sv(kRegThreads);                 // exactly the kernel's LDS arrays
    std::vector<int> si(kRegThreads), sf(kRegThreads);
    for (int pair = 0; pair < a.pairs; ++pair) {
        const double* tp = a.tot + (size_t)pair * (nd * kRegFields + 2);
        for (int t = 0; t < kRegThreads; ++t) reg_peak_scan(tp, nd, a.n, t, sv[t], si[t], sf[t]);
        for (int h = kRegThreads / 2; h > 0; h >>= 1)
            for (int t = 0; t < kRegThreads; ++t) reg_peak_tree_step(sv.data(), si.data(), sf.data(), t, h);
        reg_peak_finish(tp, a.R, a.n, sv[0], si[0], sf[0], a.peaks + (size_t)pair * kPeakFields);
        if (a.surf)
            for (int t = 0; t < kRegThreads; ++t) reg_peak_surface(tp, nd, a.n, t, sf[0], a.surf + (size_t)pair * nd);
    }
}

// the sums of register_emu.cpp as the rows k_register_totals leaves them [pairs][nd * 3 + 2]
std::vector<double> tot_rows(const void* a, int a_dtype, const long long* a_off, const void* b, int b_dtype, const long long* b_off, int pairs,
                             int ny, int nx, int R, int M) {
    const int nd = (2 * R + 1) * (2 * R + 1), per = nd * kRegFields + 2;
    std::vector<double> S((size_t)pairs * nd * kRegFields), A((size_t)pairs * 2), tot((size_t)pairs * per);
    emu_register_sums(a, a_dtype, a_off, b, b_dtype, b_off, pairs, ny, nx, R, M, S.data(), A.data(), nullptr);
    for (int i = 0; i < pairs; ++i) {
        std::memcpy(tot.data() + (size_t)i * per, S.data() + (size_t)i * nd * kRegFields, sizeof(double) * nd * kRegFields);
        tot[(size_t)i * per + nd * kRegFields] = A[2 * i];
        tot[(size_t)i * per + nd * kRegFields + 1] = A[2 * i + 1];
    }
    return tot;
}

}  // namespace

extern "C" {
// tot [pairs][(2R+1)^2 * 3 + 2] -> peaks [pairs][5], surf NULL or [pairs][(2R+1)^2].  The caller has checked the arguments.
int emu_register_peaks(const double* tot, int pairs, int R, double n, double* peaks, double* surf) {
    if (pairs < 1 || R < 1 || R > kRegMaxR) return -1;
    RegPeakArgs a;
    a.tot = tot; a.peaks = peaks; a.surf = surf; a.pairs = pairs; a.R = R; a.n = n;
    peaks_run(a);
    return 0;
}

// rl_register_estimate's stages on host arrays: shifts [pairs][2], fields [pairs][3], surf NULL or [pairs][(2R+1)^2]
int emu_register_estimate(const void* a, int a_dtype, const long long* a_off, const void* b, int b_dtype, const long long* b_off, int pairs,
                          int ny, int nx, int R, int M, int refine, double* shifts, double* fields, double* surf) {
    if (pairs < 1 || R < 1 || R > kRegMaxR || M < R || ny - 2 * M < 8 || nx - 2 * M < 8 || refine < 0) return -1;
    const double n = (double)((long long)(ny - 2 * M) * (nx - 2 * M));
    const size_t n_pix = (size_t)ny * nx, esize = b_dtype == 0 ? sizeof(float) : sizeof(double);
    std::vector<double> tot = tot_rows(a, a_dtype, a_off, b, b_dtype, b_off, pairs, ny, nx, R, M), pk((size_t)pairs * kPeakFields);
    emu_register_peaks(tot.data(), pairs, R, n, pk.data(), surf);
    for (int i = 0; i < pairs; ++i) reg_estimate_first(&pk[(size_t)i * kPeakFields], shifts + 2 * i, fields + 3 * i);
    std::vector<int> live;
    for (int i = 0; i < pairs; ++i)
        if (fields[3 * i + 2] == 0.0) live.push_back(i);
    std::vector<double> scratch(live.size() * n_pix);
    std::vector<long long> la(live.size()), lb(live.size());
    for (size_t k = 0; k < live.size(); ++k) {
        la[k] = a_off[live[k]];
        lb[k] = (long long)(k * n_pix);
    }
    for (int pass = 0; pass < refine && !live.empty(); ++pass) {
        for (size_t k = 0; k < live.size(); ++k)
            emu_shift_images((const char*)b + (size_t)b_off[live[k]] * esize, b_dtype, 1, ny, nx, shifts + 2 * live[k], 3, -HUGE_VAL,
                             scratch.data() + k * n_pix, 1, nullptr);
        std::vector<double> t1 = tot_rows(a, a_dtype, la.data(), scratch.data(), 1, lb.data(), (int)live.size(), ny, nx, 1, M);
        emu_register_peaks(t1.data(), (int)live.size(), 1, n, pk.data(), nullptr);
        for (size_t k = 0; k < live.size(); ++k) reg_estimate_refine(&pk[k * kPeakFields], shifts + 2 * live[k], fields + 3 * live[k]);
    }
    return 0;
}
}

#ifdef PEAKS_EMU_MAIN
// The stand-alone program of the sanitizer run: the sums rows, the fields and the surfaces are heap blocks of EXACTLY their byte
// counts and the "LDS" arrays exactly the kernel's, so a read or a write past any of them is the sanitizer's to find.  Results are
// held to a plain loop written here (first maximum, flat).  Prints "ok <pairs>".
namespace {
unsigned g_state = 88172645u;
double next_unit() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 17;
    g_state ^= g_state << 5;
    return (double)(g_state >> 8) / 16777216.0;
}
template <typename T>
struct Exact {
    T* p;
    explicit Exact(size_t count) : p((T*)std::malloc(count * sizeof(T))) {}
    ~Exact() { std::free(p); }
    Exact(const Exact&) = delete;
};

int peaks_case(int R, int pairs, long* done) {
    const int W = 2 * R + 1, nd = W * W, per = nd * 3 + 2;
    const double n = 400.0;
    Exact<double> tot((size_t)pairs * per), peaks((size_t)pairs * kPeakFields), surf((size_t)pairs * nd);
    for (int i = 0; i < pairs; ++i) {
        double* tp = tot.p + (size_t)i * per;
        for (int d = 0; d < nd; ++d) {
            const double s0 = next_unit() * 100.0;
            tp[3 * d] = s0;
            tp[3 * d + 1] = s0 * s0 / n + 1.0 + next_unit();
            tp[3 * d + 2] = next_unit() * 10.0;
        }
        if (nd > 3 && i % 3 == 1) {                      // a tie: the later copy must lose
            const int p = (int)(next_unit() * (nd - 1)), q = nd - 1 - (p % 2);
            tp[3 * p + 2] = 1e4;
            for (int f = 0; f < 3; ++f) tp[3 * q + f] = tp[3 * p + f];
        }
        tp[3 * nd] = next_unit() * 50.0;
        tp[3 * nd + 1] = tp[3 * nd] * tp[3 * nd] / n + (i % 5 == 4 ? 0.0 : 2.0);   // every fifth pair flat: va = 0
    }
    if (emu_register_peaks(tot.p, pairs, R, n, peaks.p, surf.p)) return 1;
    for (int i = 0; i < pairs; ++i) {
        const double* pk = peaks.p + (size_t)i * kPeakFields;
        const bool flat = i % 5 == 4;
        if (pk[4] != (flat ? 1.0 : 0.0)) return 1;
        if (flat) {
            for (int d = 0; d < nd; ++d)
                if (surf.p[(size_t)i * nd + d] != 0.0) return 1;
            continue;
        }
        int best = 0;
        for (int d = 1; d < nd; ++d)
            if (surf.p[(size_t)i * nd + d] > surf.p[(size_t)i * nd + best]) best = d;
        if (pk[2] != surf.p[(size_t)i * nd + best] || !(std::fabs(pk[0] - (best / W - R)) <= 0.5) || !(std::fabs(pk[1] - (best % W - R)) <= 0.5)) {
            std::printf("peaks R %d pair %d: %d %.17g %.17g %.17g\n", R, i, best, pk[0], pk[1], pk[2]);
            return 1;
        }
    }
    ++*done;
    return 0;
}
}  // namespace

int main() {
    long done = 0;
    for (int R : {1, 2, 8, 32})
        if (peaks_case(R, 7, &done)) return 1;
    std::printf("ok %ld\n", done);
    return 0;
}
#endif
