// Host emulator for the workgroup bodies in rescan_line_sted_amd/csrc/
// conv_kernels.hpp: runs one OS thread per GPU thread with a pthread barrier
// standing in for __syncthreads().  TEST INFRASTRUCTURE ONLY -- it exists so
// the index logic of the HIP kernels (Stockham passes, two-rows-per-transform
// packing, pad/crop, view loops) can be checked against numpy on a machine
// without a GPU.  It is built by tests/test_emulated_kernels.py with g++ and
// is never loaded by the product.
#include <pthread.h>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <type_traits>
#include <vector>

#define RL_TILE_WIDE_F64 1   // the device runs the two-column tile I/O in float only; here its index logic is tested in double
#include "emu_common.hpp"
#include "../../rescan_line_sted_amd/csrc/philox_poisson.hpp"

template <int L, typename T>
static std::vector<cx<T>> twiddles(bool column = false) {   // rows: CfgFor<L>::Cfg, columns: ColCfgFor<L>
    if (column) return twiddles_of<typename ColCfgFor<L>::type, T>();
    return twiddles_of<typename CfgFor<L>::Cfg, T>();
}

// emu_set_special(1): the bodies specialised for a compile-time image size (round 4: NYC / NXC / SUBC / CT template arguments,
// on the device instantiated for the 512 x 512 frames at L = 576) are run in their L = 256 instantiation for 192 pixels and
// 192 rows -- or NY = 128 rows (a multiple of 128 rows: the 16-byte tile I/O).  The variants come from the lists and the
// selectors of csrc/kernel_variants.hpp, as on the device, with these sizes in the place of DeviceSpecial's.
static int g_special = 0;
template <int L, int NY = 192>
struct EmuSpecial {
    static constexpr int col_ny = L == 256 ? NY : 0, row_nx = L == 256 ? 192 : 0, pair_nx = row_nx, outer_ny = 0;
};

template <int L, typename T>
static int col_t(const T* in, T* out, const T* psf_hat, int ny, int kx, int pitch, int V, int frames,
                 int in_sb, int in_sv, int mode) {
    using CF = CfgFor<L>;
    using Cfg = typename ColCfgFor<L>::type;      // the column kernels' geometry
    constexpr int C = sizeof(T) == 4 ? CF::C32 : CF::C64;
    auto tw = twiddles<L, T>(true);
    ColParams<T> p;
    p.in = reinterpret_cast<const cx<T>*>(in);
    p.out = reinterpret_cast<cx<T>*>(out);
    p.psf_hat = reinterpret_cast<const cx<T>*>(psf_hat);
    p.tw = tw.data();
    p.ny = ny; p.kx = kx; p.pitch = pitch; p.V = V; p.in_sb = in_sb; p.in_sv = in_sv;
    p.mode = mode;
    const int gy = (mode == COL_PER_IMAGE) ? frames * V : frames;   // as rlsted.cpp col_t()
    p.images = gy; p.order = 1;
    p.residual = 1;   // (the compile-time sizes run with the compact twiddles)
    ColKey k;
    if (!select_colconv(WavePrivate<Cfg>::value, !g_special ? 0 : ny == 128 ? 128 : EmuSpecial<L>::col_ny, mode, ny, V, pitch % C == 0, false, true, k)) return -3;
    run_grid((kx + C - 1) / C, gy, Cfg::T * C, (size_t)C * LdsSlots<Cfg>::value * sizeof(cx<T>),
             [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
                 auto run = [&](auto v) {
                     if (!(v.key() == k)) return false;
                     colconv_variant<L, C>(v, p, tid, bx, by, lds, s);
                     return true;
                 };
                 for_each_colconv<L, EmuSpecial<L>>(run) || for_each_colconv<L, EmuSpecial<L, 128>>(run);
             });
    return 0;
}

// RowParams::sub_one of every row launch (conv_kernels.hpp rl_ratio: ROW_RATIO stores rowFFT(ratio - 1), ROW_UPDATE
// multiplies by max(1 + acc / norm, 0))
static int g_sub_one = 0;

template <int L, typename T>
static int row_t(int mode, const T* spec_in, T* spec_out, const T* src, T* dst, const T* norm, const T* scale,
                 int ny, int nx, int pitch, int V, int gy) {
    using CF = CfgFor<L>;
    using Cfg = typename CF::Cfg;
    constexpr int Q = sizeof(T) == 4 ? CF::Q32 : CF::Q64;
    auto tw = twiddles<L, T>();
    RowParams<T> p;
    p.sub_one = g_sub_one;
    p.spec_in = reinterpret_cast<const cx<T>*>(spec_in);
    p.spec_out = reinterpret_cast<cx<T>*>(spec_out);
    p.src = src; p.dst = dst; p.norm = norm; p.scale = scale; p.tw = tw.data();
    p.ny = ny; p.nx = nx; p.pitch = pitch; p.V = V;
    RowKey k;
    if (!select_rowpass(g_special ? EmuSpecial<L>::row_nx : 0, mode, nx, V, p.sub_one != 0, k)) return -1;
    run_grid(((ny + 1) / 2 + Q - 1) / Q, gy, Cfg::T * Q, (size_t)Q * LdsSlots<Cfg>::value * sizeof(cx<T>),
             [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
                 for_each_rowpass<L, EmuSpecial<L>>([&](auto v) {
                     if (!(v.key() == k)) return false;
                     rowpass_variant<L, Q>(v, p, tid, bx, by, lds, s);
                     return true;
                 });
             });
    return 0;
}

#define DISPATCH_L(L, call)                         \
    switch (L) {                                    \
        case 64: { constexpr int LL = 64; return call; }     \
        case 192: { constexpr int LL = 192; return call; }   \
        case 256: { constexpr int LL = 256; return call; }   \
        case 576: { constexpr int LL = 576; return call; }   \
        default: return -2;                         \
    }

extern "C" {

void emu_set_sub_one(int on) { g_sub_one = on; }
void emu_set_special(int on) { g_special = on; }
void emu_set_park(int on);

// returns 1 if the column kernel of this length reads psf_hat transposed, 0 if not, <0 unknown L
int emu_geometry(int L, int* T, int* C, int* Q) {
#define GEO(LL) case LL: *T = CfgFor<LL>::Cfg::T; *C = CfgFor<LL>::C64; *Q = CfgFor<LL>::Q64; return WavePrivate<ColCfgFor<LL>::type>::value ? 1 : 0;
    switch (L) { GEO(64) GEO(192) GEO(256) GEO(576) GEO(1152) GEO(2304) GEO(4608) }
    return -2;
}

int emu_col_f64(int L, const double* in, double* out, const double* psf_hat, int ny, int kx, int pitch, int V,
                int frames, int in_sb, int in_sv, int mode) {
    DISPATCH_L(L, (col_t<LL, double>(in, out, psf_hat, ny, kx, pitch, V, frames, in_sb, in_sv, mode)))
}
int emu_col_f32(int L, const float* in, float* out, const float* psf_hat, int ny, int kx, int pitch, int V,
                int frames, int in_sb, int in_sv, int mode) {
    DISPATCH_L(L, (col_t<LL, float>(in, out, psf_hat, ny, kx, pitch, V, frames, in_sb, in_sv, mode)))
}
int emu_row_f64(int L, int mode, const double* spec_in, double* spec_out, const double* src, double* dst,
                const double* norm, const double* scale, int ny, int nx, int pitch, int V, int gy) {
    DISPATCH_L(L, (row_t<LL, double>(mode, spec_in, spec_out, src, dst, norm, scale, ny, nx, pitch, V, gy)))
}
int emu_row_f32(int L, int mode, const float* spec_in, float* spec_out, const float* src, float* dst,
                const float* norm, const float* scale, int ny, int nx, int pitch, int V, int gy) {
    DISPATCH_L(L, (row_t<LL, float>(mode, spec_in, spec_out, src, dst, norm, scale, ny, nx, pitch, V, gy)))
}

// rowpair_body (two frames in one complex image): spectra [pairs][ny][L]; frames = images covered by the launch
int emu_row_pair_f64(int L, int mode, const double* spec_in, double* spec_out, const double* src, double* dst, const double* norm,
                     int ny, int nx, int frames, int in_mod);
int emu_row_pair_f32(int L, int mode, const float* spec_in, float* spec_out, const float* src, float* dst, const float* norm,
                     int ny, int nx, int frames, int in_mod);

// colconv_outer_body (long column transforms on a wave-private core): L = M * Li, Li in {256, 576}.
// psf_hat: complex [V][kx][L] (transposed layout), or -- real_psf -- its real parts [V][kx][L].
}  // extern "C"
// ColParams-independent: waiting core results per lane kept in LDS by the whole pass (conv_kernels.hpp PARK); 0 = none
static int g_park = 0;
// Settings of the outer pass.  On the product's core (576) they ARE the product's, read from OuterCol<M * 576>; the 256 core
// is a stand-in for speed with settings of its own.  (The instantiations exactly as launch_col makes them -- tile widths and
// LDS byte counts included -- are in long_outer_emu.cpp.)
template <class Core, int M, int C>
struct OuterSet {
    static constexpr int PARK = M == 4 ? 3 : M == 8 ? 14 : 5, PARK64 = M == 4 ? 10 : M == 8 ? 24 : 4;
    static constexpr int TWLDS = (M == 8 || C == 16) ? 2 : 1, TWLDS_SPLIT = M == 8 ? 2 : M == 4 ? 1 : 0;
};
template <int M, int C>
struct OuterSet<CfgFor<576>::Cfg, M, C> {
    using OC = OuterCol<M * 576>;
    static_assert(OC::value && OC::M == M, "an outer pass the product has");
    static constexpr int PARK = OC::PARK > 0 ? OC::PARK : 5, PARK64 = OC::PARK64 > 0 ? OC::PARK64 : 4;   // (1152 parks nothing: the test's values)
    static constexpr int TWLDS = OC::TWLDS, TWLDS_SPLIT = OC::TWLDS_SPLIT;
};
template <class Core, int M, typename T, int C = 8>
static int col_outer_t(const T* in, T* out, const T* psf_hat, int real_psf, int ny, int kx, int pitch, int V, int frames,
                       int in_sb, int in_sv, int mode = COL_PER_IMAGE) {
    constexpr int L = M * Core::L;
    constexpr int n_core = PassTw<Core, false, 0>::TOTAL;
    std::vector<double> h(2 * (size_t)(n_core + (M - 1) * Core::L));
    fill_pass_twiddles<Core>(h.data());
    for (int q = 1; q < M; ++q)
        for (int k = 0; k < Core::L; ++k) {
            const long double a = -6.283185307179586476925286766559005768L * (long double)q * (long double)k / (long double)L;
            h[2 * (size_t)(n_core + (q - 1) * Core::L + k)] = (double)cosl(a);
            h[2 * (size_t)(n_core + (q - 1) * Core::L + k) + 1] = (double)sinl(a);
        }
    std::vector<cx<T>> tw(h.size() / 2);
    for (size_t i = 0; i < tw.size(); ++i) tw[i] = mk<T>((T)h[2 * i], (T)h[2 * i + 1]);
    ColParams<T> p;
    p.in = reinterpret_cast<const cx<T>*>(in);
    p.out = reinterpret_cast<cx<T>*>(out);
    p.psf_hat = real_psf ? nullptr : reinterpret_cast<const cx<T>*>(psf_hat);
    p.psf_hat_re = real_psf ? psf_hat : nullptr;
    p.tw = tw.data();
    p.ny = ny; p.kx = kx; p.pitch = pitch; p.V = V; p.in_sb = in_sb; p.in_sv = in_sv;
    p.mode = mode; p.images = mode == COL_PER_IMAGE ? frames * V : frames; p.order = 1;
    // parked values: OuterSet (g_park == 1: the f32 kernels' count, 2: the float64 kernels')
    auto parked = [&](auto park_c) {
        constexpr int PARK = decltype(park_c)::value;
        constexpr int TWLDS = OuterSet<Core, M, C>::TWLDS;     // the twiddles from an LDS copy (the core's; 2: the outer table too)
        run_grid((kx + C - 1) / C, p.images, 64 * C,
                 ((size_t)C * LdsSlots<Core>::value + (size_t)PARK * 64 * C + (TWLDS > 0 ? PassTw<Core, false, 0>::TOTAL : 0) + (TWLDS > 1 ? (M - 1) * Core::L : 0)) * sizeof(cx<T>),
                 [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
                     cx<T>* l = reinterpret_cast<cx<T>*>(lds);
                     if (real_psf) colconv_outer_body<Core, M, C, T, true, COL_PER_IMAGE, PARK, TWLDS>(p, tid, bx, by, l, s);
                     else colconv_outer_body<Core, M, C, T, false, COL_PER_IMAGE, PARK, TWLDS>(p, tid, bx, by, l, s);
                 });
    };
    if (g_park == 1) {
        parked(std::integral_constant<int, OuterSet<Core, M, C>::PARK>{});
        return 0;
    }
    if (g_park == 2) {
        parked(std::integral_constant<int, OuterSet<Core, M, C>::PARK64>{});
        return 0;
    }
    run_grid((kx + C - 1) / C, p.images, 64 * C, (size_t)C * LdsSlots<Core>::value * sizeof(cx<T>),
             [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
                 cx<T>* l = reinterpret_cast<cx<T>*>(lds);
                 if constexpr (Core::L == 256) {   // emu_set_special: the row count at compile time (the device: M x 512 rows on the 576 core)
                     if (g_special && ny == M * 192 && pitch % C == 0) {
                         if (real_psf) colconv_outer_body<Core, M, C, T, true, COL_PER_IMAGE, 0, 0, M * 192>(p, tid, bx, by, l, s);
                         else colconv_outer_body<Core, M, C, T, false, COL_PER_IMAGE, 0, 0, M * 192>(p, tid, bx, by, l, s);
                         return;
                     }
                     if (g_special && ny == M * 128 && pitch % C == 0) {   // (classes of 128 rows: the 16-byte tile I/O)
                         if (real_psf) colconv_outer_body<Core, M, C, T, true, COL_PER_IMAGE, 0, 0, M * 128>(p, tid, bx, by, l, s);
                         else colconv_outer_body<Core, M, C, T, false, COL_PER_IMAGE, 0, 0, M * 128>(p, tid, bx, by, l, s);
                         return;
                     }
                 }
                 if (real_psf) colconv_outer_body<Core, M, C, T, true>(p, tid, bx, by, l, s);
                 else colconv_outer_body<Core, M, C, T, false>(p, tid, bx, by, l, s);
             });
    return 0;
}
template <class Core, int M, typename T>
static int col_outer_split_t(const T* in, T* out, const T* psf_hat, int real_psf, int ny, int kx, int pitch, int V, int frames,
                       int sum_views) {
    constexpr int C = 8, L = M * Core::L;
    constexpr int n_core = PassTw<Core, false, 0>::TOTAL;
    std::vector<double> h(2 * (size_t)(n_core + (M - 1) * Core::L));
    fill_pass_twiddles<Core>(h.data());
    for (int q = 1; q < M; ++q)
        for (int k = 0; k < Core::L; ++k) {
            const long double a = -6.283185307179586476925286766559005768L * (long double)q * (long double)k / (long double)L;
            h[2 * (size_t)(n_core + (q - 1) * Core::L + k)] = (double)cosl(a);
            h[2 * (size_t)(n_core + (q - 1) * Core::L + k) + 1] = (double)sinl(a);
        }
    std::vector<cx<T>> tw(h.size() / 2);
    for (size_t i = 0; i < tw.size(); ++i) tw[i] = mk<T>((T)h[2 * i], (T)h[2 * i + 1]);
    ColParams<T> p;
    p.in = reinterpret_cast<const cx<T>*>(in);
    p.out = reinterpret_cast<cx<T>*>(out);
    p.psf_hat = real_psf ? nullptr : reinterpret_cast<const cx<T>*>(psf_hat);
    p.psf_hat_re = real_psf ? psf_hat : nullptr;
    p.tw = tw.data();
    // The split pass as the plan runs it.  sum_views = 0 (H): COL_SPLIT_FWD over the `frames` input images, COL_SPLIT_INV per
    // (frame, view) -> frames * V output images.  sum_views = 1 (H_t): COL_SPLIT_FWD over the frames * V input images,
    // COL_SPLIT_INV_SUM per frame -> `frames` output images.  The slot-order spectra are poisoned with NaN first.
    const int n_in = sum_views ? frames * V : frames;
    const size_t xs_img = (size_t)((kx + C - 1) / C) * outer_slots_tile_elems<Core, M, C>();
    std::vector<cx<T>> xs((size_t)n_in * xs_img, mk<T>((T)NAN, (T)NAN));
    p.ny = ny; p.kx = kx; p.pitch = pitch; p.V = V; p.in_sb = 1; p.in_sv = 0; p.order = 1;
    p.xs_out = xs.data();
    p.xs_in = xs.data();
    constexpr int TWS = OuterSet<Core, M, C>::TWLDS_SPLIT;
    constexpr size_t lds_split = ((size_t)C * LdsSlots<Core>::value + (TWS > 0 ? PassTw<Core, false, 0>::TOTAL : 0) + (TWS > 1 ? (M - 1) * Core::L : 0)) * sizeof(cx<T>);
    p.mode = COL_SPLIT_FWD; p.images = n_in;
    run_grid((kx + C - 1) / C, p.images, 64 * C, lds_split,
             [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
                 colconv_outer_body<Core, M, C, T, false, COL_SPLIT_FWD, 0, TWS>(p, tid, bx, by, reinterpret_cast<cx<T>*>(lds), s);
             });
    p.mode = sum_views ? COL_SPLIT_INV_SUM : COL_SPLIT_INV; p.images = sum_views ? frames : frames * V;
    run_grid((kx + C - 1) / C, p.images, 64 * C, lds_split,
             [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
                 cx<T>* l = reinterpret_cast<cx<T>*>(lds);
                 if (sum_views) {
                     if (real_psf) colconv_outer_body<Core, M, C, T, true, COL_SPLIT_INV_SUM, 0, TWS>(p, tid, bx, by, l, s);
                     else colconv_outer_body<Core, M, C, T, false, COL_SPLIT_INV_SUM, 0, TWS>(p, tid, bx, by, l, s);
                 } else {
                     if (real_psf) colconv_outer_body<Core, M, C, T, true, COL_SPLIT_INV, 0, TWS>(p, tid, bx, by, l, s);
                     else colconv_outer_body<Core, M, C, T, false, COL_SPLIT_INV, 0, TWS>(p, tid, bx, by, l, s);
                 }
             });
    return 0;
}
template <int L, typename T>
static int row_pair_t(int mode, const T* spec_in, T* spec_out, const T* src, T* dst, const T* norm, int ny, int nx, int frames, int in_mod) {
    using CF = CfgFor<L>;
    using Cfg = typename CF::Cfg;
    if constexpr (WavePrivate<Cfg>::value) {
        constexpr int Q = sizeof(T) == 4 ? CF::Q32 : CF::Q64;
        auto tw = twiddles<L, T>();
        RowParams<T> p;
        p.spec_in = reinterpret_cast<const cx<T>*>(spec_in);
        p.spec_out = reinterpret_cast<cx<T>*>(spec_out);
        p.src = src; p.dst = dst; p.norm = norm; p.scale = nullptr; p.tw = tw.data();
        p.ny = ny; p.nx = nx; p.pitch = L; p.V = 1; p.frames = frames; p.in_mod = in_mod;
        p.sub_one = g_sub_one;
        PairKey k;
        if (!select_rowpair(g_special ? EmuSpecial<L>::pair_nx : 0, mode, nx, p.V, p.sub_one != 0, k)) return -1;
        run_grid((ny + Q - 1) / Q, (frames + 1) / 2, 64 * Q, (size_t)Q * LdsSlots<Cfg>::value * sizeof(cx<T>),
                 [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
                     for_each_rowpair<L, EmuSpecial<L>>([&](auto v) {
                         using V = decltype(v);
                         if (!(v.key() == k)) return false;
                         rowpair_body<Cfg, Q, V::MODE, T, V::NXC, V::SUBC>(p, tid, bx, by, reinterpret_cast<cx<T>*>(lds), s);
                         return true;
                     });
                 });
        return 0;
    } else {
        return -3;
    }
}
extern "C" {
int emu_row_pair_f64(int L, int mode, const double* spec_in, double* spec_out, const double* src, double* dst, const double* norm,
                     int ny, int nx, int frames, int in_mod) {
    DISPATCH_L(L, (row_pair_t<LL, double>(mode, spec_in, spec_out, src, dst, norm, ny, nx, frames, in_mod)))
}
int emu_row_pair_f32(int L, int mode, const float* spec_in, float* spec_out, const float* src, float* dst, const float* norm,
                     int ny, int nx, int frames, int in_mod) {
    DISPATCH_L(L, (row_pair_t<LL, float>(mode, spec_in, spec_out, src, dst, norm, ny, nx, frames, in_mod)))
}
void emu_set_park(int on) { g_park = on; }
// every variant of the lists this library can run, one per line (the format of long_emu.cpp emu_long_table; the 128-row
// column variants are the 192-row rows at another size and are not repeated)
int emu_table(char* buf, int cap) {
    std::string s;
#define ROWS(LL) list_variants<LL, float, EmuSpecial<LL>>(s, true, true); list_variants<LL, double, EmuSpecial<LL>>(s, true, true);
    ROWS(64) ROWS(192) ROWS(256) ROWS(576)
#undef ROWS
    return copy_out(s, buf, cap);
}
int emu_col_outer_f64(int Li, int M, const double* in, double* out, const double* psf_hat, int real_psf, int ny, int kx,
                      int pitch, int V, int frames, int in_sb, int in_sv) {
    using C256 = CfgFor<256>::Cfg;
    using C576 = CfgFor<576>::Cfg;
    if (Li == 256 && M == 4) return col_outer_t<C256, 4, double>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, in_sb, in_sv);
    if (Li == 256 && M == 16) return col_outer_t<C256, 4, double, 16>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, in_sb, in_sv);   // M = 4 on 16-column tiles
    if (Li == 256 && M == 2) return col_outer_t<C256, 2, double>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, in_sb, in_sv);
    if (Li == 576 && M == 4) return col_outer_t<C576, 4, double>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, in_sb, in_sv);
    if (Li == 256 && M == 8) return col_outer_t<C256, 8, double>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, in_sb, in_sv);
    if (Li == 576 && M == 8) return col_outer_t<C576, 8, double>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, in_sb, in_sv);
    return -2;
}
// the split column pass (COL_SPLIT_FWD then COL_SPLIT_INV / COL_SPLIT_INV_SUM); sum_views: 0 = H (in [frames], out [frames * V]),
// 1 = H_t with the views summed (in [frames * V], out [frames])
int emu_col_outer_split_f64(int Li, int M, const double* in, double* out, const double* psf_hat, int real_psf, int ny, int kx,
                            int pitch, int V, int frames, int sum_views) {
    using C256 = CfgFor<256>::Cfg;
    using C576 = CfgFor<576>::Cfg;
    if (Li == 256 && M == 4) return col_outer_split_t<C256, 4, double>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, sum_views);
    if (Li == 256 && M == 2) return col_outer_split_t<C256, 2, double>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, sum_views);
    if (Li == 576 && M == 4) return col_outer_split_t<C576, 4, double>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, sum_views);
    if (Li == 256 && M == 8) return col_outer_split_t<C256, 8, double>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, sum_views);
    if (Li == 576 && M == 8) return col_outer_split_t<C576, 8, double>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, sum_views);
    return -2;
}

// host build of the device Poisson sampler (philox_poisson.hpp)
int emu_poisson(const double* lam, int n, unsigned long long seed, unsigned image, double* out) {
    for (int i = 0; i < n; ++i) out[i] = philox_poisson(lam[i], seed, image, (unsigned)i);
    return 0;
}
// first-attempt-only variant used by the fast Poisson kernel: flags[i] = accepted
int emu_poisson_fast(const double* lam, int n, unsigned long long seed, unsigned image, double* out, int* flags) {
    for (int i = 0; i < n; ++i) flags[i] = philox_poisson_fast(lam[i], seed, image, (unsigned)i, &out[i]) ? 1 : 0;
    return 0;
}
void emu_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* out) {
    Philox4 o = philox4x32_10(c0, c1, c2, c3, k0, k1);
    for (int i = 0; i < 4; ++i) out[i] = o.x[i];
}
}
