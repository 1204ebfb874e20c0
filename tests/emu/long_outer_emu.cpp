// Host emulator of the outer-decimation COLUMN kernels exactly as fft_kernels.hip launch_col launches them at L = 1152, 2304
// and 4608: every template argument (M, tile widths C / CW / C64, PARK / PARK64, TWLDS / TWLDS_SPLIT) is read from
// OuterCol<L>, the LDS is allocated at the byte count of outer_lds.hpp -- the functions the launcher calls -- and the choice
// between the generic kernel and the one with the row count at compile time is launch_outer's.  float64 runs the device's
// float64 code (no RL_TILE_WIDE_F64 here).  Built by tests/test_long_rows_cpu.py into liblong_outer_emu.so.
// TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <string>

#include "emu_common.hpp"
#include "../../rescan_line_sted_amd/csrc/outer_lds.hpp"

template <int L, typename T>
static std::vector<cx<T>> outer_twiddles() {   // fft_kernels.hip fill_outer_twiddles: the core's table, then W_L^(q k)
    using OC = OuterCol<L>;
    using Core = typename OC::Core;
    constexpr int n_core = PassTw<Core, false, 0>::TOTAL;
    std::vector<double> h(2 * (size_t)(n_core + (OC::M - 1) * Core::L));
    fill_pass_twiddles<Core>(h.data());
    for (int q = 1; q < OC::M; ++q)
        for (int k = 0; k < Core::L; ++k) {
            const long double a = -6.283185307179586476925286766559005768L * (long double)q * (long double)k / (long double)L;
            h[2 * (size_t)(n_core + (q - 1) * Core::L + k)] = (double)cosl(a);
            h[2 * (size_t)(n_core + (q - 1) * Core::L + k) + 1] = (double)sinl(a);
        }
    std::vector<cx<T>> tw(h.size() / 2);
    for (size_t i = 0; i < tw.size(); ++i) tw[i] = mk<T>((T)h[2 * i], (T)h[2 * i + 1]);
    return tw;
}

// k_colconv_outer<L, C, REALP, MODE, T, NYC>
template <int L, int C, bool REALP, int MODE, typename T, int NYC>
static void outer_kernel(const ColParams<T>& p, int gy, size_t lds_bytes) {
    using OC = OuterCol<L>;
    static_assert(sizeof(T) == 4 || MODE == COL_PER_IMAGE, "float64: the whole pass only");
    run_grid((p.kx + C - 1) / C, gy, 64 * C, lds_bytes, [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
        if constexpr (sizeof(T) == 4)
            colconv_outer_body<typename OC::Core, OC::M, C, float, REALP, MODE, (MODE == COL_PER_IMAGE ? OC::PARK : 0),
                               (MODE == COL_PER_IMAGE ? OC::TWLDS : OC::TWLDS_SPLIT), NYC>(p, tid, bx, by, reinterpret_cast<cx<float>*>(lds), s);
        else
            colconv_outer_body<typename OC::Core, OC::M, C, double, REALP, COL_PER_IMAGE, OC::PARK64, 0, NYC>(p, tid, bx, by, reinterpret_cast<cx<double>*>(lds), s);
    });
}
// launch_outer: the generic kernel or -- M x 512 rows, pitch a multiple of the tile width -- the one with the row count at compile time
static int g_n512 = 1;   // RL_N512 (0: the generic kernel whatever the size, what the other is compared with)
template <int L, int C, bool REALP, int MODE, typename T>
static void launch_outer(const ColParams<T>& p, int gy, size_t lds) {
    constexpr int NY = 512 * OuterCol<L>::M;
    if (g_n512 != 0 && p.ny == NY && p.pitch % C == 0) outer_kernel<L, C, REALP, MODE, T, NY>(p, gy, lds);
    else outer_kernel<L, C, REALP, MODE, T, 0>(p, gy, lds);
}

template <int L, typename T>
static ColParams<T> col_params(const T* in, T* out, const T* psf_hat, int real_psf, const cx<T>* tw, int ny, int kx, int pitch, int V) {
    ColParams<T> p;
    p.in = reinterpret_cast<const cx<T>*>(in);
    p.out = reinterpret_cast<cx<T>*>(out);
    p.psf_hat = real_psf ? nullptr : reinterpret_cast<const cx<T>*>(psf_hat);
    p.psf_hat_re = real_psf ? psf_hat : nullptr;
    p.tw = tw;
    p.ny = ny; p.kx = kx; p.pitch = pitch; p.V = V; p.order = 1;
    return p;
}

// launch_col, COL_PER_IMAGE
template <int L, typename T>
static int whole_t(const T* in, T* out, const T* psf_hat, int real_psf, int ny, int kx, int pitch, int V, int frames, int in_sb, int in_sv) {
    using OC = OuterCol<L>;
    auto tw = outer_twiddles<L, T>();
    ColParams<T> p = col_params<L, T>(in, out, psf_hat, real_psf, tw.data(), ny, kx, pitch, V);
    p.in_sb = in_sb; p.in_sv = in_sv; p.mode = COL_PER_IMAGE; p.images = frames * V;
    if constexpr (sizeof(T) == 4) {
        static_assert(OC::value, "f32 outer pass");
        constexpr size_t lds = outer_whole_lds_bytes<OC>();
        if (real_psf) launch_outer<L, OC::CW, true, COL_PER_IMAGE, float>(p, p.images, lds);
        else launch_outer<L, OC::CW, false, COL_PER_IMAGE, float>(p, p.images, lds);
    } else {
        static_assert(OC::value64, "float64 outer pass");
        constexpr size_t lds = outer_whole_lds_bytes_f64<OC>();
        if (real_psf) launch_outer<L, OC::C64, true, COL_PER_IMAGE, double>(p, p.images, lds);
        else launch_outer<L, OC::C64, false, COL_PER_IMAGE, double>(p, p.images, lds);
    }
    return 0;
}
// launch_col, COL_SPLIT_FWD then COL_SPLIT_INV / COL_SPLIT_INV_SUM, as the plan chains them (f32 only).  sum_views = 0 (H): in [frames],
// out [frames * V]; 1 (H_t): in [frames * V], out [frames].  The slot-order spectra between the halves start as NaN.
template <int L>
static int split_t(const float* in, float* out, const float* psf_hat, int real_psf, int ny, int kx, int pitch, int V, int frames, int sum_views) {
    using OC = OuterCol<L>;
    auto tw = outer_twiddles<L, float>();
    ColParams<float> p = col_params<L, float>(in, out, psf_hat, real_psf, tw.data(), ny, kx, pitch, V);
    const int n_in = sum_views ? frames * V : frames;
    const size_t xs_img = (size_t)((kx + OC::C - 1) / OC::C) * outer_slots_tile_elems<typename OC::Core, OC::M, OC::C>();
    std::vector<cx<float>> xs((size_t)n_in * xs_img, mk<float>(NAN, NAN));
    p.in_sb = 1; p.in_sv = 0; p.xs_out = xs.data(); p.xs_in = xs.data();
    constexpr size_t lds = outer_split_lds_bytes<OC>();
    p.mode = COL_SPLIT_FWD; p.images = n_in;
    launch_outer<L, OC::C, false, COL_SPLIT_FWD, float>(p, p.images, lds);
    p.mode = sum_views ? COL_SPLIT_INV_SUM : COL_SPLIT_INV; p.images = sum_views ? frames : frames * V;
    if (sum_views) {
        if (real_psf) launch_outer<L, OC::C, true, COL_SPLIT_INV_SUM, float>(p, p.images, lds);
        else launch_outer<L, OC::C, false, COL_SPLIT_INV_SUM, float>(p, p.images, lds);
    } else {
        if (real_psf) launch_outer<L, OC::C, true, COL_SPLIT_INV, float>(p, p.images, lds);
        else launch_outer<L, OC::C, false, COL_SPLIT_INV, float>(p, p.images, lds);
    }
    return 0;
}

template <int L>
static void table(std::string& out) {
    using OC = OuterCol<L>;
    char b[200];
    auto line = [&](int C, int realp, int mode, const char* t, size_t lds) {
        for (int nyc : {0, 512 * OC::M}) {
            std::snprintf(b, sizeof b, "k_colconv_outer L=%d C=%d REALP=%d MODE=%d T=%s NYC=%d LDS=%zu\n", L, C, realp, mode, t, nyc, lds);
            out += b;
        }
    };
    for (int realp : {1, 0}) line(OC::CW, realp, COL_PER_IMAGE, "f32", outer_whole_lds_bytes<OC>());
    line(OC::C, 0, COL_SPLIT_FWD, "f32", outer_split_lds_bytes<OC>());
    for (int realp : {1, 0}) line(OC::C, realp, COL_SPLIT_INV, "f32", outer_split_lds_bytes<OC>());
    for (int realp : {1, 0}) line(OC::C, realp, COL_SPLIT_INV_SUM, "f32", outer_split_lds_bytes<OC>());
    for (int realp : {1, 0}) line(OC::C64, realp, COL_PER_IMAGE, "f64", outer_whole_lds_bytes_f64<OC>());
}

#define DISPATCH_LONG(L, call)                                 \
    switch (L) {                                               \
        case 1152: { constexpr int LL = 1152; return call; }   \
        case 2304: { constexpr int LL = 2304; return call; }   \
        case 4608: { constexpr int LL = 4608; return call; }   \
        default: return -2;                                    \
    }

extern "C" {

void emu_outer_set_n512(int on) { g_n512 = on; }
// psf_hat: complex [V][kx][L] (transposed layout), or -- real_psf -- its real parts [V][kx][L]
int emu_outer_whole_f32(int L, const float* in, float* out, const float* psf_hat, int real_psf, int ny, int kx, int pitch, int V,
                        int frames, int in_sb, int in_sv) {
    DISPATCH_LONG(L, (whole_t<LL, float>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, in_sb, in_sv)))
}
int emu_outer_whole_f64(int L, const double* in, double* out, const double* psf_hat, int real_psf, int ny, int kx, int pitch, int V,
                        int frames, int in_sb, int in_sv) {
    DISPATCH_LONG(L, (whole_t<LL, double>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, in_sb, in_sv)))
}
int emu_outer_split_f32(int L, const float* in, float* out, const float* psf_hat, int real_psf, int ny, int kx, int pitch, int V,
                        int frames, int sum_views) {
    DISPATCH_LONG(L, (split_t<LL>(in, out, psf_hat, real_psf, ny, kx, pitch, V, frames, sum_views)))
}
// OuterCol<L> as the emulator sees it: M, C, CW, C64, PARK, PARK64, TWLDS, TWLDS_SPLIT, SPLIT
int emu_outer_settings(int L, int* v) {
#define SET(LL) case LL: { using OC = OuterCol<LL>; const int s[9] = {OC::M, OC::C, OC::CW, OC::C64, OC::PARK, OC::PARK64, OC::TWLDS, OC::TWLDS_SPLIT, OC::SPLIT ? 1 : 0}; for (int i = 0; i < 9; ++i) v[i] = s[i]; return 0; }
    switch (L) { SET(1152) SET(2304) SET(4608) }
#undef SET
    return -2;
}
int emu_outer_table(char* buf, int cap) {
    std::string s;
    table<1152>(s); table<2304>(s); table<4608>(s);
    std::snprintf(buf, (size_t)cap, "%s", s.c_str());
    return (int)s.size();
}

}  // extern "C"
