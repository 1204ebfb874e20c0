// Host emulator of the outer-decimation COLUMN kernels exactly as fft_kernels.hip launch_col launches them at L = 1152, 2304
// and 4608: every template argument (M, tile widths C / CW / C64, PARK / PARK64, TWLDS / TWLDS_SPLIT) is read from
// OuterCol<L>, the LDS is allocated at the byte count of outer_lds.hpp -- the functions the launcher calls -- and the variant
// is chosen by select_outer from the list of csrc/kernel_variants.hpp with the device's row counts (DeviceSpecial).  float64
// runs the device's float64 code (no RL_TILE_WIDE_F64 here).  Built by tests/test_long_rows_cpu.py into liblong_outer_emu.so.
// TEST INFRASTRUCTURE ONLY.
#include "emu_common.hpp"

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

// launch_col on an outer length: p.mode, p.images set
static int g_n512 = 1;   // RL_N512 (0: the generic kernel whatever the size, what the other is compared with)
template <int L, typename T>
static int run_outer(const ColParams<T>& p) {
    using S = DeviceSpecial<L, T>;
    OuterKey k;
    if (!select_outer<L>(sizeof(T) == 4, g_n512 ? S::outer_ny : 0, p.mode, p.ny, p.pitch, p.psf_hat_re != nullptr, k)) return -1;
    const bool found = for_each_outer<L, T, S>([&](auto v) {
        using V = decltype(v);
        if (!(v.key() == k)) return false;
        run_grid((p.kx + V::C - 1) / V::C, p.images, 64 * V::C, outer_lds_bytes<OuterCol<L>, T, V::MODE>(), [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
            outer_variant<L>(v, p, tid, bx, by, lds, s);
        });
        return true;
    });
    return found ? 0 : -4;
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
    auto tw = outer_twiddles<L, T>();
    ColParams<T> p = col_params<L, T>(in, out, psf_hat, real_psf, tw.data(), ny, kx, pitch, V);
    p.in_sb = in_sb; p.in_sv = in_sv; p.mode = COL_PER_IMAGE; p.images = frames * V;
    static_assert(kOuterCol<L, T>, "an outer pass of this type");
    return run_outer<L, T>(p);
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
    p.mode = COL_SPLIT_FWD; p.images = n_in;
    if (const int r = run_outer<L, float>(p)) return r;
    p.mode = sum_views ? COL_SPLIT_INV_SUM : COL_SPLIT_INV; p.images = sum_views ? frames : frames * V;
    return run_outer<L, float>(p);
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
}  // extern "C"
template <int L, typename T>
static void table(std::string& out) {   // the rows of this length and type, each with the LDS bytes its launch gets
    for_each_outer<L, T, DeviceSpecial<L, T>>([&](auto v) {
        using V = decltype(v);
        std::string line = line_of<L, T>(v.key());
        line.pop_back();
        out += line + fmt_line(" LDS=%zu\n", outer_lds_bytes<OuterCol<L>, T, V::MODE>());
        return false;
    });
}
extern "C" int emu_outer_table(char* buf, int cap) {
    std::string s;
    table<1152, float>(s); table<1152, double>(s); table<2304, float>(s); table<2304, double>(s); table<4608, float>(s); table<4608, double>(s);
    return copy_out(s, buf, cap);
}
