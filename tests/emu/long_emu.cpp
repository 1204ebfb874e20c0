// Host emulator of the ROW kernels of the long, workgroup-synchronous lengths (L = 1152, 2304, 4608): rowpass_body in every
// mode and rowpair_body on the `Q == 1` branch of k_rowpair, chosen by the selectors and instantiated from the lists of
// csrc/kernel_variants.hpp, as fft_kernels.hip does it -- with the device's compile-time sizes (DeviceSpecial).  A translation
// unit of its own -- tests/test_long_rows_cpu.py builds it into liblong_emu.so -- so that libemu.so keeps its build time.
// It also lists the DEVICE's variants of any length and runs the device's selectors (tests/test_kernel_variants.py).
// TEST INFRASTRUCTURE ONLY.
#include "emu_common.hpp"

template <int L, typename T>
struct LongRow {
    using CF = CfgFor<L>;
    using Cfg = typename CF::Cfg;
    using Special = DeviceSpecial<L, T>;
    static constexpr int Q = sizeof(T) == 4 ? CF::Q32 : CF::Q64;
    static constexpr int QP = Q;   // fft_kernels.hip: kPairQ32 = WavePrivate ? RL_PAIR_Q32 : kQ32
    static_assert(!WavePrivate<Cfg>::value && kPairRows<L> && QP == 1, "the wave-private lengths are emu.cpp's; k_rowpair: WavePrivate || Q == 1");
    static constexpr size_t lds_bytes(int q) { return (size_t)q * LdsSlots<Cfg>::value * sizeof(cx<T>); }

    static int row(int mode, const RowParams<T>& p, int gy) {
        RowKey k;
        if (!select_rowpass(Special::row_nx, mode, p.nx, p.V, p.sub_one != 0, k)) return -1;
        const bool found = for_each_rowpass<L, Special>([&](auto v) {
            if (!(v.key() == k)) return false;
            run_grid(((p.ny + 1) / 2 + Q - 1) / Q, gy, Cfg::T * Q, lds_bytes(Q), [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
                rowpass_variant<L, Q>(v, p, tid, bx, by, lds, s);
            });
            return true;
        });
        return found ? 0 : -4;   // the selector names a row the list does not have
    }
    // special == 0: the run-time-size bodies whatever the size (what the others are compared with)
    static int pair(int mode, const RowParams<T>& p, int gy, int special) {
        PairKey k;
        if (!select_rowpair(special ? Special::pair_nx : 0, mode, p.nx, p.V, p.sub_one != 0, k)) return -1;
        const bool found = for_each_rowpair<L, Special>([&](auto v) {
            using V = decltype(v);
            if (!(v.key() == k)) return false;
            run_grid((p.ny + QP - 1) / QP, gy, Cfg::T * QP, lds_bytes(QP), [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
                rowpair_body<Cfg, QP, V::MODE, T, V::NXC, V::SUBC>(p, tid, bx, by, reinterpret_cast<cx<T>*>(lds), s);
            });
            return true;
        });
        return found ? 0 : -4;
    }
};

template <int L, typename T>
static RowParams<T> params(const T* spec_in, T* spec_out, const T* src, T* dst, const T* norm, const T* scale, const cx<T>* tw,
                           int ny, int nx, int pitch, int V, int frames, int in_mod, int sub_one, unsigned long long* unresolved) {
    RowParams<T> p;
    p.spec_in = reinterpret_cast<const cx<T>*>(spec_in);
    p.spec_out = reinterpret_cast<cx<T>*>(spec_out);
    p.src = src; p.dst = dst; p.norm = norm; p.scale = scale; p.tw = tw;
    p.ny = ny; p.nx = nx; p.pitch = pitch; p.V = V; p.frames = frames; p.in_mod = in_mod; p.sub_one = sub_one;
    p.unresolved = unresolved;
    return p;
}
template <int L, typename T>
static int row_t(int mode, const T* spec_in, T* spec_out, const T* src, T* dst, const T* norm, const T* scale, int ny, int nx,
                 int pitch, int V, int gy, int sub_one, int in_mod, unsigned long long* unresolved) {
    auto tw = twiddles_of<typename CfgFor<L>::Cfg, T>();
    return LongRow<L, T>::row(mode, params<L, T>(spec_in, spec_out, src, dst, norm, scale, tw.data(), ny, nx, pitch, V, gy, in_mod, sub_one, unresolved), gy);
}
template <int L, typename T>
static int pair_t(int mode, const T* spec_in, T* spec_out, const T* src, T* dst, const T* norm, int ny, int nx, int pitch, int V,
                  int frames, int in_mod, int sub_one, int special, unsigned long long* unresolved) {
    auto tw = twiddles_of<typename CfgFor<L>::Cfg, T>();
    const int gy = ((frames + 1) / 2) * (mode == ROW_RATIO ? V : 1);   // ROW_RATIO of a multi-view plan: one image per (pair, view)
    return LongRow<L, T>::pair(mode, params<L, T>(spec_in, spec_out, src, dst, norm, nullptr, tw.data(), ny, nx, pitch, V, frames, in_mod, sub_one, unresolved), gy, special);
}

#define DISPATCH_LONG(L, call)                                 \
    switch (L) {                                               \
        case 1152: { constexpr int LL = 1152; return call; }   \
        case 2304: { constexpr int LL = 2304; return call; }   \
        case 4608: { constexpr int LL = 4608; return call; }   \
        default: return -2;                                    \
    }

extern "C" {

int emu_long_row_f64(int L, int mode, const double* spec_in, double* spec_out, const double* src, double* dst, const double* norm,
                     const double* scale, int ny, int nx, int pitch, int V, int gy, int sub_one, int in_mod, unsigned long long* unresolved) {
    DISPATCH_LONG(L, (row_t<LL, double>(mode, spec_in, spec_out, src, dst, norm, scale, ny, nx, pitch, V, gy, sub_one, in_mod, unresolved)))
}
int emu_long_row_f32(int L, int mode, const float* spec_in, float* spec_out, const float* src, float* dst, const float* norm,
                     const float* scale, int ny, int nx, int pitch, int V, int gy, int sub_one, int in_mod, unsigned long long* unresolved) {
    DISPATCH_LONG(L, (row_t<LL, float>(mode, spec_in, spec_out, src, dst, norm, scale, ny, nx, pitch, V, gy, sub_one, in_mod, unresolved)))
}
// spectra [pairs (x V)][ny][pitch] complex, pitch >= L (the plan: L + 32); frames: images covered by the launch
int emu_long_row_pair_f64(int L, int mode, const double* spec_in, double* spec_out, const double* src, double* dst, const double* norm,
                          int ny, int nx, int pitch, int V, int frames, int in_mod, int sub_one, int special, unsigned long long* unresolved) {
    DISPATCH_LONG(L, (pair_t<LL, double>(mode, spec_in, spec_out, src, dst, norm, ny, nx, pitch, V, frames, in_mod, sub_one, special, unresolved)))
}
int emu_long_row_pair_f32(int L, int mode, const float* spec_in, float* spec_out, const float* src, float* dst, const float* norm,
                          int ny, int nx, int pitch, int V, int frames, int in_mod, int sub_one, int special, unsigned long long* unresolved) {
    DISPATCH_LONG(L, (pair_t<LL, float>(mode, spec_in, spec_out, src, dst, norm, ny, nx, pitch, V, frames, in_mod, sub_one, special, unresolved)))
}
// geometry of a length's row kernels: threads per transform, radix list (up to 4 entries), LDS slots of a transform
int emu_long_geometry(int L, int* T, int* radices, int* np, int* lds_slots) {
#define GEO(LL) case LL: { using C = CfgFor<LL>::Cfg; *T = C::T; *np = C::NP; for (int i = 0; i < C::NP; ++i) radices[i] = C::radix(i); *lds_slots = LdsSlots<C>::value; return 0; }
    switch (L) { GEO(1152) GEO(2304) GEO(4608) }
#undef GEO
    return -2;
}
// row pairs (rows, pair != 0) per workgroup of a length's row (frame-pair) kernels
int emu_long_q(int L, int esize, int pair) {
#define QOF(LL) case LL: return esize == 4 ? (pair ? LongRow<LL, float>::QP : LongRow<LL, float>::Q) : (pair ? LongRow<LL, double>::QP : LongRow<LL, double>::Q);
    switch (L) { QOF(1152) QOF(2304) QOF(4608) }
#undef QOF
    return -2;
}
// every instantiation this library can run, one per line; returns the length of the text (truncated to cap - 1)
int emu_long_table(char* buf, int cap) {
    std::string s;
    list_variants<1152, float, DeviceSpecial<1152, float>>(s, false, true); list_variants<1152, double, DeviceSpecial<1152, double>>(s, false, true);
    list_variants<2304, float, DeviceSpecial<2304, float>>(s, false, true); list_variants<2304, double, DeviceSpecial<2304, double>>(s, false, true);
    list_variants<4608, float, DeviceSpecial<4608, float>>(s, false, true); list_variants<4608, double, DeviceSpecial<4608, double>>(s, false, true);
    return copy_out(s, buf, cap);
}

}  // extern "C"

// ---- the device's side of kernel_variants.hpp, for any of its seven lengths: no body runs here
#define DISPATCH_ANY(L, call)                                                                                        \
    switch (L) {                                                                                                     \
        case 64: { constexpr int LL = 64; return call; }     case 192: { constexpr int LL = 192; return call; }      \
        case 256: { constexpr int LL = 256; return call; }   case 576: { constexpr int LL = 576; return call; }      \
        case 1152: { constexpr int LL = 1152; return call; } case 2304: { constexpr int LL = 2304; return call; }    \
        case 4608: { constexpr int LL = 4608; return call; } default: return -2;                                     \
    }
template <int L, typename T>
static int device_table(char* buf, int cap) {
    std::string s;
    list_variants<L, T, DeviceSpecial<L, T>>(s, true, true);
    return copy_out(s, buf, cap);
}
// family 0: the column pass (launch_col), 1: k_rowpass, 2: k_rowpair.  n: the image's rows (columns) or pixels per row (rows);
// flag: ColParams::residual or RowParams::sub_one.  Writes the line of the row the device's launcher would take; -1: none.
template <int L, typename T>
static int device_select(int family, int mode, int n, int V, int pitch, int realp, int flag, char* buf, int cap) {
    using S = DeviceSpecial<L, T>;
    using CF = CfgFor<L>;
    std::string s;
    if (family == 0 && kOuterCol<L, T>) {
        OuterKey k;
        if (!select_outer<L>(sizeof(T) == 4, S::outer_ny, mode, n, pitch, realp != 0, k)) return -1;
        s = line_of<L, T>(k);
    } else if (family == 0) {
        ColKey k;
        constexpr int C = sizeof(T) == 4 ? CF::C32 : CF::C64;
        if (!select_colconv(WavePrivate<typename ColCfgFor<L>::type>::value, S::col_ny, mode, n, V, pitch % C == 0, realp != 0, flag != 0, k)) return -1;
        s = line_of<L, T>(k);
    } else if (family == 1) {
        RowKey k;
        if (!select_rowpass(S::row_nx, mode, n, V, flag != 0, k)) return -1;
        s = line_of<L, T>(k);
    } else {
        PairKey k;
        if (!kPairRows<L> || !select_rowpair(S::pair_nx, mode, n, V, flag != 0, k)) return -1;
        s = line_of<L, T>(k);
    }
    return copy_out(s, buf, cap);
}
extern "C" {
int emu_device_table(int L, int esize, char* buf, int cap) {
    DISPATCH_ANY(L, (esize == 4 ? device_table<LL, float>(buf, cap) : device_table<LL, double>(buf, cap)))
}
int emu_device_select(int L, int esize, int family, int mode, int n, int V, int pitch, int realp, int flag, char* buf, int cap) {
    DISPATCH_ANY(L, (esize == 4 ? device_select<LL, float>(family, mode, n, V, pitch, realp, flag, buf, cap)
                                : device_select<LL, double>(family, mode, n, V, pitch, realp, flag, buf, cap)))
}

}  // extern "C"
