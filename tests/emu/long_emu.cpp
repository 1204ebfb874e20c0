// Host emulator of the ROW kernels of the long, workgroup-synchronous lengths (L = 1152, 2304, 4608): rowpass_body in every
// mode and rowpair_body on the `Q == 1` branch of k_rowpair, instantiated and dispatched as fft_kernels.hip does it
// (launch_row_m, launch_row_pair_t).  A translation unit of its own -- tests/test_long_rows_cpu.py builds it into
// liblong_emu.so -- so that libemu.so keeps its build time.  TEST INFRASTRUCTURE ONLY.
//
// The instantiations are listed ONCE, in the LONG_ROWPASS / LONG_ROWPAIR tables below: the dispatch runs through them and
// emu_long_table() prints them, so the test that compares the list with what fft_kernels.hip can launch sees exactly what
// can run here.
#include <cstdio>
#include <string>

#include "emu_common.hpp"

//            MODE        ONEV   PRESUM
#define LONG_ROWPASS(X)           \
    X(ROW_FWD,    false, false)   \
    X(ROW_INV,    false, false)   \
    X(ROW_RATIO,  false, false)   \
    X(ROW_UPDATE, false, false)   \
    X(ROW_UPDATE, true,  false)   \
    X(ROW_UPDATE, true,  true)    \
    X(ROW_ADJ,    false, false)   \
    X(ROW_ADJ,    true,  false)
//            MODE        NXC   SUBC     (NXC > 0: float, L = 2304 only -- fft_kernels.hip kRowN2048)
#define LONG_ROWPAIR(X)        \
    X(ROW_FWD,    0,    -1)    \
    X(ROW_RATIO,  0,    -1)    \
    X(ROW_UPDATE, 0,    -1)    \
    X(ROW_RATIO,  2048, 1)     \
    X(ROW_UPDATE, 2048, 1)

template <int L, typename T>
constexpr bool pair_inst_exists(int nxc) {
    return nxc == 0 || (L == 2304 && sizeof(T) == 4);
}

template <int L, typename T>
struct LongRow {
    using CF = CfgFor<L>;
    using Cfg = typename CF::Cfg;
    static constexpr int Q = sizeof(T) == 4 ? CF::Q32 : CF::Q64;
    // fft_kernels.hip: kPairQ32 = WavePrivate ? RL_PAIR_Q32 : kQ32; pairs exist where WavePrivate || (Q32 == 1 && Q64 == 1)
    static constexpr int QP = Q;
    static_assert(!WavePrivate<Cfg>::value, "the wave-private lengths are emu.cpp's");
    static constexpr bool kPairRows = CF::Q32 == 1 && CF::Q64 == 1;
    static constexpr size_t lds_bytes(int q) { return (size_t)q * LdsSlots<Cfg>::value * sizeof(cx<T>); }

    template <int MODE, bool ONEV, bool PRESUM>
    static int rowpass(const RowParams<T>& p, int gy) {
        const int pairs = (p.ny + 1) / 2;
        run_grid((pairs + Q - 1) / Q, gy, Cfg::T * Q, lds_bytes(Q), [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
            rowpass_body<Cfg, Q, MODE, ONEV, T, PRESUM>(p, tid, bx, by, reinterpret_cast<cx<T>*>(lds), s);
        });
        return 0;
    }
    static int rowpass_inst(int mode, bool onev, bool presum, const RowParams<T>& p, int gy) {
#define X(M, O, P) if (mode == M && onev == O && presum == P) return rowpass<M, O, P>(p, gy);
        LONG_ROWPASS(X)
#undef X
        return -4;   // launch_row_m would launch an instantiation this emulator does not have
    }
    // the choice of launch_row_m
    static int row(int mode, const RowParams<T>& p, int gy) {
        const bool multi = mode == ROW_UPDATE || mode == ROW_ADJ;
        if (mode == ROW_UPDATE && p.V > 1 && p.sub_one) return rowpass_inst(mode, true, true, p, gy);
        return rowpass_inst(mode, multi && p.V == 1, false, p, gy);
    }

    template <int MODE, int NXC, int SUBC>
    static int rowpair(const RowParams<T>& p, int gy) {
        if constexpr (kPairRows && pair_inst_exists<L, T>(NXC)) {
            static_assert(QP == 1, "k_rowpair: WavePrivate || Q == 1");
            run_grid((p.ny + QP - 1) / QP, gy, Cfg::T * QP, lds_bytes(QP), [&](int tid, int bx, int by, unsigned char* lds, EmuSync& s) {
                rowpair_body<Cfg, QP, MODE, T, NXC, SUBC>(p, tid, bx, by, reinterpret_cast<cx<T>*>(lds), s);
            });
            return 0;
        } else {
            return -3;
        }
    }
    static int rowpair_inst(int mode, int nxc, int subc, const RowParams<T>& p, int gy) {
#define X(M, N, S) if (mode == M && nxc == N && subc == S) return rowpair<M, N, S>(p, gy);
        LONG_ROWPAIR(X)
#undef X
        return -4;
    }
    // the choice of launch_row_pair_t; special == 0: the run-time-size bodies whatever the size (what the others are compared with)
    static int pair(int mode, const RowParams<T>& p, int gy, int special) {
        if (special && pair_inst_exists<L, T>(2048) && p.nx == 2048 && p.V == 1 && p.sub_one != 0 && mode != ROW_FWD)
            return rowpair_inst(mode, 2048, 1, p, gy);
        return rowpair_inst(mode, 0, -1, p, gy);
    }

    static void table(std::string& out) {
        char b[160];
        const char* t = sizeof(T) == 4 ? "f32" : "f64";
#define X(M, O, P) std::snprintf(b, sizeof b, "k_rowpass L=%d T=%s MODE=%d ONEV=%d PRESUM=%d NXC=0 SUBC=-1\n", L, t, (int)M, (int)O, (int)P); out += b;
        LONG_ROWPASS(X)
#undef X
#define X(M, N, S) if (kPairRows && pair_inst_exists<L, T>(N)) { std::snprintf(b, sizeof b, "k_rowpair L=%d T=%s MODE=%d NXC=%d SUBC=%d\n", L, t, (int)M, (int)N, (int)S); out += b; }
        LONG_ROWPAIR(X)
#undef X
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
    LongRow<1152, float>::table(s); LongRow<1152, double>::table(s);
    LongRow<2304, float>::table(s); LongRow<2304, double>::table(s);
    LongRow<4608, float>::table(s); LongRow<4608, double>::table(s);
    std::snprintf(buf, (size_t)cap, "%s", s.c_str());
    return (int)s.size();
}

}  // extern "C"
