// kernel_variants.hpp -- the ONLY statement of which instantiations of k_colconv, k_colconv_outer, k_rowpass, k_rowpair and
// k_xcorr exist and of which one a launch gets.  Free of HIP: fft_kernels.hip launches and prepares through it, the host emulators
// (tests/emu) run and list their bodies through it.  Per family:
//   - a list, one row per instantiation, with the condition under which the row exists for a length and type;
//   - a tag type per row and for_each_<family>(f), the walk every reader uses: f(tag) for each row that exists, until f
//     returns true;
//   - select_<family>(): the run-time rule, a plain function of the launch parameters that returns the row's key.
// The image sizes some rows are compiled for are a parameter (a `Special` class for the walks, plain ints for the
// selectors; 0 = no such rows): DeviceSpecial below holds the product's, the emulators pass smaller ones or switch them off.
// To add a variant: add its row, make the selector return its key, and give the kernel's body the template argument.
#pragma once
#include <type_traits>
#include "conv_kernels.hpp"
#include "fft_configs.hpp"

// kernels with an image size at compile time (0: none anywhere)
#ifndef RL_N512
#define RL_N512 1
#endif

namespace rl {

// The product's compile-time sizes: the 512 x 512 frames of the BASELINE headline (L = 576, f32) in the column, row and
// frame-pair kernels; 2048-pixel rows in the frame-pair kernels of L = 2304, f32 (register slots of 256 pixels: 8 of 9 hold
// pixels); M x 512 rows -- the 1024 / 2048 / 4096-row images whose residue classes are the 512-of-576 case of the core -- in
// the outer-decimation column kernels.
template <int L, typename T>
struct DeviceSpecial {
    static constexpr bool N512 = RL_N512 != 0 && L == 576 && sizeof(T) == 4;
    static constexpr int col_ny = N512 ? 512 : 0, row_nx = N512 ? 512 : 0;
    static constexpr int pair_nx = N512 ? 512 : (RL_N512 != 0 && L == 2304 && sizeof(T) == 4) ? 2048 : 0;
    static constexpr int outer_ny = RL_N512 != 0 ? 512 * OuterCol<L>::M : 0;
};

// frame-pair row kernels exist for one transform per wave and for one workgroup-synchronous transform per workgroup
template <int L>
constexpr bool kPairRows = WavePrivate<typename CfgFor<L>::Cfg>::value || (CfgFor<L>::Q32 == 1 && CfgFor<L>::Q64 == 1);

// ---------------------------------------------------------------------------------------------- k_colconv
// WP: the column geometry is wave-private; NY: Special::col_ny (conv_kernels.hpp colconv_wave_body NYC / CT)
//    MODE           REALP  NYC CT  exists
#define RL_COLCONV_VARIANTS(X)                                  \
    X(COL_PER_IMAGE, false, 0,  0,  true)                       \
    X(COL_PER_IMAGE, true,  0,  0,  WP)                         \
    X(COL_H_MULTI,   false, 0,  0,  WP)                         \
    X(COL_H_MULTI,   true,  0,  0,  WP)                         \
    X(COL_HT_SUM,    false, 0,  0,  WP)                         \
    X(COL_HT_SUM,    true,  0,  0,  WP)                         \
    X(COL_PER_IMAGE, false, NY, 0,  NY != 0)                    \
    X(COL_PER_IMAGE, true,  NY, 0,  NY != 0)                    \
    X(COL_PER_IMAGE, false, NY, 1,  NY != 0 && RL_CT_RESIDUAL)  \
    X(COL_PER_IMAGE, true,  NY, 1,  NY != 0 && RL_CT_RESIDUAL)  \
    X(COL_H_MULTI,   true,  NY, 0,  NY != 0)                    \
    X(COL_HT_SUM,    true,  NY, 0,  NY != 0)                    \
    X(COL_HT_SUM,    true,  NY, 1,  NY != 0 && RL_CT_RESIDUAL)

struct ColKey {
    int mode, realp, nyc, ct;
    constexpr bool operator==(const ColKey& o) const { return mode == o.mode && realp == o.realp && nyc == o.nyc && ct == o.ct; }
};
template <int MODE_, bool REALP_, int NYC_, int CT_>
struct ColVariant {
    static constexpr int MODE = MODE_, NYC = NYC_, CT = CT_;
    static constexpr bool REALP = REALP_;
    static constexpr ColKey key() { return {MODE, REALP, NYC, CT}; }
};
template <int L, class Special, class F>
bool for_each_colconv(F&& f) {
    constexpr bool WP = WavePrivate<typename ColCfgFor<L>::type>::value;
    constexpr int NY = WP ? Special::col_ny : 0;
#define X(MODE, REALP, NYC, CT, EXISTS) \
    if constexpr (EXISTS) { if (f(ColVariant<MODE, REALP, NYC, CT>{})) return true; }
    RL_COLCONV_VARIANTS(X)
#undef X
    return false;
}
// tiles: the pitch is a multiple of the tile width; ny_special rows exactly, one view (or a fused multi-view mode with a real
// multiplier: what the reference's PSFs run): the kernels with the row count at compile time, with compact twiddles where
// the spectrum is that of `ratio - 1`.  False: no kernel serves the request.
inline bool select_colconv(bool wp, int ny_special, int mode, int ny, int V, bool tiles, bool realp, bool residual, ColKey& k) {
    if (mode != COL_PER_IMAGE && !(wp && (mode == COL_H_MULTI || mode == COL_HT_SUM))) return false;
    const bool special = wp && ny_special != 0 && ny == ny_special && tiles;
    const int ct = residual && RL_CT_RESIDUAL ? 1 : 0;
    if (special && mode == COL_PER_IMAGE && V == 1) k = {mode, realp, ny_special, ct};
    else if (special && realp && mode != COL_PER_IMAGE) k = {mode, 1, ny_special, mode == COL_HT_SUM ? ct : 0};
    else k = {mode, wp && realp, 0, 0};
    return true;
}

// ---------------------------------------------------------------------------------------------- k_colconv_outer
// Long column transforms on the wave-private core (fft_configs.hpp OuterCol<L>).  WIDTH names the tile width in OuterCol<L>:
// CW the whole pass, C the split pass, C64 float64 (the whole pass only).  Every row exists twice: with the row count at run
// time (NYC = 0) and, where Special::outer_ny is set, with that row count at compile time.
//    WIDTH REALP  MODE               T
#define RL_OUTER_VARIANTS(X)                      \
    X(CW,   true,  COL_PER_IMAGE,     float)      \
    X(CW,   false, COL_PER_IMAGE,     float)      \
    X(C,    false, COL_SPLIT_FWD,     float)      \
    X(C,    true,  COL_SPLIT_INV,     float)      \
    X(C,    false, COL_SPLIT_INV,     float)      \
    X(C,    true,  COL_SPLIT_INV_SUM, float)      \
    X(C,    false, COL_SPLIT_INV_SUM, float)      \
    X(C64,  true,  COL_PER_IMAGE,     double)     \
    X(C64,  false, COL_PER_IMAGE,     double)

struct OuterKey {
    int c, realp, mode, nyc;
    constexpr bool operator==(const OuterKey& o) const { return c == o.c && realp == o.realp && mode == o.mode && nyc == o.nyc; }
};
template <int C_, bool REALP_, int MODE_, int NYC_>
struct OuterVariant {
    static constexpr int C = C_, MODE = MODE_, NYC = NYC_;
    static constexpr bool REALP = REALP_;
    static constexpr OuterKey key() { return {C, REALP, MODE, NYC}; }
};
template <int L, typename T>
constexpr bool kOuterCol = sizeof(T) == 4 ? OuterCol<L>::value : OuterCol<L>::value64;   // this type's column pass is the outer one
template <int L, typename T, class Special, class F>
bool for_each_outer(F&& f) {
    using OC = OuterCol<L>;
    constexpr int NY = Special::outer_ny;
#define X(WIDTH, REALP, MODE, TT)                                                       \
    if constexpr (kOuterCol<L, T> && std::is_same<T, TT>::value) {                      \
        if (f(OuterVariant<OC::WIDTH, REALP, MODE, 0>{})) return true;                  \
        if constexpr (NY != 0) { if (f(OuterVariant<OC::WIDTH, REALP, MODE, NY>{})) return true; } \
    }
    RL_OUTER_VARIANTS(X)
#undef X
    return false;
}
// ny_special rows and a pitch that is a multiple of the mode's tile width: the kernel with the row count at compile time
template <int L>
inline bool select_outer(bool f32, int ny_special, int mode, int ny, int pitch, bool realp, OuterKey& k) {
    using OC = OuterCol<L>;
    const bool split = f32 && (mode == COL_SPLIT_FWD || mode == COL_SPLIT_INV || mode == COL_SPLIT_INV_SUM);
    if (mode != COL_PER_IMAGE && !split) return false;
    const int c = !f32 ? OC::C64 : split ? OC::C : OC::CW;
    k = {c, realp && mode != COL_SPLIT_FWD, mode, ny_special != 0 && ny == ny_special && pitch % c == 0 ? ny_special : 0};
    return true;
}

// ---------------------------------------------------------------------------------------------- k_rowpass
// NX: Special::row_nx (the lean bodies with the row length at compile time and `ratio - 1` arithmetic: rowlean_body NXC / SUBC)
//    MODE        ONEV   PRESUM NXC SUBC exists
#define RL_ROWPASS_VARIANTS(X)                       \
    X(ROW_FWD,    false, false, 0,  -1,  true)       \
    X(ROW_INV,    false, false, 0,  -1,  true)       \
    X(ROW_RATIO,  false, false, 0,  -1,  true)       \
    X(ROW_UPDATE, false, false, 0,  -1,  true)       \
    X(ROW_UPDATE, true,  false, 0,  -1,  true)       \
    X(ROW_UPDATE, true,  true,  0,  -1,  true)       \
    X(ROW_ADJ,    false, false, 0,  -1,  true)       \
    X(ROW_ADJ,    true,  false, 0,  -1,  true)       \
    X(ROW_RATIO,  false, false, NX, 1,   NX != 0)    \
    X(ROW_UPDATE, true,  false, NX, 1,   NX != 0)

struct RowKey {
    int mode, onev, presum, nxc, subc;
    constexpr bool operator==(const RowKey& o) const { return mode == o.mode && onev == o.onev && presum == o.presum && nxc == o.nxc && subc == o.subc; }
};
template <int MODE_, bool ONEV_, bool PRESUM_, int NXC_, int SUBC_>
struct RowVariant {
    static constexpr int MODE = MODE_, NXC = NXC_, SUBC = SUBC_;
    static constexpr bool ONEV = ONEV_, PRESUM = PRESUM_;
    static constexpr RowKey key() { return {MODE, ONEV, PRESUM, NXC, SUBC}; }
};
template <int L, class Special, class F>
bool for_each_rowpass(F&& f) {
    constexpr int NX = WavePrivate<typename CfgFor<L>::Cfg>::value ? Special::row_nx : 0;
#define X(MODE, ONEV, PRESUM, NXC, SUBC, EXISTS) \
    if constexpr (EXISTS) { if (f(RowVariant<MODE, ONEV, PRESUM, NXC, SUBC>{})) return true; }
    RL_ROWPASS_VARIANTS(X)
#undef X
    return false;
}
inline bool select_rowpass(int nx_special, int mode, int nx, int V, bool sub_one, RowKey& k) {
    if (mode < ROW_FWD || mode > ROW_ADJ) return false;
    const bool multi = mode == ROW_UPDATE || mode == ROW_ADJ;
    // the views' residual spectra are summed on their way in: one inverse transform (rowpass_body PRESUM)
    if (mode == ROW_UPDATE && V > 1 && sub_one) k = {mode, 1, 1, 0, -1};
    // per-frame lean bodies on nx_special-pixel rows: multi-view plans' RATIO, the single-spectrum UPDATE behind the column view sum
    else if (nx_special != 0 && nx == nx_special && sub_one && (mode == ROW_RATIO || (mode == ROW_UPDATE && V == 1))) k = {mode, mode == ROW_UPDATE, 0, nx_special, 1};
    else k = {mode, multi && V == 1, 0, 0, -1};   // single view: the variant without accumulator registers
    return true;
}
// single-view RL modes of the wave-private lengths: the lean item code (scalar row bases, unconditional loads).  RATIO treats
// every (frame, view) image on its own, so it always qualifies.
template <class KCfg, int MODE, bool ONEV, bool PRESUM>
constexpr bool kRowLean = !PRESUM && WavePrivate<KCfg>::value && (MODE == ROW_RATIO || (MODE == ROW_UPDATE && ONEV));

// ---------------------------------------------------------------------------------------------- k_rowpair
// frame-pair row kernels (rowpair_body); NX: Special::pair_nx
//    MODE        NXC SUBC exists
#define RL_ROWPAIR_VARIANTS(X)               \
    X(ROW_FWD,    0,  -1,  PAIRS)            \
    X(ROW_RATIO,  0,  -1,  PAIRS)            \
    X(ROW_UPDATE, 0,  -1,  PAIRS)            \
    X(ROW_RATIO,  NX, 1,   PAIRS && NX != 0) \
    X(ROW_UPDATE, NX, 1,   PAIRS && NX != 0)

struct PairKey {
    int mode, nxc, subc;
    constexpr bool operator==(const PairKey& o) const { return mode == o.mode && nxc == o.nxc && subc == o.subc; }
};
template <int MODE_, int NXC_, int SUBC_>
struct PairVariant {
    static constexpr int MODE = MODE_, NXC = NXC_, SUBC = SUBC_;
    static constexpr PairKey key() { return {MODE, NXC, SUBC}; }
};
template <int L, class Special, class F>
bool for_each_rowpair(F&& f) {
    constexpr bool PAIRS = kPairRows<L>;
    constexpr int NX = Special::pair_nx;
#define X(MODE, NXC, SUBC, EXISTS) \
    if constexpr (EXISTS) { if (f(PairVariant<MODE, NXC, SUBC>{})) return true; }
    RL_ROWPAIR_VARIANTS(X)
#undef X
    return false;
}
// nx_special-pixel rows, one view, `ratio - 1`: the specialised kernels (rowpair_body NXC / SUBC)
inline bool select_rowpair(int nx_special, int mode, int nx, int V, bool sub_one, PairKey& k) {
    if (mode != ROW_FWD && mode != ROW_RATIO && mode != ROW_UPDATE) return false;
    if (nx_special != 0 && nx == nx_special && V == 1 && sub_one && mode != ROW_FWD) k = {mode, nx_special, 1};
    else k = {mode, 0, -1};
    return true;
}

// ---------------------------------------------------------------------------------------------- k_xcorr
// The transform kernels of the coarse registration stage (xcorr_kernels.hpp: XC_ROW = 0, XC_COL = 1, XC_INV = 2), f32 only, on
// the row geometry CfgFor<L>::Cfg.  One row per (length, stage); the lengths whose column pass has a geometry of its own
// (ColCfgFor<2304>, ColCfgFor<4608>) have no rows: rl_register_xcorr refuses them.
#define RL_XCORR_LENGTHS(X) X(64) X(192) X(256) X(576) X(1152)

struct XcKey {
    int L, stage;
    constexpr bool operator==(const XcKey& o) const { return L == o.L && stage == o.stage; }
};
template <int L_, int STAGE_>
struct XcVariant {
    static constexpr int L = L_, STAGE = STAGE_;
    static constexpr XcKey key() { return {L, STAGE}; }
};
template <class F>
bool for_each_xcorr(F&& f) {
#define X(LEN)                                   \
    if (f(XcVariant<LEN, 0>{})) return true;     \
    if (f(XcVariant<LEN, 1>{})) return true;     \
    if (f(XcVariant<LEN, 2>{})) return true;
    RL_XCORR_LENGTHS(X)
#undef X
    return false;
}
// the smallest length with a row that holds n samples (n = image side + search radius); 0: none
inline int select_xcorr(long long n) {
#define X(LEN) \
    if (n <= LEN) return LEN;
    RL_XCORR_LENGTHS(X)
#undef X
    return 0;
}

}  // namespace rl
