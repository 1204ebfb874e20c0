// fft_kernels.hip -- gfx950 kernels for one FFT length (compile with
// -DRL_CFG_L=<L>).  Column pass (FFT_y * psf_hat -> IFFT_y) and the fused row
// passes (IFFT_x -> Richardson-Lucy pointwise step -> FFT_x) of the
// convolution path; bodies in conv_kernels.hpp.
#include <hip/hip_ext.h>
#include "kernel_table.hpp"
#include "kernel_variants.hpp"
#include "outer_lds.hpp"
#include "dev_sync.hpp"

// waves/SIMD requested for the f32 ROW_RATIO kernel (needs <= 96 VGPRs, which it has
// within 2 registers; the other modes spill under that bound and are left alone)
#ifndef RL_ROW_MIN_WAVES
#define RL_ROW_MIN_WAVES 5
#endif
#ifndef RL_UPD_MIN_WAVES
#define RL_UPD_MIN_WAVES 1
#endif
// (waves per SIMD requested for the long row kernels: 6 / 5 for RATIO / UPDATE -- five or six workgroups per CU instead of four --
// measured 2048^2 point 781 -> 712 frames/s, 4 views 247 -> 216: left to the compiler)
// waves/SIMD requested for the f32 per-image column kernel: 6 = three 8-wave workgroups per CU
// (80 VGPRs, no spills; 3 x 51 KB LDS), whose load / transform / store phases overlap better than
// two (+1.7 % end to end).  The multi-view modes spill under that bound and keep 1.
#ifndef RL_COL_MIN_WAVES
#define RL_COL_MIN_WAVES 6
#endif
#ifndef RL_CFG_L
#error "compile with -DRL_CFG_L=<length>"
#endif

namespace rl {

// Every kernel of this file is launched through here.  When the caller has armed a pair of timing
// events (kernel_table.hpp: launch_timing), the launch records the kernel's own begin and end on
// them -- the interval a rocprofv3 kernel trace reports -- instead of stream-order timestamps.
template <typename K, typename P>
static void rl_launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, P p) {
    LaunchTiming& t = launch_timing();
    if (t.start && t.stop) {
        hipExtLaunchKernelGGL(kernel, grid, block, (unsigned)lds, s, t.start, t.stop, 0, p);
        t.start = t.stop = nullptr;   // one launch per arming
    } else {
        hipLaunchKernelGGL(kernel, grid, block, (unsigned)lds, s, p);
    }
}

template <typename F>
static hipError_t allow_lds(F* fn, size_t bytes) {
    if (bytes <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}


using CF = CfgFor<RL_CFG_L>;
using Cfg = CF::Cfg;                               // row kernels
using CCfg = ColCfgFor<RL_CFG_L>::type;            // column kernels
constexpr int kC32 = CF::C32, kC64 = CF::C64, kQ32 = CF::Q32, kQ64 = CF::Q64;
#define RL_CAT_(a, b) a##b
#define RL_CAT(a, b) RL_CAT_(a, b)
#define RL_TABLE_FN RL_CAT(table_, RL_CFG_L)

template <typename T>
using Special = DeviceSpecial<RL_CFG_L, T>;   // the image sizes some variants are compiled for (kernel_variants.hpp)

// NOTE: the transform length is a template parameter of the kernels so that the
// kernels of different lengths (built in separate translation units) have
// distinct symbol names.
template <int L, int C, int MODE, typename T, bool REALP = false, int NYC = 0, int CT = 0>
__global__ void __launch_bounds__(ColCfgFor<L>::type::T* C, (sizeof(T) == 4 && MODE == COL_PER_IMAGE && WavePrivate<typename ColCfgFor<L>::type>::value) ? RL_COL_MIN_WAVES : 1)
    k_colconv(const ColParams<T> p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    DevSync s;
    using KCfg = typename ColCfgFor<L>::type;
    // XCD-aware work order (pure speed heuristic -- any placement is correct).  Workgroups are dealt
    // round-robin over the 8 XCDs, so linear ids l and l+8 share an L2; every XCD gets a contiguous
    // range of the item sequence.  The images of the launch are taken in blocks of G = p.order:
    //     for image block:  for tile pair:  for image in block:  for the two tiles of the pair
    // G = 1 is image-major (tile after tile of one image): concurrent workgroups touch neighbouring
    // 64-B segments of the same spectrum rows.  Larger G re-uses the psf_hat columns of a tile pair
    // for G images in a row: image-major streams the whole 1.33 MB psf_hat through every XCD once
    // per image, past ~3.7 MB of tile traffic in a 4 MiB L2 (half of it is fetched again).
    // G >= images is tile-major: psf_hat stays resident but concurrent workgroups scatter 64-B
    // accesses over all images.
    unsigned bx = blockIdx.x, by = blockIdx.y;
    const unsigned gx = gridDim.x, gy = gridDim.y, total = gx * gy;
    if (total % 8 == 0) {
        const unsigned lin = by * gx + bx;
        const unsigned w = (lin % 8) * (total / 8) + lin / 8;
        // images in blocks of G = p.order: within a block, for tile pair: for image: the two tiles
        const unsigned G = p.order < 1 ? 1u : (unsigned)p.order;
        const unsigned blk = w / (gx * G), first = blk * G;
        const unsigned g = gy - first < G ? gy - first : G;          // images in this block
        const unsigned v = w - blk * gx * G;
        const unsigned paired = (gx & ~1u) * g;                       // items of full tile pairs
        if (v < paired) {
            const unsigned pr = v / (2 * g), q = v % (2 * g);
            bx = 2 * pr + (q & 1u);
            by = first + (q >> 1);
        } else {
            bx = gx - 1;
            by = first + (v - paired);
        }
    }
    if constexpr (WavePrivate<KCfg>::value)
        colconv_wave_body<KCfg, C, MODE, T, REALP, NYC, CT>(p, (int)threadIdx.x, (int)bx, (int)by, reinterpret_cast<cx<T>*>(smem), s);
    else
        colconv_body<KCfg, C, T>(p, (int)threadIdx.x, (int)bx, (int)by, reinterpret_cast<cx<T>*>(smem), s);
}

// ---- long column transforms on the wave-private core (conv_kernels.hpp colconv_outer_body) ----
// L = 2304 = 4 x 576 and 4608 = 8 x 576, f32: fft_configs.hpp OuterCol<L>.  The f64 kernels of these lengths stay
// the workgroup-synchronous ones (4 x 9 complex doubles per lane would not fit the register file).
// (LDS byte counts of these kernels: outer_lds.hpp, shared with the host emulator)
// NYC: the image's row count at compile time (conv_kernels.hpp colconv_outer_body): instantiated for M x 512 rows -- the
// 1024 / 2048 / 4096-row images whose residue classes are the 512-of-576 case of the core
template <int L, int C, bool REALP, int MODE = COL_PER_IMAGE, typename T = float, int NYC = 0>
__global__ void __launch_bounds__(64 * C, (sizeof(T) == 4 ? OuterCol<L>::MIN_WAVES : OuterCol<L>::MIN_WAVES64)) k_colconv_outer(const ColParams<T> p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    DevSync s;
    using OC = OuterCol<L>;
    static_assert(sizeof(T) == 4 || MODE == COL_PER_IMAGE, "float64: the whole pass only");
    unsigned bx = blockIdx.x, by = blockIdx.y;
    const unsigned gx = gridDim.x, gy = gridDim.y, total = gridDim.x * gridDim.y;
    if (total % 8 == 0) {   // XCD-contiguous work order (speed only)
        const unsigned lin = by * gx + bx;
        const unsigned w = (lin % 8) * (total / 8) + lin / 8;
        if constexpr (MODE == COL_SPLIT_INV || MODE == COL_SPLIT_INV_SUM) {
            // tile-major: the images of one column tile (views fastest, then frames) follow each other on one XCD, so the tile's
            // multipliers (and, COL_SPLIT_INV, the frame's parked spectra its V views share) are fetched once and then hit in L2
            bx = w / gy;
            by = w % gy;
        } else {   // image-major
            bx = w % gx;
            by = w / gx;
        }
    }
    if constexpr (sizeof(T) == 4)
        colconv_outer_body<typename OC::Core, OC::M, C, float, REALP, MODE, (MODE == COL_PER_IMAGE ? OC::PARK : 0), (MODE == COL_PER_IMAGE ? OC::TWLDS : OC::TWLDS_SPLIT), NYC>(
            p, (int)threadIdx.x, (int)bx, (int)by, reinterpret_cast<cx<float>*>(smem), s);
    else
        colconv_outer_body<typename OC::Core, OC::M, C, double, REALP, COL_PER_IMAGE, OC::PARK64, 0, NYC>(p, (int)threadIdx.x, (int)bx, (int)by, reinterpret_cast<cx<double>*>(smem), s);
}
template <int L>
static void fill_outer_twiddles(double* out) {
    using OC = OuterCol<L>;
    using Core = typename OC::Core;
    fill_pass_twiddles<Core>(out);
    double* dst = out + 2 * PassTw<Core, false, 0>::TOTAL;
    for (int q = 1; q < OC::M; ++q)
        for (int k = 0; k < Core::L; ++k) {
            const long double ang = -6.283185307179586476925286766559005768L * (long double)q * (long double)k / (long double)L;
            dst[2 * ((q - 1) * Core::L + k)] = (double)__builtin_cosl(ang);
            dst[2 * ((q - 1) * Core::L + k) + 1] = (double)__builtin_sinl(ang);
        }
}

// waves per SIMD requested from the register allocator (f32, wave-private lengths)
template <int L, int MODE, bool ONEV, typename T>
constexpr int row_min_waves() {
    if (sizeof(T) != 4 || !WavePrivate<typename CfgFor<L>::Cfg>::value) return 1;   // float64; the long lengths (256 threads per transform)
    if (MODE == ROW_RATIO) return RL_ROW_MIN_WAVES;
    if (MODE == ROW_UPDATE && ONEV) return RL_UPD_MIN_WAVES;
    return 1;
}

template <int L, int Q, int MODE, bool ONEV, typename T, bool PRESUM = false, int NXC = 0, int SUBC = -1>
__global__ void __launch_bounds__(CfgFor<L>::Cfg::T* Q, (row_min_waves<L, MODE, ONEV, T>()))
    k_rowpass(const RowParams<T> p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    DevSync s;
    using KCfg = typename CfgFor<L>::Cfg;
    // (An XCD-consistent remap of (image, row group) items like k_colconv's measured neutral on time and cost traffic -- every
    // XCD's L2 then streams the whole normaliser instead of the eighth its row groups touch: removed.)
    const unsigned bx = blockIdx.x, by = blockIdx.y;
    constexpr bool LEAN = kRowLean<KCfg, MODE, ONEV, PRESUM>;
    static_assert(NXC == 0 || LEAN, "the compile-time row length exists for the lean bodies");
    if constexpr (LEAN)
        rowlean_body<KCfg, Q, MODE, T, NXC, SUBC>(p, (int)threadIdx.x, (int)bx, (int)by, reinterpret_cast<cx<T>*>(smem), s);
    else
        rowpass_body<KCfg, Q, MODE, ONEV, T, PRESUM>(p, (int)threadIdx.x, (int)bx, (int)by, reinterpret_cast<cx<T>*>(smem), s);
}

template <int C, typename T>
static constexpr size_t lds_bytes() {
    return (size_t)C * LdsSlots<Cfg>::value * sizeof(cx<T>);
}
template <int C, typename T>
static constexpr size_t col_lds_bytes() {
    return (size_t)C * LdsSlots<CCfg>::value * sizeof(cx<T>);
}

// frame-pair row kernels (rowpair_body)
template <int L, int Q, int MODE, typename T, int NXC = 0, int SUBC = -1>
__global__ void __launch_bounds__(CfgFor<L>::Cfg::T * Q, (row_min_waves<L, MODE == ROW_FWD ? ROW_RATIO : MODE, true, T>())) k_rowpair(const RowParams<T> p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    DevSync s;
    using KCfg = typename CfgFor<L>::Cfg;
    if constexpr (WavePrivate<KCfg>::value || Q == 1)
        rowpair_body<KCfg, Q, MODE, T, NXC, SUBC>(p, (int)threadIdx.x, (int)blockIdx.x, (int)blockIdx.y, reinterpret_cast<cx<T>*>(smem), s);
}
// rows (= waves) per workgroup of the frame-pair row kernels, f32 (RL_PAIR_Q32; measured at 512^2: 2 / 4 / 8 / 16 rows
// 18.4 / 18.8 / 19.1 / ... k frames/s)
#ifndef RL_PAIR_Q32
#define RL_PAIR_Q32 8
#endif
constexpr int kPairQ32 = WavePrivate<Cfg>::value ? RL_PAIR_Q32 : kQ32;

// The launchers: the selector of kernel_variants.hpp names a variant, one walk over the family's list turns the name into
// the instantiation.  A request no variant serves is hipErrorInvalidValue.
template <int C, typename T>
static hipError_t launch_col_t(const void* params, unsigned gx, unsigned gy, hipStream_t s) {
    const ColParams<T>& p = *static_cast<const ColParams<T>*>(params);
    ColKey k;
    if (!select_colconv(WavePrivate<CCfg>::value, Special<T>::col_ny, p.mode, p.ny, p.V, p.pitch % C == 0, p.psf_hat_re != nullptr, p.residual != 0, k))
        return hipErrorInvalidValue;
    const bool found = for_each_colconv<RL_CFG_L, Special<T>>([&](auto v) {
        using V = decltype(v);
        if (!(V::key() == k)) return false;
        rl_launch(k_colconv<RL_CFG_L, C, V::MODE, T, V::REALP, V::NYC, V::CT>, dim3(gx, gy), dim3(CCfg::T * C), col_lds_bytes<C, T>(), s, p);
        return true;
    });
    return found ? hipGetLastError() : hipErrorInvalidValue;
}
template <typename T>
static hipError_t launch_outer_t(const void* params, unsigned gy, hipStream_t s) {
    const ColParams<T>& p = *static_cast<const ColParams<T>*>(params);
    OuterKey k;
    if (!select_outer<RL_CFG_L>(sizeof(T) == 4, Special<T>::outer_ny, p.mode, p.ny, p.pitch, p.psf_hat_re != nullptr, k)) return hipErrorInvalidValue;
    const bool found = for_each_outer<RL_CFG_L, T, Special<T>>([&](auto v) {
        using V = decltype(v);
        if (!(V::key() == k)) return false;
        rl_launch(k_colconv_outer<RL_CFG_L, V::C, V::REALP, V::MODE, T, V::NYC>, dim3((unsigned)((p.kx + V::C - 1) / V::C), gy), dim3(64 * V::C), outer_lds_bytes<OuterCol<RL_CFG_L>, T, V::MODE>(), s, p);
        return true;
    });
    return found ? hipGetLastError() : hipErrorInvalidValue;
}
template <int Q, typename T>
static hipError_t launch_row_t(int mode, const void* params, unsigned gx, unsigned gy, hipStream_t s) {
    const RowParams<T>& p = *static_cast<const RowParams<T>*>(params);
    RowKey k;
    if (!select_rowpass(Special<T>::row_nx, mode, p.nx, p.V, p.sub_one != 0, k)) return hipErrorInvalidValue;
    const bool found = for_each_rowpass<RL_CFG_L, Special<T>>([&](auto v) {
        using V = decltype(v);
        if (!(V::key() == k)) return false;
        rl_launch(k_rowpass<RL_CFG_L, Q, V::MODE, V::ONEV, T, V::PRESUM, V::NXC, V::SUBC>, dim3(gx, gy), dim3(Cfg::T * Q), lds_bytes<Q, T>(), s, p);
        return true;
    });
    return found ? hipGetLastError() : hipErrorInvalidValue;
}
template <int Q, typename T>
static hipError_t launch_row_pair_t(int mode, const void* params, unsigned gy, hipStream_t s) {
    const RowParams<T>& p = *static_cast<const RowParams<T>*>(params);
    PairKey k;
    if (!select_rowpair(Special<T>::pair_nx, mode, p.nx, p.V, p.sub_one != 0, k)) return hipErrorInvalidValue;
    const bool found = for_each_rowpair<RL_CFG_L, Special<T>>([&](auto v) {
        using V = decltype(v);
        if (!(V::key() == k)) return false;
        rl_launch(k_rowpair<RL_CFG_L, Q, V::MODE, T, V::NXC, V::SUBC>, dim3((unsigned)((p.ny + Q - 1) / Q), gy), dim3(Cfg::T * Q), lds_bytes<Q, T>(), s, p);
        return true;
    });
    return found ? hipGetLastError() : hipErrorInvalidValue;
}

// float64 column passes of the outer lengths run the outer-decimation body too (per image; multi-view plans launch it per view)
static hipError_t launch_col(int dtype, const void* params, unsigned gx, unsigned gy, hipStream_t s) {
    if (dtype == DT_F32) return kOuterCol<RL_CFG_L, float> ? launch_outer_t<float>(params, gy, s) : launch_col_t<kC32, float>(params, gx, gy, s);
    return kOuterCol<RL_CFG_L, double> ? launch_outer_t<double>(params, gy, s) : launch_col_t<kC64, double>(params, gx, gy, s);
}
static hipError_t launch_row(int dtype, int mode, const void* params, unsigned gx, unsigned gy, hipStream_t s) {
    return dtype == DT_F32 ? launch_row_t<kQ32, float>(mode, params, gx, gy, s)
                           : launch_row_t<kQ64, double>(mode, params, gx, gy, s);
}
static hipError_t launch_row_pair(int dtype, int mode, const void* params, unsigned gy, hipStream_t s) {
    return dtype == DT_F32 ? launch_row_pair_t<kPairQ32, float>(mode, params, gy, s)
                           : launch_row_pair_t<kQ64, double>(mode, params, gy, s);
}

// every variant that exists for this length and type may use its dynamic LDS: the walks the launchers take.  (Where the type's
// column pass is the outer one, launch_col never takes k_colconv: its one workgroup-synchronous instantiation is still walked
// here, as it always was prepared -- dropping that unreachable kernel is a change of the device code, left for its own commit.)
template <int C, int Q, int QP, typename T>
static hipError_t prepare_t() {
    hipError_t e = hipSuccess;
    auto failed = [&e](hipError_t r) { return (e = r) != hipSuccess; };
    (void)(for_each_colconv<RL_CFG_L, Special<T>>([&](auto v) {
        using V = decltype(v);
        return failed(allow_lds(k_colconv<RL_CFG_L, C, V::MODE, T, V::REALP, V::NYC, V::CT>, col_lds_bytes<C, T>()));
    }) || for_each_outer<RL_CFG_L, T, Special<T>>([&](auto v) {
        using V = decltype(v);
        static_assert(outer_lds_bytes<OuterCol<RL_CFG_L>, T, V::MODE>() <= 160 * 1024, "LDS of a CU");
        return failed(allow_lds(k_colconv_outer<RL_CFG_L, V::C, V::REALP, V::MODE, T, V::NYC>, outer_lds_bytes<OuterCol<RL_CFG_L>, T, V::MODE>()));
    }) || for_each_rowpass<RL_CFG_L, Special<T>>([&](auto v) {
        using V = decltype(v);
        return failed(allow_lds(k_rowpass<RL_CFG_L, Q, V::MODE, V::ONEV, T, V::PRESUM, V::NXC, V::SUBC>, lds_bytes<Q, T>()));
    }) || for_each_rowpair<RL_CFG_L, Special<T>>([&](auto v) {
        using V = decltype(v);
        return failed(allow_lds(k_rowpair<RL_CFG_L, QP, V::MODE, T, V::NXC, V::SUBC>, lds_bytes<QP, T>()));
    }));
    return e;
}
static hipError_t prepare() {
    const hipError_t e = prepare_t<kC32, kQ32, kPairQ32, float>();
    return e != hipSuccess ? e : prepare_t<kC64, kQ64, kQ64, double>();
}

// (the length is a template parameter: this file is compiled once per length, and equally named entities of
// different translation units would be merged by the linker)
template <int L, bool OUTER>
struct OuterTw {   // column twiddle table of the f32 kernel: the outer-decimation kernel's, where the length has one
    static constexpr int count = PassTw<typename ColCfgFor<L>::type, false, 0>::TOTAL;
    static void fill(double* out) { fill_pass_twiddles<typename ColCfgFor<L>::type>(out); }
    static constexpr size_t split_tile = 0;
};
template <int L>
struct OuterTw<L, true> {
    using OC = OuterCol<L>;
    static constexpr int count = PassTw<typename OC::Core, false, 0>::TOTAL + (OC::M - 1) * OC::Core::L;
    static void fill(double* out) { fill_outer_twiddles<L>(out); }
    static constexpr size_t split_tile = OC::SPLIT ? outer_slots_tile_elems<typename OC::Core, OC::M, OC::C>() : 0;
};

const KernelTable* RL_TABLE_FN() {
    constexpr bool OUTER = OuterCol<RL_CFG_L>::value;
    constexpr int WP = WavePrivate<CCfg>::value ? 1 : 0;
    constexpr bool OUTER64 = OuterCol<RL_CFG_L>::value64;   // float64 column pass on the outer-decimation body too
    static const KernelTable t = {Cfg::L, Cfg::T, {OUTER ? OuterCol<RL_CFG_L>::C : kC32, OUTER64 ? OuterCol<RL_CFG_L>::C64 : kC64}, {kQ32, kQ64},
                                  {OUTER ? 1 : WP, OUTER64 ? 1 : WP}, {OUTER ? 0 : 3 * WP, OUTER64 ? 0 : 3 * WP},
                                  PassTw<Cfg, false, 0>::TOTAL, fill_pass_twiddles<Cfg>,
                                  {OuterTw<RL_CFG_L, OUTER>::count, OUTER64 ? OuterTw<RL_CFG_L, OUTER64>::count : PassTw<CCfg, false, 0>::TOTAL},
                                  {OuterTw<RL_CFG_L, OUTER>::fill, OUTER64 ? OuterTw<RL_CFG_L, OUTER64>::fill : fill_pass_twiddles<CCfg>}, launch_col, launch_row, prepare,
                                  kPairRows<RL_CFG_L> ? launch_row_pair : nullptr, OuterTw<RL_CFG_L, OUTER>::split_tile};
    return &t;
}

}  // namespace rl
