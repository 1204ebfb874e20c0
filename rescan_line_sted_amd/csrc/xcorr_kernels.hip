// xcorr_kernels.hip -- the gfx950 kernels of rl_register_xcorr (bodies, the work split, the LDS layout and the order of every sum:
// xcorr_kernels.hpp; which instantiations exist: kernel_variants.hpp RL_XCORR_LENGTHS).
//   k_xcorr_stats           a workgroup per (pair, image): mean and centred energy in float64, fixed order
//   k_xcorr<L, XC_ROW>      z = a + i b, forward transform of length Lx = L per image row
//   k_xcorr<L, XC_COL>      columns (kx, Lx - kx): forward transforms of length Ly = L, un-mix, conj(A) B, inverse, rows |dy| <= R kept
//   k_xcorr<L, XC_INV>      inverse transform of length Lx = L per kept row, columns |dx| <= R kept
//   k_xcorr_peak            a workgroup per pair: overlap normalisation, optional surface, peak and window sums in a fixed order
// Five launches per chunk of pairs, no atomics anywhere.
#include <hip/hip_runtime.h>
#include "dev_sync.hpp"
#include "kernel_variants.hpp"
#include "xcorr_kernels.hpp"

namespace rl {

__global__ __launch_bounds__(kXcThreads) void k_xcorr_stats(XcArgs p) {
    __shared__ double sm[kXcThreads];
    DevSync sync;
    xc_stats_body(p, (int)threadIdx.x, (long long)blockIdx.x, sm, sync);
}

template <int L, int STAGE>
__global__ __launch_bounds__(XcGroup<typename CfgFor<L>::Cfg>::THREADS) void k_xcorr(XcArgs p) {
    extern __shared__ double xc_lds[];
    using Cfg = typename CfgFor<L>::Cfg;
    DevSync sync;
    cx<float>* lds = reinterpret_cast<cx<float>*>(xc_lds);
    if constexpr (STAGE == XC_ROW) xc_row_body<Cfg>(p, (int)threadIdx.x, (long long)blockIdx.x, lds, sync);
    else if constexpr (STAGE == XC_COL) xc_col_body<Cfg>(p, (int)threadIdx.x, (long long)blockIdx.x, lds, sync);
    else xc_inv_body<Cfg>(p, (int)threadIdx.x, (long long)blockIdx.x, lds, sync);
}

__global__ __launch_bounds__(kXcThreads) void k_xcorr_peak(XcArgs p) {
    extern __shared__ double xc_peak_lds[];
    DevSync sync;
    xc_peak_body(p, (int)threadIdx.x, (long long)blockIdx.x, xc_peak_lds, sync);
}

namespace {
constexpr long long kMaxGrid = 0x7fffffffll;

// the row of the variant table for (L, stage); hipErrorInvalidValue: there is none
hipError_t launch_stage(int L, int stage, const XcArgs& a, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;
    for_each_xcorr([&](auto v) {
        using V = decltype(v);
        if (!(V::key() == XcKey{L, stage})) return false;
        using Cfg = typename CfgFor<V::L>::Cfg;
        const long long blocks = xc_blocks<Cfg>(a, V::STAGE);
        const size_t lds = xc_lds_bytes<Cfg>(V::STAGE);
        if (blocks < 1 || blocks > kMaxGrid || lds > 65536) return true;
        hipLaunchKernelGGL((k_xcorr<V::L, V::STAGE>), dim3((unsigned)blocks), dim3(XcGroup<Cfg>::THREADS), lds, s, a);
        e = hipGetLastError();
        return true;
    });
    return e;
}
}  // namespace

hipError_t xcorr_pairs(const XcArgs& a, hipStream_t s) {
    if (a.pairs <= 0) return hipSuccess;
    if (2LL * a.pairs > kMaxGrid || xc_peak_lds_bytes(a.R) > 65536) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_xcorr_stats, dim3(2u * (unsigned)a.pairs), dim3(kXcThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_stage(a.Lx, XC_ROW, a, s)) != hipSuccess) return e;
    if ((e = launch_stage(a.Ly, XC_COL, a, s)) != hipSuccess) return e;
    if ((e = launch_stage(a.Lx, XC_INV, a, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_xcorr_peak, dim3((unsigned)a.pairs), dim3(kXcThreads), xc_peak_lds_bytes(a.R), s, a);
    return hipGetLastError();
}

}  // namespace rl
