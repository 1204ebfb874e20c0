// bead_kernels.hip -- the gfx950 kernels of rl_find_peaks (bodies, the work split, the LDS layout and the order of every operation:
// bead_kernels.hpp).
//   k_peaks_range     a workgroup per (image, tile): separable stencil in LDS, the tile's min / max of s over the domain
//   k_peaks_levels    a workgroup per image: lo, hi and the threshold t from the tiles' partials
//   k_peaks_mark      a workgroup per (image, tile): stencil with a halo of h + r, suppression, one mask word per tile row
//   k_peaks_compact   a workgroup per image: the mask's bits in row-major order, ranks from an integer prefix, the first cap written
// Four launches per chunk of images, no atomics anywhere.
#include <hip/hip_runtime.h>
#include "bead_kernels.hpp"

namespace rl {

__global__ __launch_bounds__(kBpThreads) void k_peaks_range(BpArgs p) {
    extern __shared__ double bp_range_lds[];
    const BpTile T = bp_tile(p, (long long)blockIdx.x, 0);
    double* U = bp_range_lds;
    double* S = bp_range_lds + T.UH * T.SW;
    const int t = (int)threadIdx.x;
    bp_row_body(p, T, t, U);
    __syncthreads();
    bp_col_body(p, T, t, U, S);
    __syncthreads();
    double *lo = U, *hi = U + kBpThreads;       // (u is dead)
    bp_range_body(p, T, t, S, lo, hi);
    __syncthreads();
    for (int h = kBpThreads / 2; h > 0; h >>= 1) {
        bp_minmax_step(lo, hi, t, h);
        __syncthreads();
    }
    if (t == 0) bp_range_finish(p, T, lo, hi);
}

__global__ __launch_bounds__(kBpThreads) void k_peaks_levels(BpArgs p) {
    __shared__ double lo[kBpThreads], hi[kBpThreads];
    const int t = (int)threadIdx.x;
    bp_levels_body(p, (long long)blockIdx.x, t, lo, hi);
    __syncthreads();
    for (int h = kBpThreads / 2; h > 0; h >>= 1) {
        bp_minmax_step(lo, hi, t, h);
        __syncthreads();
    }
    if (t == 0) bp_levels_finish(p, (long long)blockIdx.x, lo, hi);
}

__global__ __launch_bounds__(kBpThreads) void k_peaks_mark(BpArgs p) {
    extern __shared__ double bp_mark_lds[];
    const BpTile T = bp_tile(p, (long long)blockIdx.x, p.r);
    double* U = bp_mark_lds;
    double* S = bp_mark_lds + T.UH * T.SW;
    const int t = (int)threadIdx.x;
    bp_row_body(p, T, t, U);
    __syncthreads();
    bp_col_body(p, T, t, U, S);
    __syncthreads();
    unsigned char* flags = reinterpret_cast<unsigned char*>(U);   // (u is dead)
    bp_mark_body(p, T, t, S, flags);
    __syncthreads();
    bp_word_body(p, T, t, flags);
}

__global__ __launch_bounds__(kBpThreads) void k_peaks_compact(BpArgs p) {
    __shared__ long long counts[kBpThreads];
    const int t = (int)threadIdx.x;
    const long long img = (long long)blockIdx.x;
    counts[t] = bp_count_body(p, img, t);
    __syncthreads();
    if (t == 0) bp_scan_body(p, img, counts);
    __syncthreads();
    bp_write_body(p, img, t, counts[t]);
}

hipError_t find_peaks(const BpArgs& a, hipStream_t s) {
    constexpr long long kMaxGrid = 0x7fffffffll;
    if (a.n <= 0) return hipSuccess;
    const long long tiles = (long long)a.n * a.nty * a.ntx;
    const size_t lds_range = bp_lds_bytes(a.h, 0), lds_mark = bp_lds_bytes(a.h, a.r);
    if (tiles < 1 || tiles > kMaxGrid || lds_range > 65536 || lds_mark > 65536) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_peaks_range, dim3((unsigned)tiles), dim3(kBpThreads), lds_range, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_peaks_levels, dim3((unsigned)a.n), dim3(kBpThreads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_peaks_mark, dim3((unsigned)tiles), dim3(kBpThreads), lds_mark, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_peaks_compact, dim3((unsigned)a.n), dim3(kBpThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace rl
