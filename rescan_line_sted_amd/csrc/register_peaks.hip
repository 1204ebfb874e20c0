// register_peaks.hip -- the gfx950 kernel of rl_register_peaks and rl_register_estimate (the body, the tie rule and the arithmetic:
// register_kernels.hpp, PEAKS).
//   k_register_peaks   a workgroup of 256 threads per pair: NCC per displacement, the first maximum through an LDS tree, the
//                      parabola on thread 0, optionally the surface
// No atomics.
#include <hip/hip_runtime.h>
#include "register_kernels.hpp"

namespace rl {

__global__ __launch_bounds__(kRegThreads) void k_register_peaks(RegPeakArgs a) {
    __shared__ double sv[kRegThreads];
    __shared__ int si[kRegThreads], sf[kRegThreads];
    const int t = threadIdx.x;
    const size_t pair = blockIdx.x;
    const int W = 2 * a.R + 1, nd = W * W;
    const double* tp = a.tot + pair * (size_t)(nd * kRegFields + 2);
    double v;
    int i, f;
    reg_peak_scan(tp, nd, a.n, t, v, i, f);
    sv[t] = v; si[t] = i; sf[t] = f;
    __syncthreads();
    for (int h = kRegThreads / 2; h > 0; h >>= 1) {
        reg_peak_tree_step(sv, si, sf, t, h);
        __syncthreads();
    }
    if (t == 0) reg_peak_finish(tp, a.R, a.n, sv[0], si[0], sf[0], a.peaks + pair * kPeakFields);
    if (a.surf) reg_peak_surface(tp, nd, a.n, t, sf[0], a.surf + pair * (size_t)nd);
}

hipError_t register_peaks(const RegPeakArgs& a, hipStream_t s) {
    if (a.pairs <= 0) return hipSuccess;
    if (a.R < 1 || a.R > kRegMaxR) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_register_peaks, dim3((unsigned)a.pairs), dim3(kRegThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace rl
