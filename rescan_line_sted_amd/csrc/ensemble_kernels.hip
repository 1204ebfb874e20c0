// ensemble_kernels.hip -- the gfx950 kernels of rl_ensemble_stats (bodies, the work split and the order of every sum:
// ensemble_kernels.hpp).
//   k_ensemble_stats<T, TT>    grid (nb, groups), 256 threads: a streaming kernel, one workgroup per run of a group's vectors; two
//                              passes over the members (out of registers for groups of up to 16), the maps, then the tree over
//                              the five sums (10 240 bytes of LDS)
//   k_ensemble_totals          one thread per group: the partials in increasing order
#include <hip/hip_runtime.h>
#include "ensemble_kernels.hpp"
#include "kernel_table.hpp"

namespace rl {

template <typename T, typename TT>
__global__ __launch_bounds__(kEnsembleThreads) void k_ensemble_stats(EnsembleParams<T, TT> p, int g0) {
    __shared__ double s[kEnsembleSums][kEnsembleThreads];
    const int t = threadIdx.x, b = blockIdx.x, g = g0 + blockIdx.y;
    double v[kEnsembleSums];
    ensemble_thread<T, TT>(p, g, b, t, v);
    for (int c = 0; c < kEnsembleSums; ++c) s[c][t] = v[c];
    __syncthreads();
    for (int h = kEnsembleThreads / 2; h > 0; h >>= 1) {
        ensemble_tree_step(s, t, h);
        __syncthreads();
    }
    if (t == 0) ensemble_write_part(p.part, p.nb, g, b, s);
}

__global__ __launch_bounds__(kEnsembleThreads) void k_ensemble_totals(const double* part, const int32_t* group_ptr, int nb, int groups,
                                                                      double* out) {
    const int g = blockIdx.x * kEnsembleThreads + threadIdx.x;
    if (g < groups) ensemble_total(part, group_ptr, nb, g, out);
}

namespace {
template <typename T, typename TT>
hipError_t stats_t(const void* src, const int64_t* member_off, const int32_t* group_ptr, const void* truth, const int64_t* truth_off,
                   const double* truth_scale, double* mean, double* var, double* part, size_t n, int g0, int groups, hipStream_t s) {
    EnsembleParams<T, TT> p;
    p.src = (const T*)src;
    p.member_off = member_off;
    p.group_ptr = group_ptr;
    p.truth = (const TT*)truth;
    p.truth_off = truth_off;
    p.truth_scale = truth_scale;
    p.mean = mean;
    p.var = var;
    p.part = part;
    p.n = n;
    p.nb = ensemble_blocks(n, sizeof(T));
    hipLaunchKernelGGL((k_ensemble_stats<T, TT>), dim3(p.nb, groups), dim3(kEnsembleThreads), 0, s, p, g0);
    return hipGetLastError();
}
}  // namespace

hipError_t ensemble_stats(int src_dtype, int truth_dtype, const void* src, const int64_t* member_off, const int32_t* group_ptr,
                          const void* truth, const int64_t* truth_off, const double* truth_scale, double* mean, double* var,
                          double* part, size_t n, int g0, int groups, hipStream_t s) {
    if (groups <= 0 || n == 0) return hipSuccess;
    const bool tf = truth && truth_dtype == DT_F32;   // (without a truth: the float64 instance, which never reads it)
    if (src_dtype == DT_F32)
        return tf ? stats_t<float, float>(src, member_off, group_ptr, truth, truth_off, truth_scale, mean, var, part, n, g0, groups, s)
                  : stats_t<float, double>(src, member_off, group_ptr, truth, truth_off, truth_scale, mean, var, part, n, g0, groups, s);
    return tf ? stats_t<double, float>(src, member_off, group_ptr, truth, truth_off, truth_scale, mean, var, part, n, g0, groups, s)
              : stats_t<double, double>(src, member_off, group_ptr, truth, truth_off, truth_scale, mean, var, part, n, g0, groups, s);
}

hipError_t ensemble_totals(int src_dtype, const double* part, const int32_t* group_ptr, size_t n, int groups, double* out,
                           hipStream_t s) {
    if (groups <= 0) return hipSuccess;
    const int nb = ensemble_blocks(n, src_dtype == DT_F32 ? sizeof(float) : sizeof(double));
    hipLaunchKernelGGL(k_ensemble_totals, dim3((groups + kEnsembleThreads - 1) / kEnsembleThreads), dim3(kEnsembleThreads), 0, s, part,
                       group_ptr, nb, groups, out);
    return hipGetLastError();
}

}  // namespace rl
