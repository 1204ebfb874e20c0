// affine_kernels.hip -- the gfx950 kernels of rl_warp_images and rl_affine_sums (bodies, the work split, the LDS layout and the order
// of every sum: affine_kernels.hpp).  The prefilter passes of order 3 are k_shift_pass of register_kernels.hip with another tap table.
//   k_warp_eval<TS, TD, ORDER>   a workgroup per output tile of 32 x 32: the tile's source footprint through LDS where it fits 48 KB,
//                                global reads through the mirror rule otherwise; the same arithmetic either way
//   k_warp_totals                the workgroups' statistics -> raised, sum per image
//   k_affine_sums<TA, TW>        a workgroup per (pair, run of interior pixels): 45 float64 sums per thread in registers, the tree
//   k_affine_totals              the runs' partials -> one row of 45 sums per pair, in increasing order
// No atomics anywhere.
#include <hip/hip_runtime.h>
#include "affine_kernels.hpp"
#include "kernel_table.hpp"

namespace rl {

template <typename TS, typename TD, int ORDER>
__global__ __launch_bounds__(kRegThreads) void k_warp_eval(WarpParams<TS, TD> p) {
    __shared__ double lds[kWarpLds];
    __shared__ double sm[kWarpFields][kRegThreads];
    const int t = threadIdx.x;
    const unsigned nb = (unsigned)p.nby * (unsigned)p.nbx;
    const size_t i = blockIdx.x / nb;
    const int b = (int)(blockIdx.x % nb), by = b / p.nbx, bx = b % p.nbx;
    const TS* s = p.src + i * (size_t)p.sy * p.sx;
    const WarpBox box = warp_box<ORDER>(p.xf + i * kWarpXf, p.oy, p.ox, by, bx, p.direct);   // (uniform)
    double sums[kWarpFields];
    if (box.staged) {
        warp_stage<TS>(s, p.sy, p.sx, box, t, lds);
        __syncthreads();
        const WarpFetchLds fetch{lds, box.y0, box.x0, box.cols};
        warp_compute<TS, TD, ORDER>(p, i, by, bx, t, fetch, sums);
    } else {
        const WarpFetchGlobal<TS> fetch{s, p.sy, p.sx};
        warp_compute<TS, TD, ORDER>(p, i, by, bx, t, fetch, sums);
    }
    if (!p.part) return;   // (uniform)
    for (int f = 0; f < kWarpFields; ++f) sm[f][t] = sums[f];
    __syncthreads();
    for (int h = kRegThreads / 2; h > 0; h >>= 1) {
        for (int f = 0; f < kWarpFields; ++f) accel_tree_step(sm[f], t, h);
        __syncthreads();
    }
    if (t < kWarpFields) p.part[(size_t)blockIdx.x * kWarpFields + t] = sm[t][0];
}

// one thread per (image, field)
__global__ __launch_bounds__(kRegThreads) void k_warp_totals(const double* part, double* stats, int nb, size_t values) {
    const size_t id = (size_t)blockIdx.x * kRegThreads + threadIdx.x;
    if (id >= values) return;
    const size_t img = id / kWarpFields;
    stats[id] = ingest_total(part + img * (size_t)nb * kWarpFields, nb, kWarpFields, (int)(id % kWarpFields));
}

template <typename TA, typename TW>
__global__ __launch_bounds__(kRegThreads) void k_affine_sums(AffParams<TA, TW> p) {
    __shared__ double sm[kAffBatch][kRegThreads];
    const int t = threadIdx.x;
    const unsigned b = blockIdx.x % p.g.nb;
    const int pair = (int)(blockIdx.x / p.g.nb);
    double acc[kAffFields];
    aff_accumulate<TA, TW>(p, pair, b, t, acc);
    double* out = p.part + (size_t)blockIdx.x * kAffFields;
#pragma unroll
    for (int f0 = 0; f0 < kAffFields; f0 += kAffBatch) {
#pragma unroll
        for (int f = 0; f < kAffBatch; ++f) sm[f][t] = acc[f0 + f];
        __syncthreads();
        for (int h = kRegThreads / 2; h > 0; h >>= 1) {
#pragma unroll
            for (int f = 0; f < kAffBatch; ++f) accel_tree_step(sm[f], t, h);
            __syncthreads();
        }
        if (t < kAffBatch) out[f0 + t] = sm[t][0];
        __syncthreads();
    }
}

// one thread per (pair, field)
__global__ __launch_bounds__(kRegThreads) void k_affine_totals(const double* part, double* tot, int nb, size_t values) {
    const size_t id = (size_t)blockIdx.x * kRegThreads + threadIdx.x;
    if (id >= values) return;
    const size_t pair = id / kAffFields;
    tot[id] = ingest_total(part + pair * (size_t)nb * kAffFields, nb, kAffFields, (int)(id % kAffFields));
}

namespace {
constexpr size_t kMaxGrid = 0x7fffffffull;

template <typename TS, typename TD, int ORDER>
hipError_t eval_t(const WarpArgs& a, hipStream_t s) {
    const WarpParams<TS, TD> p = warp_params<TS, TD>(a);
    const size_t blocks = (size_t)a.n * p.nby * p.nbx;
    if (blocks > kMaxGrid) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_warp_eval<TS, TD, ORDER>), dim3((unsigned)blocks), dim3(kRegThreads), 0, s, p);
    return hipGetLastError();
}

template <typename TA, typename TW>
hipError_t aff_t(const AffArgs& a, hipStream_t s) {
    const size_t blocks = (size_t)a.pairs * a.g.nb;
    if (blocks > kMaxGrid) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_affine_sums<TA, TW>), dim3((unsigned)blocks), dim3(kRegThreads), 0, s, aff_params<TA, TW>(a));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t values = (size_t)a.pairs * kAffFields, tb = (values + kRegThreads - 1) / kRegThreads;
    hipLaunchKernelGGL(k_affine_totals, dim3((unsigned)tb), dim3(kRegThreads), 0, s, (const double*)a.part, a.tot, (int)a.g.nb, values);
    return hipGetLastError();
}
}  // namespace

hipError_t warp_images(int src_dtype, int dst_dtype, const WarpArgs& a, double* stats, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (stats && !a.part) return hipErrorInvalidValue;
    if (a.order == 3 && src_dtype != DT_F64) return hipErrorInvalidValue;
    WarpArgs w = a;
    if (!stats) w.part = nullptr;
    hipError_t e;
    if (a.order == 3)
        e = dst_dtype == DT_F32 ? eval_t<double, float, 3>(w, s) : eval_t<double, double, 3>(w, s);
    else if (src_dtype == DT_F32)
        e = dst_dtype == DT_F32 ? eval_t<float, float, 1>(w, s) : eval_t<float, double, 1>(w, s);
    else
        e = dst_dtype == DT_F32 ? eval_t<double, float, 1>(w, s) : eval_t<double, double, 1>(w, s);
    if (e != hipSuccess || !stats) return e;
    const int nb = warp_blocks_y(a.oy) * warp_blocks_x(a.ox);
    const size_t values = (size_t)a.n * kWarpFields, tb = (values + kRegThreads - 1) / kRegThreads;
    hipLaunchKernelGGL(k_warp_totals, dim3((unsigned)tb), dim3(kRegThreads), 0, s, (const double*)a.part, stats, nb, values);
    return hipGetLastError();
}

hipError_t affine_sums(int a_dtype, int w_dtype, const AffArgs& a, hipStream_t s) {
    if (a.pairs <= 0) return hipSuccess;
    if (a_dtype == DT_F32) return w_dtype == DT_F32 ? aff_t<float, float>(a, s) : aff_t<float, double>(a, s);
    return w_dtype == DT_F32 ? aff_t<double, float>(a, s) : aff_t<double, double>(a, s);
}

}  // namespace rl
