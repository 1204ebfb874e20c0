// tv_kernels.hip -- the two gfx950 kernels of total-variation regularised Richardson-Lucy (bodies, the tile layout and the order of
// every sum: tv_kernels.hpp).  WEIGHT: one workgroup of four waves per tile of a frame, grid (tiles, frames); APPLY / SUM: a streaming
// kernel with the work split of accel_kernels.hip, grid (nb, frames).
#include <hip/hip_runtime.h>
#include "tv_kernels.hpp"
#include "kernel_table.hpp"

namespace rl {

template <typename T>
__global__ __launch_bounds__(kAccelThreads) void k_tv_weight(TvParams<T> p) {
    __shared__ __attribute__((aligned(16))) T tile[tv_lds_elems<T>()];
    __shared__ double part[kAccelMaxBlocks];
    __shared__ double s_s;
    const int t = threadIdx.x, b = blockIdx.x, f = blockIdx.y;
    // every workgroup of the frame forms the same s from the same partials in the same order
    for (int i = t; i < p.nb; i += kAccelThreads) part[i] = p.part[(size_t)f * p.nb + i];
    tv_stage_thread<T>(p, f, b, t, tile);
    __syncthreads();
    if (t == 0) s_s = tv_mean(part, p.nb, (size_t)p.ny * p.nx);
    __syncthreads();
    tv_weight_thread<T>(p, f, b, t, tile, tv_eps2<T>(p.eps_rel, s_s));
}

template <typename T>
__global__ __launch_bounds__(kAccelThreads) void k_tv_apply(TvParams<T> p) {
    __shared__ double ss[kAccelThreads];
    const int t = threadIdx.x, b = blockIdx.x, f = blockIdx.y;
    ss[t] = tv_apply_thread<T>(p, f, b, t);
    __syncthreads();
    for (int h = kAccelThreads / 2; h > 0; h >>= 1) {
        accel_tree_step(ss, t, h);
        __syncthreads();
    }
    if (t == 0) p.part[(size_t)f * p.nb + b] = ss[0];
}

namespace {
constexpr int kMaxFramesPerLaunch = 65535;   // grid.y

template <typename T>
hipError_t launch_t(bool weight, void* est, void* w, double* part, double lambda, double eps_rel, int ny, int nx, int frames, int flags,
                    hipStream_t s) {
    const size_t n = (size_t)ny * nx;
    const int nb = accel_blocks(n, sizeof(T));
    for (int f0 = 0; f0 < frames; f0 += kMaxFramesPerLaunch) {
        const int nf = frames - f0 < kMaxFramesPerLaunch ? frames - f0 : kMaxFramesPerLaunch;
        TvParams<T> p;
        p.est = (T*)est + (size_t)f0 * n;
        p.w = w ? (T*)w + (size_t)f0 * n : nullptr;
        p.part = part + (size_t)f0 * nb;
        p.lambda = lambda;
        p.eps_rel = eps_rel;
        p.ny = ny;
        p.nx = nx;
        p.nb = nb;
        p.tiles_x = tv_tiles_x(nx, sizeof(T));
        p.flags = flags;
        if (weight) hipLaunchKernelGGL(k_tv_weight<T>, dim3(p.tiles_x * tv_tiles_y(ny), nf), dim3(kAccelThreads), 0, s, p);
        else hipLaunchKernelGGL(k_tv_apply<T>, dim3(nb, nf), dim3(kAccelThreads), 0, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

hipError_t tv_weight(int dtype, const void* est, void* w, const double* part, double lambda, double eps_rel, int ny, int nx, int frames,
                     hipStream_t s) {
    if (frames <= 0 || ny <= 0 || nx <= 0) return hipSuccess;
    return dtype == DT_F32 ? launch_t<float>(true, const_cast<void*>(est), w, const_cast<double*>(part), lambda, eps_rel, ny, nx, frames, 0, s)
                           : launch_t<double>(true, const_cast<void*>(est), w, const_cast<double*>(part), lambda, eps_rel, ny, nx, frames, 0, s);
}

hipError_t tv_apply(int dtype, void* est, const void* w, double* part, int ny, int nx, int frames, int flags, hipStream_t s) {
    if (frames <= 0 || ny <= 0 || nx <= 0) return hipSuccess;
    return dtype == DT_F32 ? launch_t<float>(false, est, const_cast<void*>(w), part, 0.0, 1.0, ny, nx, frames, flags, s)
                           : launch_t<double>(false, est, const_cast<void*>(w), part, 0.0, 1.0, ny, nx, frames, flags, s);
}

}  // namespace rl
