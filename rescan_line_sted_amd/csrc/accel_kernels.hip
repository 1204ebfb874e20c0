// accel_kernels.hip -- the two gfx950 kernels of Biggs-Andrews accelerated Richardson-Lucy (bodies and the order of every
// sum: accel_kernels.hpp).  Streaming kernels, one workgroup of four waves per run of a frame's vectors: grid (nb, frames).
#include <hip/hip_runtime.h>
#include "accel_kernels.hpp"
#include "kernel_table.hpp"

namespace rl {

template <typename T>
__global__ __launch_bounds__(kAccelThreads) void k_accel_reduce(AccelParams<T> p) {
    __shared__ double sn[kAccelThreads], sd[kAccelThreads];
    const int t = threadIdx.x, b = blockIdx.x, f = blockIdx.y;
    double num, den;
    accel_reduce_thread<T>(p, f, b, t, num, den);
    if (!(p.flags & ACC_HAVE_PREV)) {   // (uniform) no g_{k-1}: the partials are 0
        if (t == 0) {
            p.part[((size_t)f * p.nb + b) * 2] = 0.0;
            p.part[((size_t)f * p.nb + b) * 2 + 1] = 0.0;
        }
        return;
    }
    sn[t] = num;
    sd[t] = den;
    __syncthreads();
    for (int h = kAccelThreads / 2; h > 0; h >>= 1) {
        accel_tree_step(sn, t, h);
        accel_tree_step(sd, t, h);
        __syncthreads();
    }
    if (t == 0) {
        p.part[((size_t)f * p.nb + b) * 2] = sn[0];
        p.part[((size_t)f * p.nb + b) * 2 + 1] = sd[0];
    }
}

template <typename T>
__global__ __launch_bounds__(kAccelThreads) void k_accel_extrapolate(AccelParams<T> p) {
    __shared__ double part[2 * kAccelMaxBlocks];
    __shared__ double a_s;
    const int t = threadIdx.x, b = blockIdx.x, f = blockIdx.y;
    if (!(p.flags & ACC_FRESH)) {
        // every workgroup of the frame forms the same a from the same partials in the same order
        for (int i = t; i < 2 * p.nb; i += kAccelThreads) part[i] = p.part[(size_t)f * p.nb * 2 + i];
        __syncthreads();
        if (t == 0) a_s = accel_alpha(part, p.nb);
    } else if (t == 0) {
        a_s = 0.0;
    }
    __syncthreads();
    const double a = a_s;
    if (b == 0 && t == 0) p.alpha[f] = a;
    accel_extrapolate_thread<T>(p, f, b, t, a);
}

namespace {
constexpr int kMaxFramesPerLaunch = 65535;   // grid.y

template <typename T>
hipError_t reduce_t(const void* est, const void* y, void* g, double* part, size_t n, int frames, int flags, hipStream_t s) {
    const int nb = accel_blocks(n, sizeof(T));
    for (int f0 = 0; f0 < frames; f0 += kMaxFramesPerLaunch) {
        const int nf = frames - f0 < kMaxFramesPerLaunch ? frames - f0 : kMaxFramesPerLaunch;
        AccelParams<T> p;
        p.est = (T*)est + (size_t)f0 * n;
        p.y = (T*)y + (size_t)f0 * n;
        p.g = (T*)g + (size_t)f0 * n;
        p.x = nullptr;
        p.part = part + (size_t)f0 * nb * 2;
        p.alpha = nullptr;
        p.n = n;
        p.nb = nb;
        p.flags = flags;
        hipLaunchKernelGGL(k_accel_reduce<T>, dim3(nb, nf), dim3(kAccelThreads), 0, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename T>
hipError_t extrapolate_t(void* est, void* y, void* x, const double* part, double* alpha, size_t n, int frames, int flags,
                         hipStream_t s) {
    const int nb = accel_blocks(n, sizeof(T));
    for (int f0 = 0; f0 < frames; f0 += kMaxFramesPerLaunch) {
        const int nf = frames - f0 < kMaxFramesPerLaunch ? frames - f0 : kMaxFramesPerLaunch;
        AccelParams<T> p;
        p.est = (T*)est + (size_t)f0 * n;
        p.y = (T*)y + (size_t)f0 * n;
        p.g = nullptr;
        p.x = (T*)x + (size_t)f0 * n;
        p.part = const_cast<double*>(part) + (size_t)f0 * nb * 2;
        p.alpha = alpha + f0;
        p.n = n;
        p.nb = nb;
        p.flags = flags;
        hipLaunchKernelGGL(k_accel_extrapolate<T>, dim3(nb, nf), dim3(kAccelThreads), 0, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

hipError_t accel_reduce(int dtype, const void* est, const void* y, void* g, double* part, size_t n, int frames, int flags,
                        hipStream_t s) {
    if (frames <= 0 || n == 0) return hipSuccess;
    return dtype == DT_F32 ? reduce_t<float>(est, y, g, part, n, frames, flags, s)
                           : reduce_t<double>(est, y, g, part, n, frames, flags, s);
}

hipError_t accel_extrapolate(int dtype, void* est, void* y, void* x, const double* part, double* alpha, size_t n, int frames,
                             int flags, hipStream_t s) {
    if (frames <= 0 || n == 0) return hipSuccess;
    return dtype == DT_F32 ? extrapolate_t<float>(est, y, x, part, alpha, n, frames, flags, s)
                           : extrapolate_t<double>(est, y, x, part, alpha, n, frames, flags, s);
}

}  // namespace rl
