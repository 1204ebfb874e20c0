// stop_kernels.hip -- the gfx950 kernels of the Poisson I-divergence and the stopping rule (bodies, the work split and the order of
// every sum: stop_kernels.hpp).  Streaming kernels, one workgroup of four waves per run of a frame's vectors: grid (nb, frames).
#include <hip/hip_runtime.h>
#include "stop_kernels.hpp"
#include "kernel_table.hpp"

namespace rl {

template <typename T>
__global__ __launch_bounds__(kStopThreads) void k_stop_divergence(DivParams<T> p) {
    __shared__ double s[kStopThreads];
    const int t = threadIdx.x, b = blockIdx.x, f = blockIdx.y;
    s[t] = stop_divergence_thread<T>(p, f, b, t);
    __syncthreads();
    for (int h = kStopThreads / 2; h > 0; h >>= 1) {
        accel_tree_step(s, t, h);
        __syncthreads();
    }
    if (t == 0) p.part[(size_t)f * p.nb + b] = s[0];
}

__global__ __launch_bounds__(kStopThreads) void k_stop_totals(const double* part, int nb, int frames, double* out) {
    const int f = blockIdx.x * kStopThreads + threadIdx.x;
    if (f < frames) out[f] = stop_total(part + (size_t)f * nb, nb);
}

template <typename T>
__global__ __launch_bounds__(kStopThreads) void k_stop_latch(LatchParams<T> p) {
    __shared__ double part[kStopMaxBlocks];
    __shared__ int copy_s;
    const int t = threadIdx.x, b = blockIdx.x, f = blockIdx.y;
    // every workgroup of the frame forms the same D from the same partials in the same order, and decides from the previous check's state
    for (int i = t; i < p.nb_part; i += kStopThreads) part[i] = p.part[(size_t)f * p.nb_part + i];
    __syncthreads();
    if (t == 0) {
        bool copy;
        const StopFrame s = stop_latch_frame<T>(p, f, stop_total(part, p.nb_part), &copy);
        copy_s = copy ? 1 : 0;
        if (b == 0) p.next[f] = s;
    }
    __syncthreads();
    if (copy_s) stop_copy_thread<T>(p, f, b, t);
}

namespace {
constexpr int kMaxFramesPerLaunch = 65535;   // grid.y

template <typename T>
hipError_t divergence_t(const void* meas, const void* pred, double* part, size_t n, int frames, hipStream_t s) {
    const int nb = stop_blocks(n, sizeof(T));
    for (int f0 = 0; f0 < frames; f0 += kMaxFramesPerLaunch) {
        const int nf = frames - f0 < kMaxFramesPerLaunch ? frames - f0 : kMaxFramesPerLaunch;
        DivParams<T> p;
        p.meas = (const T*)meas + (size_t)f0 * n;
        p.pred = (const T*)pred + (size_t)f0 * n;
        p.part = part + (size_t)f0 * nb;
        p.n = n;
        p.nb = nb;
        hipLaunchKernelGGL(k_stop_divergence<T>, dim3(nb, nf), dim3(kStopThreads), 0, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename T>
hipError_t latch_t(const void* est, void* result, const double* part, const StopFrame* prev, StopFrame* next, size_t n_img, size_t n_frame,
                   int frames, int rule, double threshold, int done, int have_prev, hipStream_t s) {
    const int nb = accel_blocks(n_img, sizeof(T)), nb_part = stop_blocks(n_frame, sizeof(T));
    for (int f0 = 0; f0 < frames; f0 += kMaxFramesPerLaunch) {
        const int nf = frames - f0 < kMaxFramesPerLaunch ? frames - f0 : kMaxFramesPerLaunch;
        LatchParams<T> p;
        p.est = (const T*)est + (size_t)f0 * n_img;
        p.result = (T*)result + (size_t)f0 * n_img;
        p.part = part + (size_t)f0 * nb_part;
        p.prev = prev + f0;
        p.next = next + f0;
        p.n = n_img;
        p.nb = nb;
        p.nb_part = nb_part;
        p.rule = rule;
        p.have_prev = have_prev;
        p.done = done;
        p.threshold = threshold;
        p.count = (double)n_frame;
        hipLaunchKernelGGL(k_stop_latch<T>, dim3(nb, nf), dim3(kStopThreads), 0, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

hipError_t stop_divergence(int dtype, const void* meas, const void* pred, double* part, size_t n_frame, int frames, hipStream_t s) {
    if (frames <= 0 || n_frame == 0) return hipSuccess;
    return dtype == DT_F32 ? divergence_t<float>(meas, pred, part, n_frame, frames, s)
                           : divergence_t<double>(meas, pred, part, n_frame, frames, s);
}

hipError_t stop_totals(int dtype, const double* part, size_t n_frame, int frames, double* out, hipStream_t s) {
    if (frames <= 0) return hipSuccess;
    const int nb = stop_blocks(n_frame, dtype == DT_F32 ? sizeof(float) : sizeof(double));
    hipLaunchKernelGGL(k_stop_totals, dim3((frames + kStopThreads - 1) / kStopThreads), dim3(kStopThreads), 0, s, part, nb, frames, out);
    return hipGetLastError();
}

hipError_t stop_latch(int dtype, const void* est, void* result, const double* part, const StopFrame* prev, StopFrame* next, size_t n_img,
                      size_t n_frame, int frames, int rule, double threshold, int done, int have_prev, hipStream_t s) {
    if (frames <= 0 || n_img == 0) return hipSuccess;
    return dtype == DT_F32 ? latch_t<float>(est, result, part, prev, next, n_img, n_frame, frames, rule, threshold, done, have_prev, s)
                           : latch_t<double>(est, result, part, prev, next, n_img, n_frame, frames, rule, threshold, done, have_prev, s);
}

}  // namespace rl
