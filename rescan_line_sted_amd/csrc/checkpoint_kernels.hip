// checkpoint_kernels.hip -- the gfx950 kernels of rl_batch_submit_checkpoints (bodies, the work split and the order of every sum:
// checkpoint_kernels.hpp).
//   k_checkpoint<T, TO>     grid (nb, frames), 256 threads: a streaming kernel, one workgroup per run of a frame's vectors; reads
//                           est and obj once, writes the cast estimate, then the tree over the six sums (12 288 bytes of LDS)
//   k_checkpoint_totals     one thread per frame: the partials in increasing order
#include <hip/hip_runtime.h>
#include "checkpoint_kernels.hpp"
#include "kernel_table.hpp"

namespace rl {

template <typename T, typename TO>
__global__ __launch_bounds__(kCheckpointThreads) void k_checkpoint(CheckpointParams<T, TO> p) {
    __shared__ double s[kCheckpointFields][kCheckpointThreads];
    const int t = threadIdx.x, b = blockIdx.x, f = blockIdx.y;
    double v[kCheckpointFields];
    checkpoint_thread<T, TO>(p, f, b, t, v);
    if (!p.part) return;   // (the same for every thread of the launch)
    for (int c = 0; c < kCheckpointFields; ++c) s[c][t] = v[c];
    __syncthreads();
    for (int h = kCheckpointThreads / 2; h > 0; h >>= 1) {
        checkpoint_tree_step(s, t, h);
        __syncthreads();
    }
    if (t == 0) checkpoint_write_part(p.part, p.nb, f, b, s);
}

__global__ __launch_bounds__(kCheckpointThreads) void k_checkpoint_totals(const double* part, int nb, int frames, double* out) {
    const int f = blockIdx.x * kCheckpointThreads + threadIdx.x;
    if (f < frames) checkpoint_total(part, nb, f, out);
}

namespace {
template <typename T, typename TO>
hipError_t take_t(const void* est, const void* obj, void* dst, double* part, size_t n, int frames, hipStream_t s) {
    CheckpointParams<T, TO> p;
    p.est = (const T*)est;
    p.obj = (const T*)obj;
    p.dst = (TO*)dst;
    p.part = part;
    p.n = n;
    p.nb = checkpoint_blocks(n, sizeof(T));
    hipLaunchKernelGGL((k_checkpoint<T, TO>), dim3(p.nb, frames), dim3(kCheckpointThreads), 0, s, p);
    return hipGetLastError();
}
}  // namespace

hipError_t checkpoint_take(int dtype, const void* est, const void* obj, int out_dtype, void* dst, double* part, size_t n, int frames,
                           hipStream_t s) {
    if (frames <= 0 || n == 0 || (!dst && !part)) return hipSuccess;
    const bool of = dst ? out_dtype == DT_F32 : dtype == DT_F32;   // (without a destination: the instance that casts nothing)
    if (dtype == DT_F32)
        return of ? take_t<float, float>(est, obj, dst, part, n, frames, s) : take_t<float, double>(est, obj, dst, part, n, frames, s);
    return of ? take_t<double, float>(est, obj, dst, part, n, frames, s) : take_t<double, double>(est, obj, dst, part, n, frames, s);
}

hipError_t checkpoint_totals(int dtype, const double* part, size_t n, int frames, double* out, hipStream_t s) {
    if (frames <= 0) return hipSuccess;
    const int nb = checkpoint_blocks(n, dtype == DT_F32 ? sizeof(float) : sizeof(double));
    hipLaunchKernelGGL(k_checkpoint_totals, dim3((frames + kCheckpointThreads - 1) / kCheckpointThreads), dim3(kCheckpointThreads), 0, s,
                       part, nb, frames, out);
    return hipGetLastError();
}

}  // namespace rl
