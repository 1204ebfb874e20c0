// ring_kernels.hip -- the gfx950 kernels of rl_ring_stats (bodies, the tiling and the order of every sum: ring_kernels.hpp).
//   k_ring_rows / k_ring_cols   grid (ceil(nx / 64), ceil(ny / 64), pairs), 256 threads, 33 024 bytes of LDS: the two complex
//                               float64 matrix products of the 2-D DFT on v_fma_f64 register tiles
//   k_ring_reduce               grid (n_rings, pairs), 256 threads, 8 KiB of LDS: the per-ring sums
#include <hip/hip_runtime.h>
#include "ring_kernels.hpp"
#include "kernel_table.hpp"

namespace rl {

template <typename TA, typename TB>
__global__ __launch_bounds__(kRingThreads) void k_ring_rows(RingRowsParams<TA, TB> p) {
    __shared__ RingLds lds;
    const int t = threadIdx.x, n0 = blockIdx.x * kRingTile, m0 = blockIdx.y * kRingTile, pair = blockIdx.z;
    RingC acc[kRingMicro * kRingMicro];
    for (int i = 0; i < kRingMicro * kRingMicro; ++i) acc[i] = RingC{0.0, 0.0};
    RingTw tw = ring_tw_init(n0 + (t & 63), p.nx, t);
    for (int k0 = 0; k0 < p.nx; k0 += kRingKT) {
        ring_rows_load_thread(p, pair, m0, k0, tw, lds, t);
        __syncthreads();
        ring_mac_thread(lds, acc, t);
        __syncthreads();
    }
    ring_store_thread(p.out, p.ny, p.nx, pair, m0, n0, acc, t);
}

__global__ __launch_bounds__(kRingThreads) void k_ring_cols(RingColsParams p) {
    __shared__ RingLds lds;
    const int t = threadIdx.x, n0 = blockIdx.x * kRingTile, m0 = blockIdx.y * kRingTile, pair = blockIdx.z;
    RingC acc[kRingMicro * kRingMicro];
    for (int i = 0; i < kRingMicro * kRingMicro; ++i) acc[i] = RingC{0.0, 0.0};
    RingTw tw = ring_tw_init(m0 + (t & 63), p.ny, t);
    for (int k0 = 0; k0 < p.ny; k0 += kRingKT) {
        ring_cols_load_thread(p, pair, n0, k0, tw, lds, t);
        __syncthreads();
        ring_mac_thread(lds, acc, t);
        __syncthreads();
    }
    ring_store_thread(p.out, p.ny, p.nx, pair, m0, n0, acc, t);
}

__global__ __launch_bounds__(kRingThreads) void k_ring_reduce(RingReduceParams p) {
    __shared__ double s[4][kRingThreads];
    const int t = threadIdx.x, ring = blockIdx.x, pair = blockIdx.y;
    double v[4];
    ring_reduce_thread(p, pair, ring, t, v);
    for (int c = 0; c < 4; ++c) s[c][t] = v[c];
    __syncthreads();
    for (int h = kRingThreads / 2; h > 0; h >>= 1) {
        ring_tree_step(s, t, h);
        __syncthreads();
    }
    if (t == 0) ring_reduce_write(p, pair, ring, s);
}

namespace {
template <typename TA, typename TB>
hipError_t rows_t(const void* a, const void* b, const int64_t* a_off, const int64_t* b_off, const double* scale, const void* wx,
                  void* t_out, int ny, int nx, int pairs, hipStream_t s) {
    RingRowsParams<TA, TB> p;
    p.a = (const TA*)a;
    p.b = (const TB*)b;
    p.a_off = a_off;
    p.b_off = b_off;
    p.scale = scale;
    p.w = (const RingC*)wx;
    p.out = (RingC*)t_out;
    p.ny = ny;
    p.nx = nx;
    const dim3 grid((nx + kRingTile - 1) / kRingTile, (ny + kRingTile - 1) / kRingTile, pairs);
    hipLaunchKernelGGL((k_ring_rows<TA, TB>), grid, dim3(kRingThreads), 0, s, p);
    return hipGetLastError();
}
}  // namespace

hipError_t ring_rows(int a_dtype, int b_dtype, const void* a, const void* b, const int64_t* a_off, const int64_t* b_off,
                     const double* scale, const void* wx, void* t_out, int ny, int nx, int pairs, hipStream_t s) {
    if (pairs <= 0) return hipSuccess;
    if (a_dtype == DT_F32)
        return b_dtype == DT_F32 ? rows_t<float, float>(a, b, a_off, b_off, scale, wx, t_out, ny, nx, pairs, s)
                                 : rows_t<float, double>(a, b, a_off, b_off, scale, wx, t_out, ny, nx, pairs, s);
    return b_dtype == DT_F32 ? rows_t<double, float>(a, b, a_off, b_off, scale, wx, t_out, ny, nx, pairs, s)
                             : rows_t<double, double>(a, b, a_off, b_off, scale, wx, t_out, ny, nx, pairs, s);
}

hipError_t ring_cols(const void* t_in, const void* wy, void* f_out, int ny, int nx, int pairs, hipStream_t s) {
    if (pairs <= 0) return hipSuccess;
    RingColsParams p;
    p.in = (const RingC*)t_in;
    p.w = (const RingC*)wy;
    p.out = (RingC*)f_out;
    p.ny = ny;
    p.nx = nx;
    const dim3 grid((nx + kRingTile - 1) / kRingTile, (ny + kRingTile - 1) / kRingTile, pairs);
    hipLaunchKernelGGL(k_ring_cols, grid, dim3(kRingThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t ring_reduce(const void* f, const int* row_ptr, const int* bins, double* out, int ny, int nx, int n_rings, int pairs,
                       hipStream_t s) {
    if (pairs <= 0) return hipSuccess;
    RingReduceParams p;
    p.f = (const RingC*)f;
    p.row_ptr = row_ptr;
    p.bins = bins;
    p.out = out;
    p.ny = ny;
    p.nx = nx;
    p.n_rings = n_rings;
    hipLaunchKernelGGL(k_ring_reduce, dim3(n_rings, pairs), dim3(kRingThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace rl
