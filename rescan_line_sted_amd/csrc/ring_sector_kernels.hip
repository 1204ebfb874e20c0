// ring_sector_kernels.hip -- the gfx950 kernel of rl_ring_sector_stats that rl_ring_stats does not have (ROWS and COLS are those of
// ring_kernels.hip; bodies and the order of every sum: ring_kernels.hpp).
//   k_ring_reduce_sectors       grid (n_rings, pairs), 256 threads = four wave64s, no LDS: wave w sums the cells of sectors
//                               w, w + 4, ... of its ring -- a lane the cell's bins lane, lane + 64, ..., then a shuffle tree
#include <hip/hip_runtime.h>
#include "ring_kernels.hpp"

namespace rl {

static_assert(kRingWave == 64, "the tree below is a wave64's");

__global__ __launch_bounds__(kRingThreads) void k_ring_reduce_sectors(RingSectorParams p) {
    const int lane = threadIdx.x & (kRingWave - 1), wave = threadIdx.x / kRingWave, ring = blockIdx.x, pair = blockIdx.y;
    for (int sector = wave; sector < p.n_sectors; sector += kRingThreads / kRingWave) {   // (uniform over the wave)
        double v[4], up[4];
        ring_sector_lane(p, pair, ring, sector, lane, v);
        for (int h = kRingWave / 2; h > 0; h >>= 1) {
            for (int c = 0; c < 4; ++c) up[c] = __shfl_down(v[c], h, kRingWave);
            ring_wave_step(v, up);
        }
        if (lane == 0) ring_sector_write(p, pair, ring, sector, v);
    }
}

hipError_t ring_reduce_sectors(const void* f, const int* cell_ptr, const int* bins, double* out, int ny, int nx, int n_rings,
                               int n_sectors, int pairs, hipStream_t s) {
    if (pairs <= 0) return hipSuccess;
    RingSectorParams p;
    p.f = (const RingC*)f;
    p.cell_ptr = cell_ptr;
    p.bins = bins;
    p.out = out;
    p.ny = ny;
    p.nx = nx;
    p.n_rings = n_rings;
    p.n_sectors = n_sectors;
    hipLaunchKernelGGL(k_ring_reduce_sectors, dim3(n_rings, pairs), dim3(kRingThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace rl
