// tile_kernels.hip -- the gfx950 kernels of rl_tile_gather and rl_tile_blend (bodies, the work split and the order of the blend's
// sum: tile_kernels.hpp).  Two streaming kernels, one thread per 16-byte vector of the destination, 256 threads per workgroup, a
// one-dimensional grid sized by the pixels; no LDS, no atomics.
//   k_tile_gather<TS, TD>   windows of src -> the frames of a plan's measurement buffer (fillers: ones)
//   k_tile_blend<TT, TO>    the tile estimates, weighted, -> the image
#include <hip/hip_runtime.h>
#include "tile_kernels.hpp"
#include "kernel_table.hpp"

namespace rl {

template <typename TS, typename TD>
__global__ __launch_bounds__(kTileThreads) void k_tile_gather(TileGatherParams<TS, TD> p, size_t vectors) {
    const size_t id = (size_t)blockIdx.x * kTileThreads + threadIdx.x;
    if (id < vectors) tile_gather_thread<TS, TD>(p, id);
}

template <typename TT, typename TO>
__global__ __launch_bounds__(kTileThreads) void k_tile_blend(TileBlendParams<TT, TO> p, size_t vectors) {
    const size_t id = (size_t)blockIdx.x * kTileThreads + threadIdx.x;
    if (id < vectors) tile_blend_thread<TT, TO>(p, id);
}

namespace {
constexpr size_t kMaxGrid = 0x7fffffffull;   // workgroups of a one-dimensional grid

template <typename TS, typename TD>
hipError_t gather_t(const void* src, void* dst, const int32_t* slot, int slots, int V, int NY, int NX, int ty, int tx, hipStream_t s) {
    const TileGatherParams<TS, TD> p = tile_gather_params<TS, TD>(src, dst, slot, slots, V, NY, NX, ty, tx);
    const size_t vectors = tile_gather_vectors(slots, V, ty, p.cpr), blocks = (vectors + kTileThreads - 1) / kTileThreads;
    if (blocks > kMaxGrid) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_tile_gather<TS, TD>), dim3((unsigned)blocks), dim3(kTileThreads), 0, s, p, vectors);
    return hipGetLastError();
}

template <typename TT, typename TO>
hipError_t blend_t(const void* tiles, void* out, const int32_t* oy, const int32_t* ox, const double* wy, const double* wx,
                   const int32_t* first_y, const int32_t* cover_y, const int32_t* first_x, const int32_t* cover_x, int F, int NY, int NX,
                   int nyt, int nxt, int ty, int tx, hipStream_t s) {
    const TileBlendParams<TT, TO> p =
        tile_blend_params<TT, TO>(tiles, out, oy, ox, wy, wx, first_y, cover_y, first_x, cover_x, F, NY, NX, nyt, nxt, ty, tx);
    const size_t vectors = tile_blend_vectors(F, NY, p.cpr), blocks = (vectors + kTileThreads - 1) / kTileThreads;
    if (blocks > kMaxGrid) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_tile_blend<TT, TO>), dim3((unsigned)blocks), dim3(kTileThreads), 0, s, p, vectors);
    return hipGetLastError();
}
}  // namespace

hipError_t tile_gather(int src_dtype, int dst_dtype, const void* src, void* dst, const int32_t* slot, int slots, int V, int NY, int NX,
                       int ty, int tx, hipStream_t s) {
    if (slots <= 0) return hipSuccess;
    if (src_dtype == DT_F32)
        return dst_dtype == DT_F32 ? gather_t<float, float>(src, dst, slot, slots, V, NY, NX, ty, tx, s)
                                   : gather_t<float, double>(src, dst, slot, slots, V, NY, NX, ty, tx, s);
    return dst_dtype == DT_F32 ? gather_t<double, float>(src, dst, slot, slots, V, NY, NX, ty, tx, s)
                               : gather_t<double, double>(src, dst, slot, slots, V, NY, NX, ty, tx, s);
}

hipError_t tile_blend(int tiles_dtype, int out_dtype, const void* tiles, void* out, const int32_t* oy, const int32_t* ox,
                      const double* wy, const double* wx, const int32_t* first_y, const int32_t* cover_y, const int32_t* first_x,
                      const int32_t* cover_x, int F, int NY, int NX, int nyt, int nxt, int ty, int tx, hipStream_t s) {
    if (F <= 0) return hipSuccess;
    if (tiles_dtype == DT_F32)
        return out_dtype == DT_F32
                   ? blend_t<float, float>(tiles, out, oy, ox, wy, wx, first_y, cover_y, first_x, cover_x, F, NY, NX, nyt, nxt, ty, tx, s)
                   : blend_t<float, double>(tiles, out, oy, ox, wy, wx, first_y, cover_y, first_x, cover_x, F, NY, NX, nyt, nxt, ty, tx, s);
    return out_dtype == DT_F32
               ? blend_t<double, float>(tiles, out, oy, ox, wy, wx, first_y, cover_y, first_x, cover_x, F, NY, NX, nyt, nxt, ty, tx, s)
               : blend_t<double, double>(tiles, out, oy, ox, wy, wx, first_y, cover_y, first_x, cover_x, F, NY, NX, nyt, nxt, ty, tx, s);
}

}  // namespace rl
