// tile_api.cpp -- C ABI of tiled Richardson-Lucy (include/rlsted.h: rl_tile_axis, rl_tile_weights, rl_tile_gather, rl_tile_blend,
// rl_device_copy): the host side -- the layout (tile_layout.hpp), validation, the tables' upload, the launches of
// tile_kernels.hip.  No kernel is launched on bad geometry.
#include <algorithm>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "tile_kernels.hpp"
#include "tile_layout.hpp"

using namespace rl;

namespace {
// the origins of one axis of a blend: inside the image, non-decreasing, every pixel covered -> the coverage tables
int blend_axis(const char* name, int n, int t, int count, const int* origins, int32_t* first, int32_t* cover) {
    for (int i = 0; i < count; ++i) {
        if (origins[i] < 0 || origins[i] > n - t) return fail(RL_ERR_INVALID, std::string(name) + ": a tile overhangs the image");
        if (i > 0 && origins[i] < origins[i - 1]) return fail(RL_ERR_INVALID, std::string(name) + ": the origins decrease");
    }
    if (tile_coverage(n, t, count, origins, first, cover)) return fail(RL_ERR_INVALID, std::string(name) + ": a pixel is covered by no tile");
    return RL_OK;
}
}  // namespace

extern "C" int rl_tile_axis(int n, int tile, int overlap, int* count, int* origins) {
    if (!count) return fail(RL_ERR_INVALID, "count is NULL");
    const int c = tile_count(n, tile, overlap);
    if (c < 0) return fail(RL_ERR_INVALID, tile_layout_message(-c));
    *count = c;
    if (origins) tile_origins(n, tile, c, origins);
    return RL_OK;
}

extern "C" int rl_tile_weights(int n, int tile, int overlap, int margin, int count, const int* origins, double* weights_out,
                               int* first_out, int* count_out) {
    if (!origins) return fail(RL_ERR_INVALID, "origins is NULL");
    if ((first_out == nullptr) != (count_out == nullptr)) return fail(RL_ERR_INVALID, "first_out and count_out go together");
    if (n < 1 || tile < 1) return fail(RL_ERR_INVALID, tile_layout_message(TILE_BAD_SIZE));
    if (overlap < 1 || overlap >= tile) return fail(RL_ERR_INVALID, tile_layout_message(TILE_BAD_OVERLAP));
    if (margin < 0 || 2 * (long long)margin >= overlap) return fail(RL_ERR_INVALID, tile_layout_message(TILE_BAD_MARGIN));
    static_assert(sizeof(int) == sizeof(int32_t), "the tables are 32-bit");
    if (int e = tile_weights(n, tile, margin, count, origins, weights_out, (int32_t*)first_out, (int32_t*)count_out))
        return fail(RL_ERR_INVALID, tile_layout_message(e));
    return RL_OK;
}

extern "C" int rl_tile_gather(rl_ctx* ctx, const void* src_dev, int src_dtype, int F, int V, int NY, int NX, const int* slots,
                              int n_slots, int ty, int tx, void* dst_dev, int dst_dtype) {
    if (!ctx || !src_dev || !slots || !dst_dev) return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(src_dtype) || !dtype_ok(dst_dtype)) return fail(RL_ERR_INVALID, "dtypes must be RL_F32 or RL_F64");
    if (F < 1 || V < 1 || NY < 1 || NX < 1) return fail(RL_ERR_INVALID, "F, V, NY and NX must be at least 1");
    if (n_slots < 1) return fail(RL_ERR_INVALID, "n_slots < 1");
    if (ty < 1 || tx < 1 || ty > NY || tx > NX) return fail(RL_ERR_INVALID, "the tile must lie within the image");
    for (int k = 0; k < n_slots; ++k) {
        const int f = slots[3 * k], ay = slots[3 * k + 1], ax = slots[3 * k + 2];
        if (f == -1) continue;
        if (f < 0 || f >= F) return fail(RL_ERR_INVALID, "slot " + std::to_string(k) + ": frame out of range");
        if (ay < 0 || ay > NY - ty || ax < 0 || ax > NX - tx) return fail(RL_ERR_INVALID, "slot " + std::to_string(k) + ": the tile overhangs the image");
    }
    const size_t src_bytes = (size_t)F * V * NY * NX * dtype_size(src_dtype), dst_bytes = (size_t)n_slots * V * ty * tx * dtype_size(dst_dtype);
    if (overlaps(src_dev, src_bytes, dst_dev, dst_bytes)) return fail(RL_ERR_INVALID, "the destination overlaps the source");
    HIP_TRY(hipSetDevice(ctx->device));
    WorkLayout lay;
    const auto r_slots = lay.add<int32_t>((size_t)n_slots * 3);
    char* base = nullptr;
    RL_TRY(ctx->tile.reserve(ctx->stream, lay.bytes(), &base));
    // (a pageable source: the copy has left it when it returns)
    HIP_TRY(hipMemcpyAsync(r_slots.at(base), slots, r_slots.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(tile_gather(src_dtype, dst_dtype, src_dev, dst_dev, r_slots.at(base), n_slots, V, NY, NX, ty, tx, ctx->stream));
    return RL_OK;
}

extern "C" int rl_tile_blend(rl_ctx* ctx, const void* tiles_dev, int tiles_dtype, int F, int NY, int NX, int ny_tiles, int nx_tiles, int ty,
                             int tx, const int* origins_y, const int* origins_x, const double* wy, const double* wx, void* out_dev,
                             int out_dtype) {
    if (!ctx || !tiles_dev || !origins_y || !origins_x || !wy || !wx || !out_dev) return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(tiles_dtype) || !dtype_ok(out_dtype)) return fail(RL_ERR_INVALID, "dtypes must be RL_F32 or RL_F64");
    if (F < 1 || NY < 1 || NX < 1) return fail(RL_ERR_INVALID, "F, NY and NX must be at least 1");
    if (ny_tiles < 1 || nx_tiles < 1) return fail(RL_ERR_INVALID, "ny_tiles and nx_tiles must be at least 1");
    if (ty < 1 || tx < 1 || ty > NY || tx > NX) return fail(RL_ERR_INVALID, "the tile must lie within the image");
    WorkLayout lay;
    const auto r_oy = lay.add<int32_t>((size_t)ny_tiles), r_ox = lay.add<int32_t>((size_t)nx_tiles);
    const auto r_wy = lay.add<double>((size_t)ny_tiles * ty), r_wx = lay.add<double>((size_t)nx_tiles * tx);
    const auto r_fy = lay.add<int32_t>((size_t)NY), r_cy = lay.add<int32_t>((size_t)NY);
    const auto r_fx = lay.add<int32_t>((size_t)NX), r_cx = lay.add<int32_t>((size_t)NX);
    // the eight tables go up in ONE copy, staged in the device layout
    std::vector<char> stage(lay.bytes(), 0);
    char* h = stage.data();
    RL_TRY(blend_axis("rows", NY, ty, ny_tiles, origins_y, r_fy.at(h), r_cy.at(h)));
    RL_TRY(blend_axis("columns", NX, tx, nx_tiles, origins_x, r_fx.at(h), r_cx.at(h)));
    std::copy(origins_y, origins_y + ny_tiles, r_oy.at(h));
    std::copy(origins_x, origins_x + nx_tiles, r_ox.at(h));
    std::copy(wy, wy + (size_t)ny_tiles * ty, r_wy.at(h));
    std::copy(wx, wx + (size_t)nx_tiles * tx, r_wx.at(h));
    const size_t tiles_bytes = (size_t)F * ny_tiles * nx_tiles * ty * tx * dtype_size(tiles_dtype);
    const size_t out_bytes = (size_t)F * NY * NX * dtype_size(out_dtype);
    if (overlaps(tiles_dev, tiles_bytes, out_dev, out_bytes)) return fail(RL_ERR_INVALID, "the output overlaps the tile store");
    HIP_TRY(hipSetDevice(ctx->device));
    char* base = nullptr;
    RL_TRY(ctx->tile.reserve(ctx->stream, lay.bytes(), &base));
    HIP_TRY(hipMemcpyAsync(base, h, lay.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(tile_blend(tiles_dtype, out_dtype, tiles_dev, out_dev, r_oy.at(base), r_ox.at(base), r_wy.at(base), r_wx.at(base), r_fy.at(base),
                       r_cy.at(base), r_fx.at(base), r_cx.at(base), F, NY, NX, ny_tiles, nx_tiles, ty, tx, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RL_OK;
}

extern "C" int rl_device_copy(rl_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes) {
    if (!ctx || (bytes && (!dst_dev || !src_dev))) return fail(RL_ERR_INVALID, "NULL argument");
    if (!bytes) return RL_OK;
    if (overlaps(dst_dev, bytes, src_dev, bytes)) return fail(RL_ERR_INVALID, "the ranges overlap");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return RL_OK;
}
