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
size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int tile_workspace(rl_ctx* ctx, size_t bytes, char** out) {
    if (bytes > ctx->tile.work_bytes) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->tile.work) (void)hipFree(ctx->tile.work);
        ctx->tile.work = nullptr;
        ctx->tile.work_bytes = 0;
        HIP_TRY(hipMalloc(&ctx->tile.work, bytes));
        ctx->tile.work_bytes = bytes;
    }
    *out = (char*)ctx->tile.work;
    return RL_OK;
}

bool dtype_ok(int d) { return d == RL_F32 || d == RL_F64; }
size_t esize_of(int d) { return d == RL_F32 ? sizeof(float) : sizeof(double); }

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return (const char*)a < (const char*)b + b_bytes && (const char*)b < (const char*)a + a_bytes;
}

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
    const size_t src_bytes = (size_t)F * V * NY * NX * esize_of(src_dtype), dst_bytes = (size_t)n_slots * V * ty * tx * esize_of(dst_dtype);
    if (overlaps(src_dev, src_bytes, dst_dev, dst_bytes)) return fail(RL_ERR_INVALID, "the destination overlaps the source");
    HIP_TRY(hipSetDevice(ctx->device));
    char* base = nullptr;
    const size_t bytes = (size_t)n_slots * 3 * sizeof(int32_t);
    RL_TRY(tile_workspace(ctx, round_up(bytes, 256), &base));
    // (a pageable source: the copy has left it when it returns)
    HIP_TRY(hipMemcpyAsync(base, slots, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(tile_gather(src_dtype, dst_dtype, src_dev, dst_dev, (const int32_t*)base, n_slots, V, NY, NX, ty, tx, ctx->stream));
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
    const size_t b_oy = round_up((size_t)ny_tiles * 4, 256), b_ox = round_up((size_t)nx_tiles * 4, 256);
    const size_t b_wy = round_up((size_t)ny_tiles * ty * 8, 256), b_wx = round_up((size_t)nx_tiles * tx * 8, 256);
    const size_t b_gy = round_up((size_t)NY * 4, 256), b_gx = round_up((size_t)NX * 4, 256);
    const size_t o_ox = b_oy, o_wy = o_ox + b_ox, o_wx = o_wy + b_wy, o_fy = o_wx + b_wx, o_cy = o_fy + b_gy, o_fx = o_cy + b_gy,
                 o_cx = o_fx + b_gx, total = o_cx + b_gx;
    // the eight tables go up in ONE copy, staged in the device layout
    std::vector<char> stage(total, 0);
    RL_TRY(blend_axis("rows", NY, ty, ny_tiles, origins_y, (int32_t*)(stage.data() + o_fy), (int32_t*)(stage.data() + o_cy)));
    RL_TRY(blend_axis("columns", NX, tx, nx_tiles, origins_x, (int32_t*)(stage.data() + o_fx), (int32_t*)(stage.data() + o_cx)));
    std::copy(origins_y, origins_y + ny_tiles, (int32_t*)stage.data());
    std::copy(origins_x, origins_x + nx_tiles, (int32_t*)(stage.data() + o_ox));
    std::copy(wy, wy + (size_t)ny_tiles * ty, (double*)(stage.data() + o_wy));
    std::copy(wx, wx + (size_t)nx_tiles * tx, (double*)(stage.data() + o_wx));
    const size_t tiles_bytes = (size_t)F * ny_tiles * nx_tiles * ty * tx * esize_of(tiles_dtype);
    const size_t out_bytes = (size_t)F * NY * NX * esize_of(out_dtype);
    if (overlaps(tiles_dev, tiles_bytes, out_dev, out_bytes)) return fail(RL_ERR_INVALID, "the output overlaps the tile store");
    HIP_TRY(hipSetDevice(ctx->device));
    char* base = nullptr;
    RL_TRY(tile_workspace(ctx, total, &base));
    HIP_TRY(hipMemcpyAsync(base, stage.data(), total, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(tile_blend(tiles_dtype, out_dtype, tiles_dev, out_dev, (const int32_t*)base, (const int32_t*)(base + o_ox),
                       (const double*)(base + o_wy), (const double*)(base + o_wx), (const int32_t*)(base + o_fy),
                       (const int32_t*)(base + o_cy), (const int32_t*)(base + o_fx), (const int32_t*)(base + o_cx), F, NY, NX, ny_tiles,
                       nx_tiles, ty, tx, ctx->stream));
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
