// ring_api.cpp -- C ABI of the per-ring spectrum statistics of device-resident image pairs (include/rlsted.h, rl_ring_stats) and of
// their angle-resolved form (rl_ring_sector_stats): the host side -- the ring table (built once per (ny, nx, n_rings) and context)
// or the sector table (per (ny, nx, n_rings, n_sectors)), the chunking under the workspace cap, the launches of ring_kernels.hip
// and ring_sector_kernels.hip.  Only offsets and scales go up and n_pairs * n_rings [* n_sectors] * RL_RING_FIELDS doubles come down.
#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "ring_kernels.hpp"

using namespace rl;

namespace {
constexpr int kRingMaxPairsPerLaunch = 65535;   // grid.z
constexpr int kRingMaxRings = 4 * kRingMaxN;

int upload_table(const std::vector<int>& row_ptr, const std::vector<int>& bins, rl_ctx::RingTable* t) {
    HIP_TRY(hipMalloc((void**)&t->row_ptr, row_ptr.size() * sizeof(int)));
    hipError_t e = hipMalloc((void**)&t->bins, std::max<size_t>(bins.size(), 1) * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(t->row_ptr, row_ptr.data(), row_ptr.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess && !bins.empty()) e = hipMemcpy(t->bins, bins.data(), bins.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(t->row_ptr);
        if (t->bins) (void)hipFree(t->bins);
        return fail(RL_ERR_HIP, std::string("ring table: ") + hipGetErrorString(e));
    }
    return RL_OK;
}

int ring_table(rl_ctx* ctx, int ny, int nx, int n_rings, rl_ctx::RingTable* out) {
    const auto key = std::make_pair(std::make_pair(ny, nx), n_rings);
    auto it = ctx->ring.tables.find(key);
    if (it != ctx->ring.tables.end()) {
        *out = it->second;
        return RL_OK;
    }
    std::vector<int> row_ptr, bins;
    ring_build_table(ny, nx, n_rings, row_ptr, bins);
    rl_ctx::RingTable t;
    RL_TRY(upload_table(row_ptr, bins, &t));
    ctx->ring.tables[key] = t;
    *out = t;
    return RL_OK;
}

int sector_table(rl_ctx* ctx, int ny, int nx, int n_rings, int n_sectors, rl_ctx::RingTable* out) {
    const auto key = std::make_pair(std::make_pair(ny, nx), std::make_pair(n_rings, n_sectors));
    auto it = ctx->ring.sector_tables.find(key);
    if (it != ctx->ring.sector_tables.end()) {
        *out = it->second;
        return RL_OK;
    }
    std::vector<int> cell_ptr, bins;
    if (!ring_build_sector_table(ny, nx, n_rings, n_sectors, cell_ptr, bins))
        return fail(RL_ERR_UNSUPPORTED, "a bin lies within 2^-30 of a sector boundary that is no multiple of 45 degrees");
    rl_ctx::RingTable t;
    RL_TRY(upload_table(cell_ptr, bins, &t));
    ctx->ring.sector_tables[key] = t;
    *out = t;
    return RL_OK;
}

// both entry points: n_sectors = 0 is rl_ring_stats (the ring table, k_ring_reduce), n_sectors >= 1 rl_ring_sector_stats (the
// sector table, k_ring_reduce_sectors, n_sectors times the result); everything else is one path
int ring_run(rl_ctx* ctx, const void* a_dev, int a_dtype, const int64_t* a_offsets, const void* b_dev, int b_dtype,
             const int64_t* b_offsets, const double* b_scale, int n_pairs, int ny, int nx, int n_rings, int n_sectors, double* out) {
    if (!ctx || !a_dev || !a_offsets || !b_dev || !b_offsets || !out) return fail(RL_ERR_INVALID, "NULL argument");
    if (n_pairs < 1) return fail(RL_ERR_INVALID, "n_pairs < 1");
    if (ny < 2 || nx < 2) return fail(RL_ERR_INVALID, "ny and nx must be at least 2");
    if (n_rings < 1) return fail(RL_ERR_INVALID, "n_rings < 1");
    if (!dtype_ok(a_dtype) || !dtype_ok(b_dtype)) return fail(RL_ERR_INVALID, "dtype must be RL_F32 or RL_F64");
    if (ny > kRingMaxN || nx > kRingMaxN) return fail(RL_ERR_UNSUPPORTED, "ring statistics cover images up to 4096 x 4096");
    if (n_rings > kRingMaxRings) return fail(RL_ERR_UNSUPPORTED, "more than 16384 rings");
    if (n_sectors > kRingMaxSectors) return fail(RL_ERR_UNSUPPORTED, "more than 64 sectors");
    for (int i = 0; i < n_pairs; ++i)
        if (a_offsets[i] < 0 || b_offsets[i] < 0) return fail(RL_ERR_INVALID, "negative image offset");
    HIP_TRY(hipSetDevice(ctx->device));

    void *wx = nullptr, *wy = nullptr;
    RL_TRY(ctx->plain_twiddles(nx, &wx));
    RL_TRY(ctx->plain_twiddles(ny, &wy));
    rl_ctx::RingTable table;
    if (n_sectors) RL_TRY(sector_table(ctx, ny, nx, n_rings, n_sectors, &table));
    else RL_TRY(ring_table(ctx, ny, nx, n_rings, &table));

    const size_t img = (size_t)ny * nx * sizeof(RingC);
    const size_t per_out = (size_t)n_rings * (n_sectors ? n_sectors : 1) * kRingFields * sizeof(double);
    // T and F of the pairs in flight (2 * 16 * ny * nx bytes per pair) stay below the cap; a single pair larger than it runs alone
    int chunk = (int)std::min<size_t>(chunk_under(ctx->ring_cap, 2 * img, (size_t)n_pairs), (size_t)kRingMaxPairsPerLaunch);
    if (n_sectors) chunk = (int)chunk_under(ctx->ring_cap, per_out, (size_t)chunk);   // the results of a chunk stay under the cap too
    WorkLayout lay;
    const auto r_aoff = lay.add<int64_t>((size_t)n_pairs), r_boff = lay.add<int64_t>((size_t)n_pairs);
    const auto r_scale = lay.add<double>((size_t)n_pairs);
    const auto r_out = lay.add<double>((size_t)chunk * per_out / sizeof(double));
    const auto r_tf = lay.add<char>(2 * (size_t)chunk * img);   // T, then F behind it without padding
    char* base = nullptr;
    RL_TRY(ctx->ring.work.reserve(ctx->stream, lay.bytes(), &base));
    int64_t *d_aoff = r_aoff.at(base), *d_boff = r_boff.at(base);
    double *d_scale = r_scale.at(base), *d_out = r_out.at(base);
    char *d_t = r_tf.at(base), *d_f = d_t + (size_t)chunk * img;

    std::vector<double> ones;
    if (!b_scale) {
        ones.assign((size_t)n_pairs, 1.0);
        b_scale = ones.data();
    }
    // (pageable sources: these copies have left the host arrays when they return)
    HIP_TRY(hipMemcpyAsync(d_aoff, a_offsets, (size_t)n_pairs * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_boff, b_offsets, (size_t)n_pairs * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_scale, b_scale, (size_t)n_pairs * 8, hipMemcpyHostToDevice, ctx->stream));
    int& trips = ctx->chunks_run[RL_CHUNK_RING] = 0;
    for (int p0 = 0; p0 < n_pairs; p0 += chunk) {
        const int np = std::min(chunk, n_pairs - p0);
        ++trips;
        HIP_TRY(ring_rows(a_dtype, b_dtype, a_dev, b_dev, d_aoff + p0, d_boff + p0, d_scale + p0, wx, d_t, ny, nx, np, ctx->stream));
        HIP_TRY(ring_cols(d_t, wy, d_f, ny, nx, np, ctx->stream));
        if (n_sectors) HIP_TRY(ring_reduce_sectors(d_f, table.row_ptr, table.bins, d_out, ny, nx, n_rings, n_sectors, np, ctx->stream));
        else HIP_TRY(ring_reduce(d_f, table.row_ptr, table.bins, d_out, ny, nx, n_rings, np, ctx->stream));
        HIP_TRY(hipMemcpyAsync((char*)out + (size_t)p0 * per_out, d_out, (size_t)np * per_out, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RL_OK;
}
}  // namespace

extern "C" {

int rl_ring_count(int ny, int nx) { return std::min(ny, nx) / 2; }

int rl_ring_stats(rl_ctx* ctx, const void* a_dev, int a_dtype, const int64_t* a_offsets, const void* b_dev, int b_dtype,
                  const int64_t* b_offsets, const double* b_scale, int n_pairs, int ny, int nx, int n_rings, double* out) {
    return ring_run(ctx, a_dev, a_dtype, a_offsets, b_dev, b_dtype, b_offsets, b_scale, n_pairs, ny, nx, n_rings, 0, out);
}

int rl_ring_sector_stats(rl_ctx* ctx, const void* a_dev, int a_dtype, const int64_t* a_offsets, const void* b_dev, int b_dtype,
                         const int64_t* b_offsets, const double* b_scale, int n_pairs, int ny, int nx, int n_rings, int n_sectors,
                         double* out) {
    if (n_sectors < 1) return fail(RL_ERR_INVALID, "n_sectors < 1");
    return ring_run(ctx, a_dev, a_dtype, a_offsets, b_dev, b_dtype, b_offsets, b_scale, n_pairs, ny, nx, n_rings, n_sectors, out);
}

}  // extern "C"
