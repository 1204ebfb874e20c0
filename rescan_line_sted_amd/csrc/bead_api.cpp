// bead_api.cpp -- C ABI of the bead peak finder (include/rlsted.h rl_find_peaks): validation, the chunking of the images under the
// workspace cap and the launches of bead_kernels.hip.  Only the taps and the offsets go up; the levels, the counts and the first cap
// candidates of every image come down.  No kernel is launched on bad arguments.
#include <algorithm>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "bead_kernels.hpp"

using namespace rl;

namespace {
constexpr long long kMaxGrid = 0x7fffffffll;
}  // namespace

extern "C" int rl_find_peaks_chunk_bytes(rl_ctx* ctx, size_t bytes) {
    if (!ctx || bytes < 1) return fail(RL_ERR_INVALID, "NULL context or a cap of 0 bytes");
    ctx->beads_cap = bytes;
    return RL_OK;
}

extern "C" int rl_find_peaks(rl_ctx* ctx, const void* src_dev, int src_dtype, const int64_t* offsets, int n, int ny, int nx,
                             const double* taps, int h, int r, int b, double rel, double threshold, int cap, int32_t* yx_out,
                             double* s_out, double* x_out, int64_t* count_out, double* levels_out) {
    if (!ctx || !src_dev || !offsets || !taps || !yx_out || !s_out || !x_out || !count_out || !levels_out)
        return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(src_dtype)) return fail(RL_ERR_INVALID, "src_dtype must be RL_F32 or RL_F64");
    if (n < 1) return fail(RL_ERR_INVALID, "n must be at least 1");
    if (h < 0 || h > kBpMaxH) return fail(RL_ERR_INVALID, "h must lie in 0 .. 16");
    if (r < 1 || r > kBpMaxR) return fail(RL_ERR_INVALID, "the suppression radius must lie in 1 .. 16");
    if (b < h + r) return fail(RL_ERR_INVALID, "the border must be at least h + r");
    if ((long long)ny < 2LL * b + 1 || (long long)nx < 2LL * b + 1)
        return fail(RL_ERR_INVALID, "an image must be at least 2 b + 1 pixels on each axis");
    if (cap < 1) return fail(RL_ERR_INVALID, "cap must be at least 1");
    for (int i = 0; i < n; ++i)
        if (offsets[i] < 0) return fail(RL_ERR_INVALID, "image " + std::to_string(i) + ": negative offset");
    static_assert(kBpLevels == RL_PEAK_LEVELS, "the header's field count");
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets are copied as they are");
    HIP_TRY(hipSetDevice(ctx->device));
    const int ndy = ny - 2 * b, ndx = nx - 2 * b;
    BpArgs a;
    a.src = src_dev; a.f64 = src_dtype == RL_F64; a.ny = ny; a.nx = nx; a.h = h; a.r = r; a.b = b; a.cap = cap;
    a.rel = rel; a.threshold = threshold;
    a.nty = (ndy + kBpTY - 1) / kBpTY;
    a.ntx = (ndx + kBpTX - 1) / kBpTX;
    const long long tiles = (long long)a.nty * a.ntx;
    if (tiles > kMaxGrid) return fail(RL_ERR_INVALID, "the image has more tiles than a launch can hold");
    // what one image takes of the workspace: its tile partials, mask, and the cap candidates' positions and two values
    const size_t part_n = (size_t)tiles * 2, mask_n = (size_t)ndy * a.ntx, yx_n = (size_t)cap * 2, val_n = (size_t)cap;
    WorkLayout one;
    one.add<double>(part_n);
    one.add<unsigned>(mask_n);
    one.add<int>(yx_n);
    one.add<double>(val_n, 2);
    size_t chunk = chunk_under(ctx->beads_cap, one.bytes(), (size_t)n);
    chunk = std::min<size_t>(chunk, (size_t)(kMaxGrid / tiles));
    WorkLayout lay;
    const auto r_taps = lay.add<double>((size_t)(2 * h + 1));
    const auto r_off = lay.add<long long>((size_t)n);
    const auto r_lev = lay.add<double>(chunk * kBpLevels);
    const auto r_cnt = lay.add<long long>(chunk);
    // (each of these holds chunk padded per-image slots; the kernels index it [img][...] with the unpadded strides, which fit)
    const auto r_part = lay.add<double>(part_n, chunk);
    const auto r_mask = lay.add<unsigned>(mask_n, chunk);
    const auto r_yx = lay.add<int>(yx_n, chunk);
    const auto r_sv = lay.add<double>(val_n, chunk), r_xv = lay.add<double>(val_n, chunk);
    char* w = nullptr;
    RL_TRY(ctx->beads.reserve(ctx->stream, lay.bytes(), &w));
    double* w_dev = r_taps.at(w);
    long long* off_dev = r_off.at(w);
    a.w = w_dev;
    a.levels = r_lev.at(w); a.count = r_cnt.at(w);
    a.part = r_part.at(w); a.mask = r_mask.at(w); a.yx = r_yx.at(w); a.sv = r_sv.at(w); a.xv = r_xv.at(w);
    HIP_TRY(hipMemcpyAsync(w_dev, taps, (size_t)(2 * h + 1) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(off_dev, offsets, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    std::vector<double> lev(chunk * kBpLevels), sv(chunk * (size_t)cap), xv(chunk * (size_t)cap);
    std::vector<long long> cnt(chunk);
    std::vector<int> yx(chunk * (size_t)cap * 2);
    int& trips = ctx->chunks_run[RL_CHUNK_BEADS] = 0;
    for (size_t first = 0; first < (size_t)n; first += chunk) {
        const size_t m = std::min(chunk, (size_t)n - first);
        ++trips;
        a.off = off_dev + first;
        a.n = (int)m;
        HIP_TRY(find_peaks(a, ctx->stream));
        HIP_TRY(hipMemcpyAsync(lev.data(), a.levels, m * kBpLevels * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(cnt.data(), a.count, m * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(yx.data(), a.yx, m * (size_t)cap * 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(sv.data(), a.sv, m * (size_t)cap * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(xv.data(), a.xv, m * (size_t)cap * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < m; ++i) {
            const size_t g = first + i, k = (size_t)std::min<long long>(cnt[i], cap);
            std::copy(lev.begin() + i * kBpLevels, lev.begin() + (i + 1) * kBpLevels, levels_out + g * kBpLevels);
            count_out[g] = cnt[i];
            std::copy(yx.begin() + i * cap * 2, yx.begin() + i * cap * 2 + k * 2, yx_out + g * cap * 2);
            std::copy(sv.begin() + i * cap, sv.begin() + i * cap + k, s_out + g * cap);
            std::copy(xv.begin() + i * cap, xv.begin() + i * cap + k, x_out + g * cap);
        }
    }
    return RL_OK;
}
