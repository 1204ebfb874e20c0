// ensemble_api.cpp -- C ABI of the per-pixel ensemble statistics of device-resident images (include/rlsted.h, rl_ensemble_stats):
// the host side -- validation, the offset tables' upload, the launches of ensemble_kernels.hip in chunks of groups, the download
// of n_groups * RL_ENSEMBLE_FIELDS doubles.
#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "ensemble_kernels.hpp"

using namespace rl;

static_assert(kEnsembleFields == RL_ENSEMBLE_FIELDS, "the header's field count is the kernels'");

namespace {
constexpr int kEnsembleMaxGroupsPerLaunch = 65535;   // grid.y
}  // namespace

extern "C" int rl_ensemble_stats(rl_ctx* ctx, const void* src_dev, int src_dtype, const int64_t* member_offsets, const int32_t* group_ptr,
                                 int n_groups, const void* truth_dev, int truth_dtype, const int64_t* truth_offsets,
                                 const double* truth_scale, size_t n_pixels, double* mean_dev, double* var_dev, double* out) {
    if (!ctx || !src_dev || !member_offsets || !group_ptr || !out) return fail(RL_ERR_INVALID, "NULL argument");
    if (n_groups < 1) return fail(RL_ERR_INVALID, "n_groups < 1");
    if (n_pixels < 1) return fail(RL_ERR_INVALID, "n_pixels < 1");
    if (!dtype_ok(src_dtype)) return fail(RL_ERR_INVALID, "src_dtype must be RL_F32 or RL_F64");
    if (truth_dev && !dtype_ok(truth_dtype)) return fail(RL_ERR_INVALID, "truth_dtype must be RL_F32 or RL_F64");
    if (truth_dev && !truth_offsets) return fail(RL_ERR_INVALID, "a truth buffer without truth_offsets");
    if (group_ptr[0] < 0) return fail(RL_ERR_INVALID, "group_ptr[0] < 0");
    for (int g = 0; g < n_groups; ++g)
        if (group_ptr[g + 1] <= group_ptr[g]) return fail(RL_ERR_INVALID, "an empty or decreasing group_ptr range");
    const size_t members = (size_t)group_ptr[n_groups];
    int64_t lo = member_offsets[group_ptr[0]], hi = lo;
    for (size_t m = (size_t)group_ptr[0]; m < members; ++m) {
        if (member_offsets[m] < 0) return fail(RL_ERR_INVALID, "negative member offset");
        lo = std::min(lo, member_offsets[m]);
        hi = std::max(hi, member_offsets[m]);
    }
    if (truth_dev)
        for (int g = 0; g < n_groups; ++g)
            if (truth_offsets[g] < 0) return fail(RL_ERR_INVALID, "negative truth offset");
    const size_t esize = dtype_size(src_dtype);
    const char* s0 = (const char*)src_dev + (size_t)lo * esize;
    const size_t s_bytes = ((size_t)hi - (size_t)lo + n_pixels) * esize;
    const size_t map_bytes = (size_t)n_groups * n_pixels * sizeof(double);
    if ((mean_dev && overlaps(s0, s_bytes, mean_dev, map_bytes)) || (var_dev && overlaps(s0, s_bytes, var_dev, map_bytes)))
        return fail(RL_ERR_INVALID, "a map overlaps the member images");
    HIP_TRY(hipSetDevice(ctx->device));

    const int nb = ensemble_blocks(n_pixels, esize);
    WorkLayout lay;
    const auto r_off = lay.add<int64_t>(members);
    const auto r_ptr = lay.add<int32_t>((size_t)n_groups + 1);
    const auto r_toff = lay.add<int64_t>((size_t)n_groups);
    const auto r_scale = lay.add<double>((size_t)n_groups);
    const size_t b_tables = lay.bytes();   // the four tables, then what the device alone writes
    const auto r_part = lay.add<double>((size_t)n_groups * nb * kEnsembleSums);
    const auto r_out = lay.add<double>((size_t)n_groups * kEnsembleFields);
    char* base = nullptr;
    RL_TRY(ctx->ensemble.reserve(ctx->stream, lay.bytes(), &base));
    int64_t *d_off = r_off.at(base), *d_toff = r_toff.at(base);
    int32_t* d_ptr = r_ptr.at(base);
    double *d_scale = r_scale.at(base), *d_part = r_part.at(base), *d_out = r_out.at(base);

    // the four tables go up in ONE copy, staged in the device layout (a pageable source: the copy has left it when it returns)
    std::vector<char> stage(b_tables, 0);
    std::copy(member_offsets, member_offsets + members, r_off.at(stage.data()));
    std::copy(group_ptr, group_ptr + n_groups + 1, r_ptr.at(stage.data()));
    if (truth_dev) {
        std::copy(truth_offsets, truth_offsets + n_groups, r_toff.at(stage.data()));
        double* sc = r_scale.at(stage.data());
        for (int g = 0; g < n_groups; ++g) sc[g] = truth_scale ? truth_scale[g] : 1.0;
    }
    HIP_TRY(hipMemcpyAsync(base, stage.data(), b_tables, hipMemcpyHostToDevice, ctx->stream));
    for (int g0 = 0; g0 < n_groups; g0 += kEnsembleMaxGroupsPerLaunch) {
        const int ng = std::min(kEnsembleMaxGroupsPerLaunch, n_groups - g0);
        HIP_TRY(ensemble_stats(src_dtype, truth_dtype, src_dev, d_off, d_ptr, truth_dev, d_toff, d_scale, mean_dev, var_dev, d_part,
                               n_pixels, g0, ng, ctx->stream));
    }
    HIP_TRY(ensemble_totals(src_dtype, d_part, d_ptr, n_pixels, n_groups, d_out, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n_groups * kEnsembleFields * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RL_OK;
}
