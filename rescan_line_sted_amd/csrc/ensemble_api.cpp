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

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int ensemble_workspace(rl_ctx* ctx, size_t bytes, char** out) {
    if (bytes > ctx->ensemble.work_bytes) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->ensemble.work) (void)hipFree(ctx->ensemble.work);
        ctx->ensemble.work = nullptr;
        ctx->ensemble.work_bytes = 0;
        HIP_TRY(hipMalloc(&ctx->ensemble.work, bytes));
        ctx->ensemble.work_bytes = bytes;
    }
    *out = (char*)ctx->ensemble.work;
    return RL_OK;
}

bool overlaps(const char* a0, const char* a1, const void* b, size_t bytes) {
    return b && (const char*)b < a1 && a0 < (const char*)b + bytes;
}
}  // namespace

extern "C" int rl_ensemble_stats(rl_ctx* ctx, const void* src_dev, int src_dtype, const int64_t* member_offsets, const int32_t* group_ptr,
                                 int n_groups, const void* truth_dev, int truth_dtype, const int64_t* truth_offsets,
                                 const double* truth_scale, size_t n_pixels, double* mean_dev, double* var_dev, double* out) {
    if (!ctx || !src_dev || !member_offsets || !group_ptr || !out) return fail(RL_ERR_INVALID, "NULL argument");
    if (n_groups < 1) return fail(RL_ERR_INVALID, "n_groups < 1");
    if (n_pixels < 1) return fail(RL_ERR_INVALID, "n_pixels < 1");
    if (src_dtype != RL_F32 && src_dtype != RL_F64) return fail(RL_ERR_INVALID, "src_dtype must be RL_F32 or RL_F64");
    if (truth_dev && truth_dtype != RL_F32 && truth_dtype != RL_F64) return fail(RL_ERR_INVALID, "truth_dtype must be RL_F32 or RL_F64");
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
    const size_t esize = src_dtype == RL_F32 ? sizeof(float) : sizeof(double);
    const char* s0 = (const char*)src_dev + (size_t)lo * esize;
    const char* s1 = (const char*)src_dev + ((size_t)hi + n_pixels) * esize;
    const size_t map_bytes = (size_t)n_groups * n_pixels * sizeof(double);
    if (overlaps(s0, s1, mean_dev, map_bytes) || overlaps(s0, s1, var_dev, map_bytes))
        return fail(RL_ERR_INVALID, "a map overlaps the member images");
    HIP_TRY(hipSetDevice(ctx->device));

    const int nb = ensemble_blocks(n_pixels, esize);
    const size_t b_off = round_up(members * 8, 256), b_ptr = round_up(((size_t)n_groups + 1) * 4, 256);
    const size_t b_grp = round_up((size_t)n_groups * 8, 256);
    const size_t b_part = round_up((size_t)n_groups * nb * kEnsembleSums * sizeof(double), 256);
    const size_t b_out = round_up((size_t)n_groups * kEnsembleFields * sizeof(double), 256);
    char* base = nullptr;
    RL_TRY(ensemble_workspace(ctx, b_off + b_ptr + 2 * b_grp + b_part + b_out, &base));
    int64_t* d_off = (int64_t*)base;
    int32_t* d_ptr = (int32_t*)(base + b_off);
    int64_t* d_toff = (int64_t*)(base + b_off + b_ptr);
    double* d_scale = (double*)(base + b_off + b_ptr + b_grp);
    double* d_part = (double*)(base + b_off + b_ptr + 2 * b_grp);
    double* d_out = (double*)(base + b_off + b_ptr + 2 * b_grp + b_part);

    // the four tables go up in ONE copy, staged in the device layout (a pageable source: the copy has left it when it returns)
    const size_t b_tables = b_off + b_ptr + 2 * b_grp;
    std::vector<char> stage(b_tables, 0);
    std::copy(member_offsets, member_offsets + members, (int64_t*)stage.data());
    std::copy(group_ptr, group_ptr + n_groups + 1, (int32_t*)(stage.data() + b_off));
    if (truth_dev) {
        std::copy(truth_offsets, truth_offsets + n_groups, (int64_t*)(stage.data() + b_off + b_ptr));
        double* sc = (double*)(stage.data() + b_off + b_ptr + b_grp);
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
