// calib_api.cpp -- C ABI of the camera calibration (include/rlsted.h: rl_calib_*, rl_repair_pixels): validation, the accumulators of
// one sensor window, the defect list staged in the context's workspace, and the launches of calib_kernels.hip.  No kernel is
// launched on bad arguments.
#include <string>
#include <vector>

#include "ctx.hpp"
#include "calib_kernels.hpp"
#include "ingest_kernels.hpp"

using namespace rl;

struct rl_calib {
    rl_ctx* ctx = nullptr;
    int raw_dtype = 0, src_ny = 0, src_pitch = 0, y0 = 0, x0 = 0, ny = 0, nx = 0;
    long long frames = 0;
    void *sum = nullptr, *sumsq = nullptr;   // [ny][nx] of 8 bytes each: int64 / uint64, or float64 for f32 raw
    size_t n_pix() const { return (size_t)ny * nx; }
    bool integer() const { return raw_dtype != RL_RAW_F32; }
};

namespace {
bool raw_ok(int d) { return d == RL_RAW_U8 || d == RL_RAW_U16 || d == RL_RAW_I16 || d == RL_RAW_F32; }

int calib_clear(rl_calib* c) {
    HIP_TRY(hipMemsetAsync(c->sum, 0, c->n_pix() * 8, c->ctx->stream));
    HIP_TRY(hipMemsetAsync(c->sumsq, 0, c->n_pix() * 8, c->ctx->stream));
    c->frames = 0;
    return RL_OK;
}
}  // namespace

extern "C" int rl_calib_destroy(rl_calib* c) {
    if (!c) return RL_OK;
    if (c->ctx) {
        (void)hipSetDevice(c->ctx->device);
        (void)hipStreamSynchronize(c->ctx->stream);
    }
    if (c->sum) (void)hipFree(c->sum);
    if (c->sumsq) (void)hipFree(c->sumsq);
    delete c;
    return RL_OK;
}

extern "C" int rl_calib_create(rl_ctx* ctx, int raw_dtype, int src_ny, int src_pitch, int y0, int x0, int ny, int nx, rl_calib** out) {
    if (!ctx || !out) return fail(RL_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (!raw_ok(raw_dtype)) return fail(RL_ERR_INVALID, "raw_dtype must be one of RL_RAW_*");
    if (src_ny < 1 || src_pitch < 1 || ny < 1 || nx < 1) return fail(RL_ERR_INVALID, "src_ny, src_pitch, ny and nx must be at least 1");
    if (y0 < 0 || x0 < 0 || y0 > src_ny - ny || x0 > src_pitch - nx) return fail(RL_ERR_INVALID, "the window overhangs the sensor frame");
    HIP_TRY(hipSetDevice(ctx->device));
    rl_calib* c = new rl_calib;
    c->ctx = ctx;
    c->raw_dtype = raw_dtype; c->src_ny = src_ny; c->src_pitch = src_pitch; c->y0 = y0; c->x0 = x0; c->ny = ny; c->nx = nx;
    int rc = RL_OK;
    if (hipMalloc(&c->sum, c->n_pix() * 8) != hipSuccess || hipMalloc(&c->sumsq, c->n_pix() * 8) != hipSuccess)
        rc = fail(RL_ERR_HIP, "hipMalloc of the accumulators failed");
    if (rc == RL_OK) rc = calib_clear(c);
    if (rc != RL_OK) {
        const std::string why = rl::last_error();
        (void)hipGetLastError();
        (void)rl_calib_destroy(c);
        return fail(rc, why);
    }
    *out = c;
    return RL_OK;
}

extern "C" int rl_calib_accumulate(rl_calib* c, const void* raw_dev, int n_frames) {
    if (!c || !raw_dev) return fail(RL_ERR_INVALID, "NULL argument");
    if (n_frames < 1) return fail(RL_ERR_INVALID, "n_frames must be at least 1");
    if (!calib_frames_ok(c->integer(), c->frames, n_frames))
        return fail(RL_ERR_INVALID, "an accumulator of an integer raw type holds at most " + std::to_string(kCalibMaxFrames) + " frames");
    HIP_TRY(hipSetDevice(c->ctx->device));
    HIP_TRY(calib_accumulate(c->raw_dtype, raw_dev, c->sum, c->sumsq, c->src_ny, c->src_pitch, c->y0, c->x0, c->ny, c->nx, n_frames, c->ctx->stream));
    c->frames += n_frames;
    return RL_OK;
}

extern "C" int rl_calib_frames(const rl_calib* c, long long* frames) {
    if (!c || !frames) return fail(RL_ERR_INVALID, "NULL argument");
    *frames = c->frames;
    return RL_OK;
}

extern "C" int rl_calib_sums(rl_calib* c, void* sum_host, void* sumsq_host) {
    if (!c || (!sum_host && !sumsq_host)) return fail(RL_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(c->ctx->device));
    HIP_TRY(hipStreamSynchronize(c->ctx->stream));
    if (sum_host) HIP_TRY(hipMemcpy(sum_host, c->sum, c->n_pix() * 8, hipMemcpyDeviceToHost));
    if (sumsq_host) HIP_TRY(hipMemcpy(sumsq_host, c->sumsq, c->n_pix() * 8, hipMemcpyDeviceToHost));
    return RL_OK;
}

extern "C" int rl_calib_finalize(rl_calib* c, double* mean_dev, double* var_dev) {
    if (!c || (!mean_dev && !var_dev)) return fail(RL_ERR_INVALID, "NULL argument");
    if (c->frames < 1) return fail(RL_ERR_INVALID, "no frame has been accumulated");
    if (mean_dev && var_dev && overlaps(mean_dev, c->n_pix() * 8, var_dev, c->n_pix() * 8))
        return fail(RL_ERR_INVALID, "the two maps overlap");
    HIP_TRY(hipSetDevice(c->ctx->device));
    HIP_TRY(calib_finalize(c->raw_dtype, c->sum, c->sumsq, c->frames, c->n_pix(), mean_dev, var_dev, c->ctx->stream));
    return RL_OK;
}

extern "C" int rl_calib_reset(rl_calib* c) {
    if (!c) return fail(RL_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(c->ctx->device));
    return calib_clear(c);
}

extern "C" int rl_repair_pixels(rl_ctx* ctx, void* img_dev, int dtype, int n_images, int ny, int nx, const unsigned char* mask_host,
                                int radius, long long* unrepaired) {
    if (!ctx || !img_dev || !mask_host) return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(dtype)) return fail(RL_ERR_INVALID, "dtype must be RL_F32 or RL_F64");
    if (n_images < 1 || ny < 1 || nx < 1) return fail(RL_ERR_INVALID, "n_images, ny and nx must be at least 1");
    if ((size_t)ny * (size_t)nx > 0x7fffffffull) return fail(RL_ERR_INVALID, "an image of more than 2^31 - 1 pixels");
    if (radius < 1 || radius > kRepairMaxRadius) return fail(RL_ERR_INVALID, "radius must lie in 1 .. 3");
    std::vector<RepairEntry> list;
    long long left = 0;
    repair_list(mask_host, ny, nx, radius, list, nullptr, &left);
    if (unrepaired)
        for (int i = 0; i < n_images; ++i) unrepaired[i] = left;
    if (list.empty()) return RL_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    WorkLayout lay;
    const auto r_list = lay.add<RepairEntry>(list.size());
    char* base = nullptr;
    RL_TRY(ctx->calib.reserve(ctx->stream, lay.bytes(), &base));
    HIP_TRY(hipMemcpyAsync(r_list.at(base), list.data(), r_list.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // (the list goes away with this call)
    HIP_TRY(repair(dtype, img_dev, n_images, (size_t)ny * nx, nx, r_list.at(base), (int)list.size(), ctx->stream));
    return RL_OK;
}
