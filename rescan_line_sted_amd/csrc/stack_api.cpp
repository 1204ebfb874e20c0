// stack_api.cpp -- C ABI of the acquired-stack path (include/rlsted.h: rl_ingest, rl_export, rl_stack_create, rl_stack_run,
// rl_stack_run_registered, rl_stack_set_defects, rl_stack_destroy, rl_device_upload_bytes): validation, the launches of ingest_kernels.hip, and the chunk
// pipeline that overlaps upload, iterations and download -- with, in the registered run, the estimates (rl_register_estimate) and
// the shift (rl_shift_images) between the ingest and the iterations.  The pipeline reaches the plan through the C ABI alone (rl_deconv_dims, rl_deconv_device_ptr,
// rl_deconv_measurement_written, rl_deconv_reset_estimate, rl_deconv_iterate), as the tiled path does.  No kernel is launched on
// bad arguments.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "calib_kernels.hpp"
#include "ingest_kernels.hpp"

using namespace rl;

namespace {
size_t raw_size(int d) { return d == RL_RAW_U8 ? 1 : (d == RL_RAW_F32 ? 4 : (d == RL_RAW_U16 || d == RL_RAW_I16 ? 2 : 0)); }
size_t out_size(int d) { return d == RL_OUT_F32 ? 4 : (d == RL_OUT_F64 ? 8 : (d == RL_OUT_U16 ? 2 : 0)); }

// the per-workgroup partials of a call's statistics, `doubles` of them, in the context's ingest workspace
int stats_partials(rl_ctx* ctx, size_t doubles, double** out) {
    WorkLayout lay;
    const auto r_part = lay.add<double>(doubles);
    char* base = nullptr;
    RL_TRY(ctx->ingest.reserve(ctx->stream, lay.bytes(), &base));
    *out = r_part.at(base);
    return RL_OK;
}

// the camera's numbers (rl_ingest's and rl_stack_create's)
int check_camera(double offset, double gain, double epsilon, double saturation) {
    if (!std::isfinite(gain) || gain <= 0.0) return fail(RL_ERR_INVALID, "gain must be positive and finite");
    if (!std::isfinite(epsilon) || epsilon < 0.0) return fail(RL_ERR_INVALID, "epsilon must be finite and at least 0");
    if (std::isnan(offset) || std::isnan(saturation)) return fail(RL_ERR_INVALID, "offset or saturation is nan");
    return RL_OK;
}

// the window (y0, x0) + ny x nx inside a frame of src_ny rows of `cols` columns
int check_window(int src_ny, int cols, int y0, int x0, int ny, int nx) {
    if (y0 < 0 || x0 < 0 || y0 > src_ny - ny || x0 > cols - nx) return fail(RL_ERR_INVALID, "the window overhangs the sensor frame");
    return RL_OK;
}

// a page-locked (or otherwise registered) host array is copied to and from directly: its first and its last byte must both be
// known to the runtime as host memory (an array that only begins in a page-locked block goes through the slots' blocks)
bool byte_is_pinned(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // (an ordinary pointer is "invalid value" to the runtime: not an error of ours)
        return false;
    }
    return a.type == hipMemoryTypeHost;
}
bool host_is_pinned(const void* p, size_t bytes) {
    return bytes > 0 && byte_is_pinned(p) && byte_is_pinned((const char*)p + bytes - 1);
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

extern "C" int rl_ingest(rl_ctx* ctx, const void* raw_dev, int raw_dtype, int src_images, int src_ny, int src_pitch, int y0, int x0,
                         long long frame_stride, long long view_stride, int n_slots, int n_valid, int V, int ny, int nx,
                         const float* dark_dev, double offset, double gain, double epsilon, double saturation, void* dst_dev,
                         int dst_dtype, double* stats_dev) {
    if (!ctx || !raw_dev || !dst_dev) return fail(RL_ERR_INVALID, "NULL argument");
    if (!raw_size(raw_dtype)) return fail(RL_ERR_INVALID, "raw_dtype must be one of RL_RAW_*");
    if (!dtype_ok(dst_dtype)) return fail(RL_ERR_INVALID, "dst_dtype must be RL_F32 or RL_F64");
    if (src_images < 1 || src_ny < 1 || src_pitch < 1 || n_slots < 1 || V < 1 || ny < 1 || nx < 1)
        return fail(RL_ERR_INVALID, "src_images, src_ny, src_pitch, n_slots, V, ny and nx must be at least 1");
    if (n_valid < 0 || n_valid > n_slots) return fail(RL_ERR_INVALID, "n_valid must lie in 0 .. n_slots");
    RL_TRY(check_window(src_ny, src_pitch, y0, x0, ny, nx));
    RL_TRY(check_camera(offset, gain, epsilon, saturation));
    if (n_valid > 0) {   // the index is linear in (slot, view): its extremes are at the corners
        for (int b : {0, n_valid - 1})
            for (int v : {0, V - 1}) {
                const __int128 i = (__int128)b * frame_stride + (__int128)v * view_stride;
                if (i < 0 || i >= src_images)
                    return fail(RL_ERR_INVALID, "slot " + std::to_string(b) + ", view " + std::to_string(v) + ": source image out of range");
            }
    }
    const size_t src_bytes = (size_t)src_images * src_ny * src_pitch * raw_size(raw_dtype);
    const size_t images = (size_t)n_slots * V, dst_bytes = images * ny * nx * dtype_size(dst_dtype);
    if (overlaps(raw_dev, src_bytes, dst_dev, dst_bytes)) return fail(RL_ERR_INVALID, "the destination overlaps the source");
    if (dark_dev && overlaps(dark_dev, (size_t)ny * nx * sizeof(float), dst_dev, dst_bytes))
        return fail(RL_ERR_INVALID, "the destination overlaps the dark map");
    if (stats_dev && overlaps(stats_dev, images * kIngestFields * sizeof(double), dst_dev, dst_bytes))
        return fail(RL_ERR_INVALID, "the destination overlaps the statistics");
    static_assert(kIngestFields == RL_INGEST_FIELDS && kExportFields == RL_EXPORT_FIELDS, "the header's field counts");
    static_assert(RAW_U8 == RL_RAW_U8 && RAW_U16 == RL_RAW_U16 && RAW_I16 == RL_RAW_I16 && RAW_F32 == RL_RAW_F32, "the header's codes");
    HIP_TRY(hipSetDevice(ctx->device));
    IngestArgs a;
    a.raw = raw_dev; a.dst = dst_dev; a.dark = dark_dev; a.part = nullptr; a.stats = stats_dev;
    a.frame_stride = frame_stride; a.view_stride = view_stride;
    a.src_ny = src_ny; a.src_pitch = src_pitch; a.y0 = y0; a.x0 = x0; a.n_slots = n_slots; a.n_valid = n_valid; a.V = V; a.ny = ny; a.nx = nx;
    a.offset = offset; a.gain = gain; a.epsilon = epsilon; a.saturation = saturation;
    if (stats_dev) RL_TRY(stats_partials(ctx, images * ingest_blocks(ingest_vectors(ny, nx)) * kIngestFields, &a.part));
    HIP_TRY(ingest(raw_dtype, dst_dtype, a, ctx->stream));
    return RL_OK;
}

extern "C" int rl_export(rl_ctx* ctx, const void* est_dev, int est_dtype, int n, int ny, int nx, double scale, void* out_dev,
                         int out_dtype, double* stats_dev) {
    if (!ctx || !est_dev || !out_dev) return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(est_dtype)) return fail(RL_ERR_INVALID, "est_dtype must be RL_F32 or RL_F64");
    if (!out_size(out_dtype)) return fail(RL_ERR_INVALID, "out_dtype must be one of RL_OUT_*");
    if (n < 1 || ny < 1 || nx < 1) return fail(RL_ERR_INVALID, "n, ny and nx must be at least 1");
    if (std::isnan(scale)) return fail(RL_ERR_INVALID, "scale is nan");
    static_assert(OUT_F32 == RL_OUT_F32 && OUT_F64 == RL_OUT_F64 && OUT_U16 == RL_OUT_U16, "the header's codes");
    const size_t n_pix = (size_t)ny * nx, est_bytes = (size_t)n * n_pix * dtype_size(est_dtype), out_bytes = (size_t)n * n_pix * out_size(out_dtype);
    if (overlaps(est_dev, est_bytes, out_dev, out_bytes)) return fail(RL_ERR_INVALID, "the output overlaps the estimates");
    if (stats_dev && overlaps(stats_dev, (size_t)n * kExportFields * sizeof(double), out_dev, out_bytes))
        return fail(RL_ERR_INVALID, "the output overlaps the statistics");
    HIP_TRY(hipSetDevice(ctx->device));
    ExportArgs a;
    a.est = est_dev; a.out = out_dev; a.part = nullptr; a.stats = stats_dev; a.n = n; a.n_pix = n_pix; a.scale = scale;
    if (stats_dev) RL_TRY(stats_partials(ctx, (size_t)n * ingest_blocks(export_vectors(n_pix)) * kExportFields, &a.part));
    HIP_TRY(export_estimates(est_dtype, out_dtype, a, ctx->stream));
    return RL_OK;
}

// ---- the pipeline ----------------------------------------------------------------------------------------------------------------
struct rl_stack {
    rl_deconv* plan = nullptr;
    rl_ctx* ctx = nullptr;
    rl_stack_params prm{};
    int B = 0, V = 0, ny = 0, nx = 0, dtype = RL_F32;
    void *meas = nullptr, *est = nullptr;   // the plan's buffers
    float* dark = nullptr;                  // device [ny][nx]
    hipStream_t in = nullptr, out = nullptr;
    // A chunk's blocks.  host_raw / dev_raw: B * V sensor frames; dev_out / host_out: B images of out_dtype followed (256-byte
    // aligned) by the chunk's statistics, [B * V][4] then [B][2] float64, so that ONE copy brings both back.
    struct Slot {
        char *host_raw = nullptr, *dev_raw = nullptr, *dev_out = nullptr, *host_out = nullptr;
        hipEvent_t up0 = nullptr, uploaded = nullptr, freed = nullptr, c0 = nullptr, exported = nullptr, dn0 = nullptr, downloaded = nullptr;
        bool used = false;
    } slot[2];
    size_t frame_elems() const { return (size_t)prm.src_ny * prm.src_pitch; }
    size_t raw_bytes() const { return (size_t)B * V * frame_elems() * raw_size(prm.raw_dtype); }
    size_t image_bytes() const { return (size_t)ny * nx * out_size(prm.out_dtype); }
    size_t stats_offset() const { return round_up((size_t)B * image_bytes(), 256); }
    size_t stats_bytes() const { return ((size_t)B * V * kIngestFields + (size_t)B * kExportFields) * sizeof(double); }
    size_t out_bytes() const { return stats_offset() + stats_bytes(); }
    // rl_stack_run_registered's buffers, allocated on first use: staging [B][V][ny][nx] and refs [V][ny][nx] of the plan's dtype,
    // scratch B * V float64 images
    void *staging = nullptr, *refs = nullptr;
    double* scratch = nullptr;
    // rl_stack_set_defects: the device list of the repairable defects of the plan's window (calib_kernels.hpp), or none
    RepairEntry* defects = nullptr;
    int n_defects = 0;
    // the repair of a chunk's B * V ingested images at `img`, on the context's stream (nothing is enqueued without defects)
    int repair_chunk(void* img) {
        if (!n_defects) return RL_OK;
        HIP_TRY(repair(dtype, img, B * V, (size_t)ny * nx, nx, defects, n_defects, ctx->stream));
        return RL_OK;
    }
};

namespace {
struct Chunk {
    int first, nt;
    rl_stack::Slot* sl;
};

// chunk c: raw_host -> the slot's device raw buffer, on the copy-in stream
int stack_upload(rl_stack* st, const Chunk& c, const char* raw, bool direct, int n_frames) {
    rl_stack::Slot& sl = *c.sl;
    if (sl.used) HIP_TRY(hipEventSynchronize(sl.freed));   // the chunk before last has consumed this block
    const size_t img = st->frame_elems() * raw_size(st->prm.raw_dtype);
    const bool by_view = st->prm.order == RL_ORDER_VIEW_FRAME;
    // FRAME_VIEW: one piece [nt][V]; VIEW_FRAME: V pieces [nt], view v of the chunk at device image v * nt
    const int pieces = by_view ? st->V : 1;
    const size_t piece = (size_t)c.nt * (by_view ? 1 : st->V) * img;
    HIP_TRY(hipEventRecord(sl.up0, st->in));
    for (int v = 0; v < pieces; ++v) {
        const char* src = raw + ((size_t)v * n_frames + (size_t)c.first * (by_view ? 1 : st->V)) * img;
        if (!direct) {
            memcpy(sl.host_raw + v * piece, src, piece);
            src = sl.host_raw + v * piece;
        }
        HIP_TRY(hipMemcpyAsync(sl.dev_raw + v * piece, src, piece, hipMemcpyHostToDevice, st->in));
    }
    HIP_TRY(hipEventRecord(sl.uploaded, st->in));
    return RL_OK;
}

// chunk c on the context's stream: ingest, the plan's iterations from ones, export
int stack_compute(rl_stack* st, const Chunk& c, int k_iters, double* times) {
    rl_stack::Slot& sl = *c.sl;
    hipStream_t s = st->ctx->stream;
    const rl_stack_params& p = st->prm;
    const bool by_view = p.order == RL_ORDER_VIEW_FRAME;
    double* stats = (double*)(sl.dev_out + st->stats_offset());
    HIP_TRY(hipStreamWaitEvent(s, sl.uploaded, 0));
    if (sl.used) HIP_TRY(hipStreamWaitEvent(s, sl.downloaded, 0));   // (the out buffer's last download; the host has waited for it too)
    HIP_TRY(hipEventRecord(sl.c0, s));
    const int rc = rl_ingest(st->ctx, sl.dev_raw, p.raw_dtype, c.nt * st->V, p.src_ny, p.src_pitch, p.y0, p.x0, by_view ? 1 : st->V,
                             by_view ? c.nt : 1, st->B, c.nt, st->V, st->ny, st->nx, st->dark, p.offset, p.gain, p.epsilon, p.saturation,
                             st->meas, st->dtype, stats);
    HIP_TRY(hipEventRecord(sl.freed, s));
    sl.used = true;
    RL_TRY(rc);
    RL_TRY(st->repair_chunk(st->meas));
    RL_TRY(rl_deconv_measurement_written(st->plan));
    RL_TRY(rl_deconv_reset_estimate(st->plan));
    RL_TRY(rl_deconv_iterate(st->plan, k_iters));
    // (the iterations have been waited for, the chunk's upload with them; the next use of this slot records these events anew)
    float up_ms = 0;
    HIP_TRY(hipEventElapsedTime(&up_ms, sl.up0, sl.uploaded));
    times[1] += up_ms;
    RL_TRY(rl_export(st->ctx, st->est, st->dtype, st->B, st->ny, st->nx, p.out_scale, sl.dev_out, p.out_dtype,
                     stats + (size_t)st->B * st->V * kIngestFields));
    HIP_TRY(hipEventRecord(sl.exported, s));
    return RL_OK;
}

// chunk c: the slot's device out buffer -> its page-locked block (or the caller's page-locked array), on the copy-out stream
int stack_download(rl_stack* st, const Chunk& c, char* out, bool direct) {
    rl_stack::Slot& sl = *c.sl;
    HIP_TRY(hipStreamWaitEvent(st->out, sl.exported, 0));
    HIP_TRY(hipEventRecord(sl.dn0, st->out));
    const size_t images = (size_t)c.nt * st->image_bytes();
    if (direct) {
        HIP_TRY(hipMemcpyAsync(out + (size_t)c.first * st->image_bytes(), sl.dev_out, images, hipMemcpyDeviceToHost, st->out));
        HIP_TRY(hipMemcpyAsync(sl.host_out + st->stats_offset(), sl.dev_out + st->stats_offset(), st->stats_bytes(), hipMemcpyDeviceToHost, st->out));
    } else if (c.nt == st->B) {
        HIP_TRY(hipMemcpyAsync(sl.host_out, sl.dev_out, st->out_bytes(), hipMemcpyDeviceToHost, st->out));   // ONE copy: images and statistics
    } else {
        HIP_TRY(hipMemcpyAsync(sl.host_out, sl.dev_out, images, hipMemcpyDeviceToHost, st->out));
        HIP_TRY(hipMemcpyAsync(sl.host_out + st->stats_offset(), sl.dev_out + st->stats_offset(), st->stats_bytes(), hipMemcpyDeviceToHost, st->out));
    }
    HIP_TRY(hipEventRecord(sl.downloaded, st->out));
    return RL_OK;
}

// chunk c has arrived: the caller's arrays, the event times
int stack_drain(rl_stack* st, const Chunk& c, char* out, bool direct, double* ingest_stats, double* export_stats, double* times) {
    rl_stack::Slot& sl = *c.sl;
    HIP_TRY(hipEventSynchronize(sl.downloaded));
    if (!direct) memcpy(out + (size_t)c.first * st->image_bytes(), sl.host_out, (size_t)c.nt * st->image_bytes());
    const double* stats = (const double*)(sl.host_out + st->stats_offset());
    if (ingest_stats)
        std::copy(stats, stats + (size_t)c.nt * st->V * kIngestFields, ingest_stats + (size_t)c.first * st->V * kIngestFields);
    if (export_stats) {
        const double* e = stats + (size_t)st->B * st->V * kIngestFields;
        std::copy(e, e + (size_t)c.nt * kExportFields, export_stats + (size_t)c.first * kExportFields);
    }
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, sl.c0, sl.exported));
    times[2] += ms;
    HIP_TRY(hipEventElapsedTime(&ms, sl.dn0, sl.downloaded));
    times[3] += ms;
    return RL_OK;
}

int stack_build(rl_stack* st) {
    HIP_TRY(hipStreamCreateWithFlags(&st->in, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&st->out, hipStreamNonBlocking));
    if (st->prm.dark) {
        const size_t bytes = (size_t)st->ny * st->nx * sizeof(float);
        HIP_TRY(hipMalloc((void**)&st->dark, bytes));
        HIP_TRY(hipMemcpy(st->dark, st->prm.dark, bytes, hipMemcpyHostToDevice));
        st->prm.dark = nullptr;   // (the caller's array may go away)
    }
    for (rl_stack::Slot& sl : st->slot) {
        HIP_TRY(hipHostMalloc((void**)&sl.host_raw, st->raw_bytes(), hipHostMallocDefault));
        HIP_TRY(hipMalloc((void**)&sl.dev_raw, st->raw_bytes()));
        HIP_TRY(hipMalloc((void**)&sl.dev_out, st->out_bytes()));
        HIP_TRY(hipHostMalloc((void**)&sl.host_out, st->out_bytes(), hipHostMallocDefault));
        for (hipEvent_t* e : {&sl.up0, &sl.uploaded, &sl.freed, &sl.c0, &sl.exported, &sl.dn0, &sl.downloaded}) HIP_TRY(hipEventCreate(e));
    }
    return RL_OK;
}
}  // namespace

extern "C" int rl_stack_destroy(rl_stack* st) {
    if (!st) return RL_OK;
    if (st->ctx) {
        (void)hipSetDevice(st->ctx->device);
        if (st->in) (void)hipStreamSynchronize(st->in);
        (void)hipStreamSynchronize(st->ctx->stream);
        if (st->out) (void)hipStreamSynchronize(st->out);
    }
    for (rl_stack::Slot& sl : st->slot) {
        if (sl.host_raw) (void)hipHostFree(sl.host_raw);
        if (sl.dev_raw) (void)hipFree(sl.dev_raw);
        if (sl.dev_out) (void)hipFree(sl.dev_out);
        if (sl.host_out) (void)hipHostFree(sl.host_out);
        for (hipEvent_t e : {sl.up0, sl.uploaded, sl.freed, sl.c0, sl.exported, sl.dn0, sl.downloaded})
            if (e) (void)hipEventDestroy(e);
    }
    if (st->dark) (void)hipFree(st->dark);
    if (st->defects) (void)hipFree(st->defects);
    for (void* p : {st->staging, st->refs, (void*)st->scratch})
        if (p) (void)hipFree(p);
    if (st->in) (void)hipStreamDestroy(st->in);
    if (st->out) (void)hipStreamDestroy(st->out);
    delete st;
    return RL_OK;
}

extern "C" int rl_stack_create(rl_deconv* plan, const rl_stack_params* params, rl_stack** out) {
    if (!plan || !params || !out) return fail(RL_ERR_INVALID, "NULL argument");
    *out = nullptr;
    const rl_stack_params& p = *params;
    if (!raw_size(p.raw_dtype)) return fail(RL_ERR_INVALID, "raw_dtype must be one of RL_RAW_*");
    if (!out_size(p.out_dtype)) return fail(RL_ERR_INVALID, "out_dtype must be one of RL_OUT_*");
    if (p.order != RL_ORDER_FRAME_VIEW && p.order != RL_ORDER_VIEW_FRAME) return fail(RL_ERR_INVALID, "order must be one of RL_ORDER_*");
    if (p.src_ny < 1 || p.src_nx < 1 || p.src_pitch < p.src_nx) return fail(RL_ERR_INVALID, "the sensor frame needs src_ny, src_nx >= 1 and src_pitch >= src_nx");
    RL_TRY(check_camera(p.offset, p.gain, p.epsilon, p.saturation));
    if (std::isnan(p.out_scale)) return fail(RL_ERR_INVALID, "out_scale is nan");
    rl_stack* st = new rl_stack;
    st->plan = plan;
    st->ctx = plan_ctx(plan);
    st->prm = p;
    int rc = rl_deconv_dims(plan, &st->B, &st->V, &st->ny, &st->nx);
    if (rc == RL_OK) rc = check_window(p.src_ny, p.src_nx, p.y0, p.x0, st->ny, st->nx);
    if (rc == RL_OK) rc = rl_deconv_device_ptr(plan, 1, &st->meas, nullptr, &st->dtype);
    if (rc == RL_OK) rc = rl_deconv_device_ptr(plan, 0, &st->est, nullptr, nullptr);
    if (rc == RL_OK && hipSetDevice(st->ctx->device) != hipSuccess) rc = fail(RL_ERR_HIP, "hipSetDevice failed");
    if (rc == RL_OK) rc = stack_build(st);
    if (rc != RL_OK) {
        const std::string why = rl::last_error();   // (the clean-up must not replace the message)
        (void)rl_stack_destroy(st);
        return fail(rc, why);
    }
    *out = st;
    return RL_OK;
}

extern "C" int rl_stack_set_defects(rl_stack* st, const unsigned char* mask_host, int radius) {
    if (!st) return fail(RL_ERR_INVALID, "NULL argument");
    if (mask_host && (radius < 1 || radius > kRepairMaxRadius)) return fail(RL_ERR_INVALID, "radius must lie in 1 .. 3");
    if ((size_t)st->ny * (size_t)st->nx > 0x7fffffffull) return fail(RL_ERR_INVALID, "an image of more than 2^31 - 1 pixels");
    HIP_TRY(hipSetDevice(st->ctx->device));
    HIP_TRY(hipStreamSynchronize(st->ctx->stream));   // (a run in flight reads the present list)
    if (st->defects) (void)hipFree(st->defects);
    st->defects = nullptr;
    st->n_defects = 0;
    if (!mask_host) return RL_OK;
    std::vector<RepairEntry> list;
    repair_list(mask_host, st->ny, st->nx, radius, list, nullptr, nullptr);
    if (list.empty()) return RL_OK;
    HIP_TRY(hipMalloc((void**)&st->defects, list.size() * sizeof(RepairEntry)));
    HIP_TRY(hipMemcpy(st->defects, list.data(), list.size() * sizeof(RepairEntry), hipMemcpyHostToDevice));
    st->n_defects = (int)list.size();
    return RL_OK;
}

namespace {
// the chunks of a run, in the order of the header's description; compute(chunk) is the context stream's part of a chunk
template <typename Compute>
int stack_chunks(rl_stack* st, const char* raw, bool raw_direct, int n_frames, char* out, bool out_direct, double* ingest_stats,
                 double* export_stats, double* times, Compute compute) {
    const int chunks = (n_frames + st->B - 1) / st->B;
    auto chunk = [&](int i) { return Chunk{i * st->B, std::min(st->B, n_frames - i * st->B), &st->slot[i % 2]}; };
    RL_TRY(stack_upload(st, chunk(0), raw, raw_direct, n_frames));
    for (int i = 0; i < chunks; ++i) {
        if (i + 1 < chunks) RL_TRY(stack_upload(st, chunk(i + 1), raw, raw_direct, n_frames));   // before chunk i iterates
        RL_TRY(compute(chunk(i)));
        RL_TRY(stack_download(st, chunk(i), out, out_direct));                                   // while chunk i + 1 iterates
        if (i > 0) RL_TRY(stack_drain(st, chunk(i - 1), out, out_direct, ingest_stats, export_stats, times));
    }
    return stack_drain(st, chunk(chunks - 1), out, out_direct, ingest_stats, export_stats, times);
}

// a failed run: copies may still be in flight -- an upload reading the caller's page-locked raw array, a download writing the
// caller's page-locked out array: they are waited for before the caller hears of the failure and may let go of either (statuses
// ignored: the first failure is the one reported)
int stack_failed(rl_stack* st, int rc) {
    const std::string why = rl::last_error();
    (void)hipStreamSynchronize(st->in);
    (void)hipStreamSynchronize(st->ctx->stream);
    (void)hipStreamSynchronize(st->out);
    (void)hipGetLastError();
    return fail(rc, why);
}

// ---- the registered run --------------------------------------------------------------------------------------------------------
struct RegRun {
    const rl_stack_register* rp;
    const double* given;            // [F][V][2] or nullptr
    rl_stack_register_out* ro;
    bool estimating;
    int M;
    double est_ms = 0.0;
    std::vector<double> view_shift; // [V][2]
};

// the pairs (reference offset, moving offset) estimated in one rl_register_estimate; shifts [n][2] and fields [n][3] come back
int stack_estimate(rl_stack* st, RegRun& r, const void* ref, const void* mov, const std::vector<int64_t>& ro, const std::vector<int64_t>& mo,
                   std::vector<double>& shifts, std::vector<double>& fields) {
    const int n = (int)mo.size();
    shifts.assign((size_t)n * 2, 0.0);
    fields.assign((size_t)n * 3, 0.0);
    return rl_register_estimate(st->ctx, ref, st->dtype, ro.data(), mov, st->dtype, mo.data(), n, st->ny, st->nx, r.rp->max_shift, r.M,
                                r.rp->refine, r.rp->refine > 0 ? st->scratch : nullptr, shifts.data(), fields.data(), nullptr);
}

// chunk c on the context's stream: ingest into the staging buffer, the estimates, the shift into the plan's measurement, the
// iterations from ones, export
int stack_compute_registered(rl_stack* st, const Chunk& c, int k_iters, RegRun& r, double* times) {
    rl_stack::Slot& sl = *c.sl;
    hipStream_t s = st->ctx->stream;
    const rl_stack_params& p = st->prm;
    const bool by_view = p.order == RL_ORDER_VIEW_FRAME;
    const int V = st->V, B = st->B;
    const size_t n_pix = (size_t)st->ny * st->nx, esz = dtype_size(st->dtype);
    double* stats = (double*)(sl.dev_out + st->stats_offset());
    HIP_TRY(hipStreamWaitEvent(s, sl.uploaded, 0));
    if (sl.used) HIP_TRY(hipStreamWaitEvent(s, sl.downloaded, 0));
    HIP_TRY(hipEventRecord(sl.c0, s));
    const int rc = rl_ingest(st->ctx, sl.dev_raw, p.raw_dtype, c.nt * V, p.src_ny, p.src_pitch, p.y0, p.x0, by_view ? 1 : V, by_view ? c.nt : 1,
                             B, c.nt, V, st->ny, st->nx, st->dark, p.offset, p.gain, p.epsilon, p.saturation, st->staging, st->dtype, stats);
    HIP_TRY(hipEventRecord(sl.freed, s));
    sl.used = true;
    RL_TRY(rc);
    RL_TRY(st->repair_chunk(st->staging));                          // (before references and estimates)
    std::vector<double> chunk((size_t)B * V * 2, 0.0);              // (fillers: no shift)
    if (r.given) {
        std::copy(r.given + (size_t)c.first * V * 2, r.given + ((size_t)c.first + c.nt) * V * 2, chunk.begin());
    } else {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<int64_t> ro, mo;
        std::vector<double> sh, fl;
        if (c.first == 0) {
            HIP_TRY(hipMemcpyAsync(st->refs, st->staging, V * n_pix * esz, hipMemcpyDeviceToDevice, s));
            if (r.rp->views && V > 1) {
                for (int v = 1; v < V; ++v) {
                    ro.push_back(0);
                    mo.push_back((int64_t)(v * n_pix));
                }
                RL_TRY(stack_estimate(st, r, st->refs, st->refs, ro, mo, sh, fl));
                for (int v = 1; v < V; ++v) {
                    std::copy(&sh[(v - 1) * 2], &sh[(v - 1) * 2] + 2, &r.view_shift[(size_t)v * 2]);
                    std::copy(&fl[(v - 1) * 3], &fl[(v - 1) * 3] + 3, r.ro->view_fields + (size_t)v * 3);
                }
                std::copy(r.view_shift.begin(), r.view_shift.end(), r.ro->view_shifts);
            }
        }
        if (r.rp->frames) {
            ro.clear();
            mo.clear();
            std::vector<int> idx;                                    // f * V + v of each pair; frame 0 is its own reference
            for (int f = 0; f < c.nt; ++f)
                for (int v = 0; v < V; ++v)
                    if (c.first + f > 0) {
                        ro.push_back((int64_t)(v * n_pix));
                        mo.push_back((int64_t)(((size_t)f * V + v) * n_pix));
                        idx.push_back(f * V + v);
                    }
            if (!idx.empty()) {
                RL_TRY(stack_estimate(st, r, st->refs, st->staging, ro, mo, sh, fl));
                for (size_t k = 0; k < idx.size(); ++k) {
                    chunk[(size_t)idx[k] * 2] = sh[k * 2];
                    chunk[(size_t)idx[k] * 2 + 1] = sh[k * 2 + 1];
                    std::copy(&fl[k * 3], &fl[k * 3] + 3, r.ro->fields + ((size_t)c.first * V + idx[k]) * 3);
                }
            }
        }
        for (int f = 0; f < c.nt; ++f)
            for (size_t k = 0; k < (size_t)V * 2; ++k) chunk[(size_t)f * V * 2 + k] = chunk[(size_t)f * V * 2 + k] + r.view_shift[k];
        r.est_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    std::vector<double> sst((size_t)B * V * 2);
    RL_TRY(rl_shift_images(st->ctx, st->staging, st->dtype, B * V, st->ny, st->nx, chunk.data(), r.rp->interp, p.epsilon, st->meas, st->dtype,
                           sst.data()));
    std::copy(chunk.begin(), chunk.begin() + (size_t)c.nt * V * 2, r.ro->shifts + (size_t)c.first * V * 2);
    for (size_t i = 0; i < (size_t)c.nt * V; ++i) r.ro->raised[(size_t)c.first * V + i] = sst[i * 2];
    RL_TRY(rl_deconv_measurement_written(st->plan));
    RL_TRY(rl_deconv_reset_estimate(st->plan));
    RL_TRY(rl_deconv_iterate(st->plan, k_iters));
    float up_ms = 0;
    HIP_TRY(hipEventElapsedTime(&up_ms, sl.up0, sl.uploaded));
    times[1] += up_ms;
    RL_TRY(rl_export(st->ctx, st->est, st->dtype, B, st->ny, st->nx, p.out_scale, sl.dev_out, p.out_dtype, stats + (size_t)B * V * kIngestFields));
    HIP_TRY(hipEventRecord(sl.exported, s));
    return RL_OK;
}
}  // namespace

extern "C" int rl_stack_run(rl_stack* st, const void* raw_host, int n_frames, int k_iters, void* out_host, double* ingest_stats,
                            double* export_stats, double* times_ms) {
    if (!st || !raw_host || !out_host) return fail(RL_ERR_INVALID, "NULL argument");
    if (n_frames < 1 || k_iters < 0) return fail(RL_ERR_INVALID, "n_frames must be at least 1 and k_iters at least 0");
    HIP_TRY(hipSetDevice(st->ctx->device));
    const auto t0 = std::chrono::steady_clock::now();
    const size_t raw_total = (size_t)n_frames * st->V * st->frame_elems() * raw_size(st->prm.raw_dtype);
    const bool raw_direct = host_is_pinned(raw_host, raw_total), out_direct = host_is_pinned(out_host, (size_t)n_frames * st->image_bytes());
    double times[4] = {0, 0, 0, 0};
    const int rc = stack_chunks(st, (const char*)raw_host, raw_direct, n_frames, (char*)out_host, out_direct, ingest_stats, export_stats, times,
                                [&](const Chunk& c) { return stack_compute(st, c, k_iters, times); });
    if (rc != RL_OK) return stack_failed(st, rc);
    times[0] = ms_since(t0);
    if (times_ms) std::copy(times, times + 4, times_ms);
    return RL_OK;
}

extern "C" int rl_stack_run_registered(rl_stack* st, const void* raw_host, int n_frames, int k_iters, const rl_stack_register* rp,
                                       const double* given_shifts, void* out_host, double* ingest_stats, double* export_stats,
                                       rl_stack_register_out* register_out, double* times_ms) {
    if (!st || !raw_host || !rp || !out_host || !register_out) return fail(RL_ERR_INVALID, "NULL argument");
    rl_stack_register_out& ro = *register_out;
    if (!ro.shifts || !ro.fields || !ro.view_shifts || !ro.view_fields || !ro.raised) return fail(RL_ERR_INVALID, "NULL array in register_out");
    if (n_frames < 1 || k_iters < 0) return fail(RL_ERR_INVALID, "n_frames must be at least 1 and k_iters at least 0");
    if (rp->interp != 1 && rp->interp != 3) return fail(RL_ERR_INVALID, "interp must be 1 or 3");
    const int V = st->V;
    if (given_shifts) {
        for (size_t i = 0; i < (size_t)n_frames * V * 2; ++i)
            if (!std::isfinite(given_shifts[i])) return fail(RL_ERR_INVALID, "the given shifts must be finite");
    }
    RegRun r;
    r.rp = rp; r.given = given_shifts; r.ro = &ro; r.M = rp->max_shift + 2;
    r.estimating = !given_shifts && (rp->views || rp->frames);
    r.view_shift.assign((size_t)V * 2, 0.0);
    if (r.estimating) {
        if (rp->max_shift < 1 || rp->max_shift > 32) return fail(RL_ERR_INVALID, "max_shift must lie in 1 .. 32");
        if (rp->refine < 0) return fail(RL_ERR_INVALID, "refine must be at least 0");
        if (st->ny - 2 * r.M < 8 || st->nx - 2 * r.M < 8) return fail(RL_ERR_INVALID, "the window leaves no 8 x 8 interior inside a margin of max_shift + 2");
    }
    HIP_TRY(hipSetDevice(st->ctx->device));
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n_pix = (size_t)st->ny * st->nx, esz = dtype_size(st->dtype);
    if (!st->staging) HIP_TRY(hipMalloc(&st->staging, (size_t)st->B * V * n_pix * esz));
    if (!st->refs) HIP_TRY(hipMalloc(&st->refs, (size_t)V * n_pix * esz));
    if (r.estimating && rp->refine > 0 && !st->scratch) HIP_TRY(hipMalloc((void**)&st->scratch, (size_t)st->B * V * n_pix * sizeof(double)));
    std::fill(ro.shifts, ro.shifts + (size_t)n_frames * V * 2, 0.0);
    std::fill(ro.fields, ro.fields + (size_t)n_frames * V * 3, 0.0);
    std::fill(ro.view_shifts, ro.view_shifts + (size_t)V * 2, 0.0);
    std::fill(ro.view_fields, ro.view_fields + (size_t)V * 3, 0.0);
    std::fill(ro.raised, ro.raised + (size_t)n_frames * V, 0.0);
    const size_t raw_total = (size_t)n_frames * V * st->frame_elems() * raw_size(st->prm.raw_dtype);
    const bool raw_direct = host_is_pinned(raw_host, raw_total), out_direct = host_is_pinned(out_host, (size_t)n_frames * st->image_bytes());
    double times[4] = {0, 0, 0, 0};
    const int rc = stack_chunks(st, (const char*)raw_host, raw_direct, n_frames, (char*)out_host, out_direct, ingest_stats, export_stats, times,
                                [&](const Chunk& c) { return stack_compute_registered(st, c, k_iters, r, times); });
    if (rc != RL_OK) return stack_failed(st, rc);
    times[0] = ms_since(t0);
    if (times_ms) {
        std::copy(times, times + 4, times_ms);
        times_ms[4] = r.est_ms;
    }
    return RL_OK;
}

extern "C" int rl_device_upload_bytes(rl_ctx* ctx, void* dev, const void* host, size_t bytes) {
    if (!ctx || (bytes && (!dev || !host))) return fail(RL_ERR_INVALID, "NULL argument");
    if (!bytes) return RL_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // (the host array may go away)
    return RL_OK;
}
