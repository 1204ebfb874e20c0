// register_api.cpp -- C ABI of the registration primitives (include/rlsted.h: rl_register_sums, rl_shift_images,
// rl_register_peaks, rl_register_estimate, rl_register_xcorr, rl_warp_images, rl_affine_sums): validation, the shift's and the
// prefilter's taps (formed on the host in long double, register_kernels.hpp shift_taps, affine_kernels.hpp warp_prefilter_taps), the
// chunking under the workspace caps and the launches of register_kernels.hip, register_peaks.hip, xcorr_kernels.hip and
// affine_kernels.hip.  Only offsets and taps go up and the sums, peaks and statistics come down.  No kernel is
// launched on bad arguments.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "kernel_variants.hpp"
#include "affine_kernels.hpp"
#include "register_kernels.hpp"
#include "xcorr_kernels.hpp"

using namespace rl;

namespace {
const KernelTable* xcorr_table(int L) {
    switch (L) {
        case 64: return table_64();
        case 192: return table_192();
        case 256: return table_256();
        case 576: return table_576();
        case 1152: return table_1152();
    }
    return nullptr;
}

// the sums of n pairs (offsets: device arrays) in chunks of `chunk` through tot / part, each chunk followed by its peaks into
// peaks [n][5] and, when surf is not null, surf [n][nd]; enqueued on the context's stream.  trips: null, or where the loop's trips go
int enqueue_sums_peaks(rl_ctx* ctx, const RegGeom& g, const void* ref, int ref_dtype, const long long* a_off, const void* mov, int mov_dtype,
                       const long long* b_off, size_t n, size_t chunk, double* tot, double* part, double n_terms, double* peaks, double* surf,
                       int* trips) {
    if (trips) *trips = 0;
    for (size_t first = 0; first < n; first += chunk) {
        if (trips) ++*trips;
        const size_t m = std::min(chunk, n - first);
        RegSumArgs a;
        a.a = ref; a.b = mov; a.a_off = a_off + first; a.b_off = b_off + first; a.part = part; a.tot = tot; a.pairs = (int)m; a.g = g;
        HIP_TRY(register_sums(ref_dtype, mov_dtype, a, ctx->stream));
        RegPeakArgs p;
        p.tot = tot; p.peaks = peaks + first * kPeakFields; p.surf = surf ? surf + first * g.nd : nullptr; p.pairs = (int)m; p.R = g.R; p.n = n_terms;
        HIP_TRY(register_peaks(p, ctx->stream));
    }
    return RL_OK;
}

size_t sum_chunk(const rl_ctx* ctx, const RegGeom& g, size_t n) {
    return chunk_under(ctx->reg_sum_cap, reg_part_doubles(g) * sizeof(double), n);
}
}  // namespace

extern "C" int rl_register_sums(rl_ctx* ctx, const void* ref_dev, int ref_dtype, const int64_t* ref_offsets, const void* mov_dev,
                                int mov_dtype, const int64_t* mov_offsets, int n_pairs, int ny, int nx, int R, int M, double* sums_out,
                                double* ref_out) {
    if (!ctx || !ref_dev || !ref_offsets || !mov_dev || !mov_offsets || !sums_out || !ref_out) return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(ref_dtype) || !dtype_ok(mov_dtype)) return fail(RL_ERR_INVALID, "dtypes must be RL_F32 or RL_F64");
    if (n_pairs < 1) return fail(RL_ERR_INVALID, "n_pairs must be at least 1");
    if (R < 1 || R > kRegMaxR) return fail(RL_ERR_INVALID, "the search radius must lie in 1 .. 32");
    if (M < R) return fail(RL_ERR_INVALID, "the margin must be at least the search radius");
    RL_TRY(check_interior(ny, nx, M));
    RL_TRY(check_pair_offsets(ref_offsets, mov_offsets, n_pairs));
    static_assert(kRegFields == RL_REGISTER_FIELDS && kShiftFields == RL_SHIFT_FIELDS, "the header's field counts");
    HIP_TRY(hipSetDevice(ctx->device));
    const RegGeom g = reg_geom(ny, nx, R, M);
    const size_t per_tot = (size_t)g.nd * kRegFields + 2, per_part = reg_part_doubles(g);
    const size_t chunk = sum_chunk(ctx, g, (size_t)n_pairs);
    WorkLayout lay;
    const auto r_a = lay.add<long long>((size_t)n_pairs), r_b = lay.add<long long>((size_t)n_pairs);
    const auto r_tot = lay.add<double>(chunk * per_tot), r_part = lay.add<double>(chunk * per_part);
    char* w = nullptr;
    RL_TRY(ctx->reg.reserve(ctx->stream, lay.bytes(), &w));
    long long *a_off = r_a.at(w), *b_off = r_b.at(w);
    double *tot = r_tot.at(w), *part = r_part.at(w);
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets are copied as they are");
    HIP_TRY(hipMemcpyAsync(a_off, ref_offsets, (size_t)n_pairs * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(b_off, mov_offsets, (size_t)n_pairs * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    std::vector<double> host(chunk * per_tot);
    int& trips = ctx->chunks_run[RL_CHUNK_REGISTER_SUMS] = 0;
    for (size_t first = 0; first < (size_t)n_pairs; first += chunk) {
        const size_t n = std::min(chunk, (size_t)n_pairs - first);
        ++trips;
        RegSumArgs a;
        a.a = ref_dev; a.b = mov_dev; a.a_off = a_off + first; a.b_off = b_off + first; a.part = part; a.tot = tot; a.pairs = (int)n; a.g = g;
        HIP_TRY(register_sums(ref_dtype, mov_dtype, a, ctx->stream));
        HIP_TRY(hipMemcpyAsync(host.data(), tot, n * per_tot * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < n; ++i) {
            const double* t = host.data() + i * per_tot;
            std::copy(t, t + (size_t)g.nd * kRegFields, sums_out + (first + i) * g.nd * kRegFields);
            ref_out[(first + i) * 2] = t[(size_t)g.nd * kRegFields];
            ref_out[(first + i) * 2 + 1] = t[(size_t)g.nd * kRegFields + 1];
        }
    }
    return RL_OK;
}

extern "C" int rl_shift_images(rl_ctx* ctx, const void* src_dev, int src_dtype, int n, int ny, int nx, const double* shifts, int order,
                               double floor, void* dst_dev, int dst_dtype, double* stats_out) {
    if (!ctx || !src_dev || !shifts || !dst_dev) return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(src_dtype) || !dtype_ok(dst_dtype)) return fail(RL_ERR_INVALID, "dtypes must be RL_F32 or RL_F64");
    if (n < 1 || ny < 1 || nx < 1) return fail(RL_ERR_INVALID, "n, ny and nx must be at least 1");
    if (order != 1 && order != 3) return fail(RL_ERR_INVALID, "order must be 1 or 3");
    if (std::isnan(floor)) return fail(RL_ERR_INVALID, "floor is nan");
    for (size_t i = 0; i < 2 * (size_t)n; ++i)
        if (!(std::fabs(shifts[i]) <= 1e9)) return fail(RL_ERR_INVALID, "image " + std::to_string(i / 2) + ": the shift must be finite, at most 1e9 pixels");
    const size_t n_pix = (size_t)ny * nx;
    if (overlaps(src_dev, (size_t)n * n_pix * dtype_size(src_dtype), dst_dev, (size_t)n * n_pix * dtype_size(dst_dtype)))
        return fail(RL_ERR_INVALID, "the destination overlaps the source");
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<ShiftImage> table((size_t)n);
    for (int i = 0; i < n; ++i) {
        shift_taps(shifts[2 * (size_t)i], order, ny, table[i].gy, &table[i].oy, &table[i].nty);
        shift_taps(shifts[2 * (size_t)i + 1], order, nx, table[i].gx, &table[i].ox, &table[i].ntx);
    }
    const int nb = shift_blocks_y(ny) * shift_blocks_x(nx);
    const size_t chunk = chunk_under(ctx->shift_cap, n_pix * sizeof(double), (size_t)n);
    WorkLayout lay;
    const auto r_table = lay.add<ShiftImage>((size_t)n);
    const auto r_stats = lay.add<double>((size_t)n * kShiftFields), r_part = lay.add<double>(chunk * nb * kShiftFields);
    const auto r_tmp = lay.add<double>(chunk * n_pix);
    char* w = nullptr;
    RL_TRY(ctx->reg.reserve(ctx->stream, lay.bytes(), &w));
    ShiftImage* table_dev = r_table.at(w);
    double *stats = r_stats.at(w), *part = r_part.at(w), *tmp = r_tmp.at(w);
    HIP_TRY(hipMemcpyAsync(table_dev, table.data(), (size_t)n * sizeof(ShiftImage), hipMemcpyHostToDevice, ctx->stream));
    int& trips = ctx->chunks_run[RL_CHUNK_SHIFT] = 0;
    for (size_t first = 0; first < (size_t)n; first += chunk) {
        ++trips;
        ShiftArgs a;
        a.src = (const char*)src_dev + first * n_pix * dtype_size(src_dtype);
        a.dst = (char*)dst_dev + first * n_pix * dtype_size(dst_dtype);
        a.img = table_dev + first;
        a.part = stats_out ? part : nullptr;
        a.n = (int)std::min(chunk, (size_t)n - first);
        a.ny = ny; a.nx = nx; a.floor = floor;
        HIP_TRY(shift_images(src_dtype, dst_dtype, a, tmp, stats_out ? stats + first * kShiftFields : nullptr, ctx->stream));
    }
    if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, stats, (size_t)n * kShiftFields * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // (the taps' table is the call's own)
    return RL_OK;
}

extern "C" int rl_register_peaks(rl_ctx* ctx, const double* tot_dev, int n_pairs, int R, double n_terms, double* peaks_out, double* surface_out) {
    if (!ctx || !tot_dev || !peaks_out) return fail(RL_ERR_INVALID, "NULL argument");
    if (n_pairs < 1) return fail(RL_ERR_INVALID, "n_pairs must be at least 1");
    if (R < 1 || R > kRegMaxR) return fail(RL_ERR_INVALID, "the search radius must lie in 1 .. 32");
    if (!std::isfinite(n_terms) || !(n_terms >= 1.0)) return fail(RL_ERR_INVALID, "n_terms must be finite and at least 1");
    static_assert(kPeakFields == RL_PEAK_FIELDS, "the header's field count");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t nd = (size_t)(2 * R + 1) * (2 * R + 1);
    WorkLayout lay;
    const auto r_peaks = lay.add<double>((size_t)n_pairs * kPeakFields);
    const auto r_surf = lay.add<double>(surface_out ? (size_t)n_pairs * nd : 0);
    char* w = nullptr;
    RL_TRY(ctx->reg.reserve(ctx->stream, lay.bytes(), &w));
    RegPeakArgs a;
    a.tot = tot_dev; a.peaks = r_peaks.at(w); a.surf = r_surf.at(w); a.pairs = n_pairs; a.R = R; a.n = n_terms;
    HIP_TRY(register_peaks(a, ctx->stream));
    HIP_TRY(hipMemcpyAsync(peaks_out, a.peaks, r_peaks.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    if (surface_out) HIP_TRY(hipMemcpyAsync(surface_out, a.surf, r_surf.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RL_OK;
}

extern "C" int rl_register_estimate(rl_ctx* ctx, const void* ref_dev, int ref_dtype, const int64_t* ref_offsets, const void* mov_dev,
                                    int mov_dtype, const int64_t* mov_offsets, int n_pairs, int ny, int nx, int R, int M, int refine,
                                    double* scratch_dev, double* shifts_out, double* fields_out, double* surface_out) {
    if (!ctx || !ref_dev || !ref_offsets || !mov_dev || !mov_offsets || !shifts_out || !fields_out) return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(ref_dtype) || !dtype_ok(mov_dtype)) return fail(RL_ERR_INVALID, "dtypes must be RL_F32 or RL_F64");
    if (n_pairs < 1) return fail(RL_ERR_INVALID, "n_pairs must be at least 1");
    if (R < 1 || R > kRegMaxR) return fail(RL_ERR_INVALID, "the search radius must lie in 1 .. 32");
    if (M < R) return fail(RL_ERR_INVALID, "the margin must be at least the search radius");
    RL_TRY(check_interior(ny, nx, M));
    if (refine < 0) return fail(RL_ERR_INVALID, "refine must be at least 0");
    if (refine > 0 && !scratch_dev) return fail(RL_ERR_INVALID, "refine > 0 needs a scratch buffer");
    RL_TRY(check_pair_offsets(ref_offsets, mov_offsets, n_pairs));
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_pairs, n_pix = (size_t)ny * nx;
    const RegGeom g = reg_geom(ny, nx, R, M), g1 = reg_geom(ny, nx, 1, M);
    const size_t chunk = sum_chunk(ctx, g, n), chunk1 = sum_chunk(ctx, g1, n);
    const size_t per_tot = (size_t)g.nd * kRegFields + 2, per_tot1 = (size_t)g1.nd * kRegFields + 2;
    const size_t schunk = chunk_under(ctx->shift_cap, n_pix * sizeof(double), n);
    WorkLayout lay;
    const auto r_a = lay.add<long long>(n), r_b = lay.add<long long>(n), r_la = lay.add<long long>(n), r_lb = lay.add<long long>(n);
    const auto r_peaks = lay.add<double>(n * kPeakFields), r_surf = lay.add<double>(surface_out ? n * g.nd : 0);
    const auto r_tot = lay.add<double>(std::max(chunk * per_tot, chunk1 * per_tot1));   // (both stages' sums go through tot and part)
    const auto r_part = lay.add<double>(std::max(chunk * reg_part_doubles(g), chunk1 * reg_part_doubles(g1)));
    const auto r_table = lay.add<ShiftImage>(refine ? n : 0);
    const auto r_tmp = lay.add<double>(refine ? schunk * n_pix : 0);
    char* w = nullptr;
    RL_TRY(ctx->reg.reserve(ctx->stream, lay.bytes(), &w));
    long long *a_off = r_a.at(w), *b_off = r_b.at(w), *la_off = r_la.at(w), *lb_off = r_lb.at(w);
    double *peaks = r_peaks.at(w), *surf = r_surf.at(w), *tot = r_tot.at(w), *part = r_part.at(w), *tmp = r_tmp.at(w);
    ShiftImage* table_dev = r_table.at(w);
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets are copied as they are");
    HIP_TRY(hipMemcpyAsync(a_off, ref_offsets, n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(b_off, mov_offsets, n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    const double n_terms = (double)(((long long)ny - 2LL * M) * ((long long)nx - 2LL * M));
    // stages 1 - 3: sums, peaks, 5 doubles per pair down
    std::vector<double> pk(n * kPeakFields);
    RL_TRY(enqueue_sums_peaks(ctx, g, ref_dev, ref_dtype, a_off, mov_dev, mov_dtype, b_off, n, chunk, tot, part, n_terms, peaks, surf,
                              &ctx->chunks_run[RL_CHUNK_REGISTER_SUMS]));
    HIP_TRY(hipMemcpyAsync(pk.data(), peaks, n * kPeakFields * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (surface_out) HIP_TRY(hipMemcpyAsync(surface_out, surf, n * g.nd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i) reg_estimate_first(&pk[i * kPeakFields], shifts_out + 2 * i, fields_out + 3 * i);
    // stage 4: per pass, the pairs that are not flat shifted by their estimate into the scratch, a 3 x 3 window, the offset added
    std::vector<size_t> live;
    for (size_t i = 0; i < n; ++i)
        if (fields_out[3 * i + 2] == 0.0) live.push_back(i);
    std::vector<ShiftImage> table(refine ? live.size() : 0);
    std::vector<long long> la(live.size()), lb(live.size());
    for (size_t k = 0; k < live.size(); ++k) {
        la[k] = ref_offsets[live[k]];
        lb[k] = (long long)(k * n_pix);
    }
    if (refine && !live.empty()) {
        HIP_TRY(hipMemcpyAsync(la_off, la.data(), live.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(lb_off, lb.data(), live.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    }
    const size_t mov_size = dtype_size(mov_dtype);
    for (int pass = 0; pass < refine && !live.empty(); ++pass) {
        const size_t L = live.size();
        for (size_t k = 0; k < L; ++k) {
            const double* s = shifts_out + 2 * live[k];
            shift_taps(s[0], 3, ny, table[k].gy, &table[k].oy, &table[k].nty);
            shift_taps(s[1], 3, nx, table[k].gx, &table[k].ox, &table[k].ntx);
        }
        HIP_TRY(hipMemcpyAsync(table_dev, table.data(), L * sizeof(ShiftImage), hipMemcpyHostToDevice, ctx->stream));
        int& trips = ctx->chunks_run[RL_CHUNK_SHIFT] = 0;
        for (size_t k = 0; k < L;) {            // runs of consecutive moving images, at most schunk at a time
            ++trips;
            size_t m = 1;
            while (k + m < L && m < schunk && mov_offsets[live[k + m]] == mov_offsets[live[k]] + (int64_t)(m * n_pix)) ++m;
            ShiftArgs a;
            a.src = (const char*)mov_dev + (size_t)mov_offsets[live[k]] * mov_size;
            a.dst = scratch_dev + k * n_pix;
            a.img = table_dev + k;
            a.part = nullptr;
            a.n = (int)m;
            a.ny = ny; a.nx = nx; a.floor = -HUGE_VAL;
            HIP_TRY(shift_images(mov_dtype, RL_F64, a, tmp, nullptr, ctx->stream));
            k += m;
        }
        RL_TRY(enqueue_sums_peaks(ctx, g1, ref_dev, ref_dtype, la_off, scratch_dev, RL_F64, lb_off, L, chunk1, tot, part, n_terms, peaks, nullptr, nullptr));
        HIP_TRY(hipMemcpyAsync(pk.data(), peaks, L * kPeakFields * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t k = 0; k < L; ++k) reg_estimate_refine(&pk[k * kPeakFields], shifts_out + 2 * live[k], fields_out + 3 * live[k]);
    }
    return RL_OK;
}

extern "C" int rl_register_xcorr(rl_ctx* ctx, const void* ref_dev, int ref_dtype, const int64_t* ref_offsets, const void* mov_dev,
                                 int mov_dtype, const int64_t* mov_offsets, int n_pairs, int ny, int nx, int R, double* peaks_out,
                                 float* surface_out) {
    if (!ctx || !ref_dev || !ref_offsets || !mov_dev || !mov_offsets || !peaks_out) return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(ref_dtype) || !dtype_ok(mov_dtype)) return fail(RL_ERR_INVALID, "dtypes must be RL_F32 or RL_F64");
    if (n_pairs < 1) return fail(RL_ERR_INVALID, "n_pairs must be at least 1");
    if (ny < 1 || nx < 1) return fail(RL_ERR_INVALID, "ny and nx must be at least 1");
    if (R < 1 || R > std::min(ny, nx) / 2) return fail(RL_ERR_INVALID, "the search radius must lie in 1 .. min(ny, nx) / 2");
    const int Ly = select_xcorr((long long)ny + R), Lx = select_xcorr((long long)nx + R);
    if (!Ly || !Lx)
        return fail(RL_ERR_INVALID, "ny + R and nx + R must not exceed the largest transform length of the coarse stage (" + std::to_string(kXcMaxL) + ")");
    RL_TRY(check_pair_offsets(ref_offsets, mov_offsets, n_pairs));
    static_assert(kXcFields == RL_XCORR_FIELDS, "the header's field count");
    HIP_TRY(hipSetDevice(ctx->device));
    void *tw_y = nullptr, *tw_x = nullptr;
    RL_TRY(ctx->twiddles(xcorr_table(Ly), RL_F32, &tw_y));
    RL_TRY(ctx->twiddles(xcorr_table(Lx), RL_F32, &tw_x));
    const size_t W = 2 * (size_t)R + 1;
    // what one pair takes of the workspace: its spectrum, kept rows, correlation window and, when asked for, surface
    const size_t spec_n = (size_t)ny * Lx, rows_n = W * Lx, corr_n = W * W, surf_n = surface_out ? corr_n : 0;
    WorkLayout one;
    one.add<cx<float>>(spec_n);
    one.add<cx<float>>(rows_n);
    one.add<float>(corr_n);
    one.add<float>(surf_n);
    const size_t chunk = chunk_under(ctx->xcorr_cap, one.bytes(), (size_t)n_pairs);
    WorkLayout lay;
    const auto r_a = lay.add<long long>((size_t)n_pairs), r_b = lay.add<long long>((size_t)n_pairs);
    const auto r_stats = lay.add<double>(chunk * 4), r_peaks = lay.add<double>(chunk * kXcFields);
    const auto r_spec = lay.add<cx<float>>(spec_n, chunk), r_rows = lay.add<cx<float>>(rows_n, chunk);   // (a padded slot per pair)
    const auto r_corr = lay.add<float>(corr_n, chunk), r_surf = lay.add<float>(surf_n, chunk);
    char* w = nullptr;
    RL_TRY(ctx->reg.reserve(ctx->stream, lay.bytes(), &w));
    long long *a_off = r_a.at(w), *b_off = r_b.at(w);
    XcArgs a;
    a.a = ref_dev; a.b = mov_dev; a.a_f64 = ref_dtype == RL_F64; a.b_f64 = mov_dtype == RL_F64;
    a.ny = ny; a.nx = nx; a.R = R; a.Ly = Ly; a.Lx = Lx;
    a.stats = r_stats.at(w); a.peaks = r_peaks.at(w);
    a.spec = r_spec.at(w); a.rows = r_rows.at(w); a.corr = r_corr.at(w); a.surf = r_surf.at(w);
    a.tw_y = (const cx<float>*)tw_y; a.tw_x = (const cx<float>*)tw_x;
    HIP_TRY(hipMemcpyAsync(a_off, ref_offsets, (size_t)n_pairs * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(b_off, mov_offsets, (size_t)n_pairs * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    int& trips = ctx->chunks_run[RL_CHUNK_XCORR] = 0;
    for (size_t first = 0; first < (size_t)n_pairs; first += chunk) {
        const size_t n = std::min(chunk, (size_t)n_pairs - first);
        ++trips;
        a.a_off = a_off + first; a.b_off = b_off + first; a.pairs = (int)n;
        HIP_TRY(xcorr_pairs(a, ctx->stream));
        HIP_TRY(hipMemcpyAsync(peaks_out + first * kXcFields, a.peaks, n * kXcFields * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (surface_out)
            HIP_TRY(hipMemcpyAsync(surface_out + first * W * W, a.surf, n * W * W * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return RL_OK;
}

extern "C" int rl_warp_chunk_bytes(rl_ctx* ctx, size_t bytes) {
    if (!ctx || bytes < 1) return fail(RL_ERR_INVALID, "NULL context or a cap of 0 bytes");
    ctx->warp_cap = bytes;
    return RL_OK;
}

extern "C" int rl_warp_path(rl_ctx* ctx, int path) {
    if (!ctx || (path != 0 && path != 1)) return fail(RL_ERR_INVALID, "NULL context or a path that is neither 0 nor 1");
    ctx->warp_direct = path;
    return RL_OK;
}

extern "C" int rl_warp_images(rl_ctx* ctx, const void* src_dev, int src_dtype, int n, int sy, int sx, const double* xf, int order,
                              double floor, void* dst_dev, int dst_dtype, int oy, int ox, double* stats_out) {
    if (!ctx || !src_dev || !xf || !dst_dev) return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(src_dtype) || !dtype_ok(dst_dtype)) return fail(RL_ERR_INVALID, "dtypes must be RL_F32 or RL_F64");
    if (n < 1 || sy < 1 || sx < 1 || oy < 1 || ox < 1) return fail(RL_ERR_INVALID, "n, sy, sx, oy and ox must be at least 1");
    if (order != 1 && order != 3) return fail(RL_ERR_INVALID, "order must be 1 or 3");
    if (std::isnan(floor)) return fail(RL_ERR_INVALID, "floor is nan");
    for (size_t i = 0; i < (size_t)n; ++i) {
        const double* m = xf + i * kWarpXf;
        for (int k = 0; k < kWarpXf; ++k)
            if (!std::isfinite(m[k])) return fail(RL_ERR_INVALID, "image " + std::to_string(i) + ": the transform must be finite");
        for (int c = 0; c < 4; ++c) {
            double Y, X;
            warp_coord(m, c & 2 ? oy - 1 : 0, c & 1 ? ox - 1 : 0, Y, X);
            if (!(std::fabs(Y) <= kWarpMaxCoord) || !(std::fabs(X) <= kWarpMaxCoord))
                return fail(RL_ERR_INVALID, "image " + std::to_string(i) + ": the output grid must map to coordinates of at most 1e9 pixels");
        }
    }
    const size_t s_pix = (size_t)sy * sx, o_pix = (size_t)oy * ox;
    if (overlaps(src_dev, (size_t)n * s_pix * dtype_size(src_dtype), dst_dev, (size_t)n * o_pix * dtype_size(dst_dtype)))
        return fail(RL_ERR_INVALID, "the destination overlaps the source");
    static_assert(kWarpFields == RL_SHIFT_FIELDS, "the header's field count");
    HIP_TRY(hipSetDevice(ctx->device));
    const int nb = warp_blocks_y(oy) * warp_blocks_x(ox);
    const size_t per = (order == 3 ? 2 * s_pix * sizeof(double) + sizeof(ShiftImage) : 0) + (size_t)nb * kWarpFields * sizeof(double);
    const size_t chunk = chunk_under(ctx->warp_cap, per, (size_t)n);
    WorkLayout lay;
    const auto r_xf = lay.add<double>((size_t)n * kWarpXf), r_stats = lay.add<double>((size_t)n * kWarpFields);
    const auto r_part = lay.add<double>(chunk * nb * kWarpFields);
    const auto r_table = lay.add<ShiftImage>(order == 3 ? chunk : 0);   // (the prefilter's regions: order 3 alone)
    const auto r_tmp = lay.add<double>(order == 3 ? chunk * s_pix : 0), r_coef = lay.add<double>(order == 3 ? chunk * s_pix : 0);
    char* w = nullptr;
    RL_TRY(ctx->reg.reserve(ctx->stream, lay.bytes(), &w));
    double *xf_dev = r_xf.at(w), *stats = r_stats.at(w), *part = r_part.at(w), *tmp = r_tmp.at(w), *coef = r_coef.at(w);
    ShiftImage* table_dev = r_table.at(w);
    HIP_TRY(hipMemcpyAsync(xf_dev, xf, (size_t)n * kWarpXf * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    std::vector<ShiftImage> table;
    if (order == 3) {           // the same taps for every image of a chunk
        table.resize(chunk);
        warp_prefilter_taps(sy, table[0].gy, &table[0].oy, &table[0].nty);
        warp_prefilter_taps(sx, table[0].gx, &table[0].ox, &table[0].ntx);
        for (size_t k = 1; k < chunk; ++k) table[k] = table[0];
        HIP_TRY(hipMemcpyAsync(table_dev, table.data(), chunk * sizeof(ShiftImage), hipMemcpyHostToDevice, ctx->stream));
    }
    int& trips = ctx->chunks_run[RL_CHUNK_WARP] = 0;
    for (size_t first = 0; first < (size_t)n; first += chunk) {
        const size_t m = std::min(chunk, (size_t)n - first);
        ++trips;
        const char* src = (const char*)src_dev + first * s_pix * dtype_size(src_dtype);
        if (order == 3) {       // the prefilter alone: along x into tmp, along y into coef
            ShiftArgs f;
            f.src = src; f.dst = coef; f.img = table_dev; f.part = nullptr; f.n = (int)m; f.ny = sy; f.nx = sx; f.floor = -HUGE_VAL;
            HIP_TRY(shift_images(src_dtype, RL_F64, f, tmp, nullptr, ctx->stream));
        }
        WarpArgs a;
        a.src = order == 3 ? (const void*)coef : (const void*)src;
        a.dst = (char*)dst_dev + first * o_pix * dtype_size(dst_dtype);
        a.xf = xf_dev + first * kWarpXf;
        a.part = stats_out ? part : nullptr;
        a.n = (int)m; a.sy = sy; a.sx = sx; a.oy = oy; a.ox = ox; a.order = order; a.direct = ctx->warp_direct; a.floor = floor;
        HIP_TRY(warp_images(order == 3 ? RL_F64 : src_dtype, dst_dtype, a, stats_out ? stats + first * kWarpFields : nullptr, ctx->stream));
    }
    if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, stats, (size_t)n * kWarpFields * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // (the tables are the call's own)
    return RL_OK;
}

extern "C" int rl_affine_sums(rl_ctx* ctx, const void* ref_dev, int ref_dtype, const int64_t* ref_offsets, const void* w_dev, int w_dtype,
                              const int64_t* w_offsets, int n_pairs, int ny, int nx, int M, double* sums_out) {
    if (!ctx || !ref_dev || !ref_offsets || !w_dev || !w_offsets || !sums_out) return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(ref_dtype) || !dtype_ok(w_dtype)) return fail(RL_ERR_INVALID, "dtypes must be RL_F32 or RL_F64");
    if (n_pairs < 1) return fail(RL_ERR_INVALID, "n_pairs must be at least 1");
    if (M < 1) return fail(RL_ERR_INVALID, "the margin must be at least 1");
    RL_TRY(check_interior(ny, nx, M));
    if ((long long)ny * nx > 0x7fffffffLL) return fail(RL_ERR_INVALID, "an image must have fewer than 2^31 pixels");
    RL_TRY(check_pair_offsets(ref_offsets, w_offsets, n_pairs));
    static_assert(kAffFields == RL_AFFINE_FIELDS, "the header's field count");
    HIP_TRY(hipSetDevice(ctx->device));
    const AffGeom g = aff_geom(ny, nx, M);
    const size_t per_part = (size_t)g.nb * kAffFields;
    const size_t chunk = chunk_under(ctx->reg_sum_cap, per_part * sizeof(double), (size_t)n_pairs);
    WorkLayout lay;
    const auto r_a = lay.add<long long>((size_t)n_pairs), r_b = lay.add<long long>((size_t)n_pairs);
    const auto r_tot = lay.add<double>(chunk * kAffFields), r_part = lay.add<double>(chunk * per_part);
    char* w = nullptr;
    RL_TRY(ctx->reg.reserve(ctx->stream, lay.bytes(), &w));
    long long *a_off = r_a.at(w), *b_off = r_b.at(w);
    double *tot = r_tot.at(w), *part = r_part.at(w);
    HIP_TRY(hipMemcpyAsync(a_off, ref_offsets, (size_t)n_pairs * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(b_off, w_offsets, (size_t)n_pairs * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    int& trips = ctx->chunks_run[RL_CHUNK_REGISTER_SUMS] = 0;
    for (size_t first = 0; first < (size_t)n_pairs; first += chunk) {
        const size_t n = std::min(chunk, (size_t)n_pairs - first);
        ++trips;
        AffArgs a;
        a.a = ref_dev; a.w = w_dev; a.a_off = a_off + first; a.w_off = b_off + first; a.part = part; a.tot = tot; a.pairs = (int)n; a.g = g;
        HIP_TRY(affine_sums(ref_dtype, w_dtype, a, ctx->stream));
        HIP_TRY(hipMemcpyAsync(sums_out + first * kAffFields, tot, n * kAffFields * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return RL_OK;
}
