// rlsted.cpp -- C ABI (include/rlsted.h) over the gfx950 kernels.
// Host orchestration only: buffer ownership, kernel sequencing on one HIP
// stream per context, host<->device staging.  No arithmetic of the hot path
// runs on the host.
#include "../../include/rlsted.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "accel_kernels.hpp"
#include "aux_kernels.hpp"
#include "checkpoint_kernels.hpp"
#include "conv_kernels.hpp"
#include "cycle_schedule.hpp"
#include "kernel_table.hpp"
#include "object_classes.hpp"
#include "plan_options.hpp"
#include "ctx.hpp"
#include "sep_kernels.hpp"
#include "sep_taps.hpp"
#include "stop_kernels.hpp"
#include "tv_kernels.hpp"

using namespace rl;

namespace rl {
std::string& last_error() {
    thread_local std::string e;
    return e;
}
int fail(int code, const std::string& msg) {
    last_error() = msg;
    return code;
}
LaunchTiming& launch_timing() {
    thread_local LaunchTiming t;
    return t;
}
bool debug_sync() {
    static const bool v = getenv("RLSTED_DEBUG_SYNC") != nullptr;
    return v;
}
}  // namespace rl

namespace {

const KernelTable* table_for(int L) {
    switch (L) {
        case 64: return table_64();
        case 192: return table_192();
        case 256: return table_256();
        case 576: return table_576();
        case 1152: return table_1152();
        case 2304: return table_2304();
        case 4608: return table_4608();
    }
    return nullptr;
}
const int kLengths[] = {64, 192, 256, 576, 1152, 2304, 4608};

// Device temporaries of the plan set-up: freed when the scope ends, whichever way it ends (hipFree waits for the device).
struct TempBuffers {
    std::vector<void*> bufs;
    int get(void** p, size_t bytes) {
        HIP_TRY(hipMalloc(p, bytes));
        bufs.push_back(*p);
        return RL_OK;
    }
    ~TempBuffers() {
        for (void* b : bufs) (void)hipFree(b);
    }
};

}  // namespace

struct rl_deconv {
    rl_ctx* ctx = nullptr;
    PlanOptions opt;
    int V = 0, py = 0, px = 0, B = 0, ny = 0, nx = 0, dtype = RL_F32;
    int ly = 0, lx = 0, kx = 0, pitch = 0;
    const KernelTable *ty = nullptr, *tx = nullptr;
    void *twy = nullptr, *twx = nullptr;
    // device buffers (element type = dtype)
    void* psf_hat = nullptr;   // [V][ly][pitch] complex
    void* psf_hat_re = nullptr;   // real parts, when the PSF spectrum is real (point-symmetric PSFs) and the column
                                  // transform is wave private: the column kernels then multiply by a real array
    double psf_hat_imag_ratio = 0;   // max |im| / max |z| of the PSF spectrum
    void* spec_a = nullptr;    // [B] spectrum images (layout: conv_kernels.hpp spec_off)
    void* spec_b = nullptr;    // [B*V] spectrum images
    void* spec_x = nullptr;    // [B*V] column spectra in register-slot order between the halves of the split column pass (col_split() plans)
    void* spec_ones = nullptr; // [V] column-transformed spectra of H(estimate = 1): the same for every frame (ref:522)
    // storage-precision study builds (conv_kernels.hpp RL_SPEC_QUANT): powers of two that bring the DC term of an
    // estimate-type / ratio-type spectrum to 2^14 (RLSTED_Q_EXP_EST / RLSTED_Q_EXP_RATIO = log2 of the DC bound)
    float q_est = 1.0f, q_ratio = 1.0f;
    // f32 plans (conv_kernels.hpp rl_ratio): the normaliser H_t(ones) from the PSFs' integral images instead of the f32 transform
    // path (deconv_build), and -- non-negative PSFs -- the second half of every iteration on `ratio - 1`
    // (RLSTED_SUB_ONE=0: off).  Both shrink f32 rounding error, neither changes the arithmetic in exact terms.
    bool sub_one = false;
    // `ratio - 1` clamps the SUM of the views' back-projections where the reference clamps each view's (ref:587).  The two agree
    // whenever no view's term is negative -- always for one view, and for several as long as the measurement has no negative
    // pixel (PSFs >= 0 is a condition of sub_one).  A multi-view measurement WITH negative pixels (background-subtracted data
    // through rl_deconv_set_measurement) therefore runs the plain arithmetic with the per-view clamp; so does RLSTED_FUSE_VIEWS=0,
    // the switch that asks for the reference's per-view clamp.
    bool meas_negative = false;
    // lanes of the ROW_RATIO launches that met a prediction H(est) <= 0 inside the image (conv_kernels.hpp rl_ratio: such a pixel is
    // neutral); device counter, read by rl_deconv_unresolved.  Zero on data whose predictions the plan's arithmetic resolves.
    unsigned long long* unresolved = nullptr;
    bool sub() const { return sub_one && !(V > 1 && meas_negative); }
    void* obj = nullptr;       // [B][ny][nx]
    void* noiseless = nullptr; // [B*V][ny][nx]
    void* meas = nullptr;      // [B*V][ny][nx]
    void* est = nullptr;       // [B][ny][nx]
    void* norm = nullptr;      // [ny][nx]
    void* scratch = nullptr;   // [B*V][ny][nx] staging for rl_forward / rl_adjoint
    size_t bytes = 0;
    bool have_obj = false, have_meas = false;
    // ---- device memory: every buffer of the plan comes from alloc() and goes in rl_deconv_destroy -- or in release(), for one that is
    // replaced during the plan's life.  `bytes` (rl_deconv_info's device_bytes) adds up what alloc() handed out, less the small buffers
    // that never were part of that figure (UNCOUNTED).  SLACK: RL_STREAM_SLACK zeroed bytes behind the buffer -- the streaming row
    // kernels load whole 64-lane segments without clamping; lanes past the end of the last row of a buffer read (and discard) these bytes.
    enum { UNCOUNTED = 1, SLACK = 2 };
    struct Owned { void* p; size_t counted; };
    std::vector<Owned> owned;
    template <typename P>
    int alloc(P** p, size_t n, int flags = 0) {
        const size_t total = n + ((flags & SLACK) ? RL_STREAM_SLACK : 0);
        HIP_TRY(hipMalloc((void**)p, total));
        owned.push_back({(void*)*p, (flags & UNCOUNTED) ? 0 : total});
        bytes += owned.back().counted;
        if (flags & SLACK) HIP_TRY(hipMemsetAsync((char*)*p + n, 0, RL_STREAM_SLACK, ctx->stream));
        return RL_OK;
    }
    template <typename P>
    int release(P** p) {
        for (Owned& o : owned)
            if (*p && o.p == (void*)*p) {
                HIP_TRY(hipFree(o.p));
                bytes -= o.counted;
                o = owned.back();
                owned.pop_back();
                break;
            }
        *p = nullptr;
        return RL_OK;
    }
    // host float64 values -> a device array of the plan's dtype (the stencils' taps)
    int upload_taps(void** p, const std::vector<double>& v) {
        RL_TRY(alloc(p, v.size() * dtype_size(dtype), UNCOUNTED));
        return rl::upload_as(dtype, v, *p);
    }
    // H_t views summed before the inverse transforms (one clamp of the sum instead of one per
    // view, ref:587): default for f32 plans, off for f64 (faithful); RLSTED_FUSE_VIEWS=0/1 overrides
    bool fuse_views = false;
    // ---- streams and events: every one the plan creates comes from here and goes in rl_deconv_destroy
    struct Handles {
        std::vector<hipStream_t> streams;
        std::vector<hipEvent_t> events;
        int stream(hipStream_t* s) {
            HIP_TRY(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
            streams.push_back(*s);
            return RL_OK;
        }
        int event(hipEvent_t* e, unsigned flags = hipEventDisableTiming) {
            HIP_TRY(hipEventCreateWithFlags(e, flags));
            events.push_back(*e);
            return RL_OK;
        }
    };
    Handles handles;
    // A lane of run_slices (cycle_schedule.hpp): its stream and the events recorded on it or for it -- done: its end, for the join;
    // drawn: behind its last in-lane draw from the class rates, for the next cycle's class simulation; begun: in front of a slice's
    // first iteration launch, and drawn_ahead: behind the draw, on the context's stream, of the slice the lane takes next (draws ahead).
    struct Lane {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr, drawn = nullptr, begun = nullptr, drawn_ahead = nullptr;
    };
    Lane lane[kMaxLanes];
    hipEvent_t fork = nullptr, rates_ready = nullptr;   // the lanes leave the context's stream; the class rates are written
    CycleSchedule schedule;                           // of the run at hand (kept: the list is rebuilt in place)
    CycleState cycle_state;                           // what the last run left behind: lanes still open, events the next cycle waits for
    hipStream_t active = nullptr;                     // stream the kernel launch helpers use
    void* slice_ws = nullptr;                         // per-slice Poisson work lists of run_slices()
    void *key_seeds = nullptr, *key_ids = nullptr;    // per-frame Philox keys of rl_deconv_simulate_keyed
    size_t slice_ws_bytes = 0, slice_ws_stride = 0;
    // ---- rl_batch_submit: the tasks of a chunk -- objects, brightness targets, Philox keys -- are staged in one page-locked
    // block, uploaded on a copy stream of the plan's own and consumed on the context's stream; two blocks, so that chunk i + 1
    // is staged and uploaded while chunk i iterates.  Block layout (host and device): header -- [B] float64 targets, [B] uint64
    // seeds, [B] uint32 image ids, [B] uint32 object index, [2][B] uint32 lists of the shared simulation (ShareLists) -- then the chunk's DISTINCT objects, [<= B][n_img] float64 (tasks that
    // share an object pointer -- a sweep's seeds -- are staged and uploaded once; only the used prefix of the block crosses PCIe);
    // the device block is followed by the objects' float64 sums and their scratch (aux_sums_elems(B)).
    struct BatchSlot {
        char* host = nullptr;
        char* dev = nullptr;
        hipEvent_t uploaded = nullptr, freed = nullptr;
        bool used = false;
    };
    BatchSlot bslot[2];
    void* batch_out = nullptr;       // rl_batch_run's result buffer (grow only)
    size_t batch_out_bytes = 0;
    hipStream_t copy_stream = nullptr;
    unsigned long batch_chunks = 0;
    size_t slot_objects_bytes() const { return (size_t)B * n_img() * sizeof(double); }
    size_t slot_header_bytes() const { return ((size_t)B * (8 + 8 + 4 + 4 + 4 + 4) + 15) / 16 * 16; }
    size_t slot_host_bytes() const { return slot_header_bytes() + slot_objects_bytes(); }
    bool batch_slots_ready = false;
    int ensure_batch_slots() {
        if (batch_slots_ready) return RL_OK;
        // (a call that failed half way is taken up where it stopped: every resource is created once, the destructor frees what exists)
        if (!copy_stream) RL_TRY(handles.stream(&copy_stream));
        for (BatchSlot& sl : bslot) {
            if (!sl.host) HIP_TRY(hipHostMalloc((void**)&sl.host, slot_host_bytes(), hipHostMallocDefault));
            if (!sl.dev) RL_TRY(alloc(&sl.dev, slot_host_bytes() + 8 + aux_sums_elems((size_t)B) * sizeof(double)));
            if (!sl.uploaded) RL_TRY(handles.event(&sl.uploaded));
            if (!sl.freed) RL_TRY(handles.event(&sl.freed));
        }
        batch_slots_ready = true;
        return RL_OK;
    }
    hipStream_t cur() const { return active ? active : ctx->stream; }
    bool est_ready = false;    // est holds a valid estimate
    // ---- Biggs-Andrews acceleration (accel_kernels.hpp, rl_deconv_set_acceleration): per frame the previous point x_{k-1}, the
    // extrapolated point y_k and the step g_k in three image buffers, the dot products' per-workgroup partials and the a of the
    // last extrapolated point in float64 -- allocated when the mode is first switched on.  The history spans rl_deconv_iterate
    // calls; acc_steps = the psi steps taken in it (0: none -- new data, a set estimate, a change of mode).
    int accel = RL_ACCEL_NONE;
    void *acc_x = nullptr, *acc_y = nullptr, *acc_g = nullptr;
    double *acc_part = nullptr, *acc_alpha = nullptr;
    long acc_steps = 0;
    int acc_blocks() const { return accel_blocks(n_img(), dtype_size(dtype)); }
    int ensure_accel() {
        const size_t img = (size_t)B * n_img() * dtype_size(dtype), part = (size_t)B * acc_blocks() * 2 * sizeof(double);
        for (void** p : {&acc_x, &acc_y, &acc_g})
            if (!*p) RL_TRY(alloc(p, img));
        if (!acc_part) RL_TRY(alloc(&acc_part, part));
        if (!acc_alpha) {
            RL_TRY(alloc(&acc_alpha, (size_t)B * sizeof(double)));
            HIP_TRY(hipMemsetAsync(acc_alpha, 0, (size_t)B * sizeof(double), ctx->stream));
        }
        return RL_OK;
    }
    int accel_reset() {   // (on the context's stream, before any slice of the next run forks off it)
        acc_steps = 0;
        if (acc_alpha) HIP_TRY(hipMemsetAsync(acc_alpha, 0, (size_t)B * sizeof(double), ctx->stream));
        return RL_OK;
    }
    // psi step s of the history on frames [f0, f0 + nf): extrapolate (not from the start x_0 = ones, whose y_0 is x_0 -- the shortcut
    // iteration still applies), rebuild the spectrum of est = y_s where the loop reads one, iterate, then g_s and its partials.
    // ROW_UPDATE's spectrum is of x_{s+1}, not of the next y: the pair loop skips that store, the others leave it for ROW_FWD.
    int accel_step(int f0, int nf, long s, bool first, bool from_ones) {
        const size_t o = (size_t)f0 * n_img();
        double* part = acc_part + (size_t)f0 * acc_blocks() * 2;
        if (!from_ones) {
            HIP_TRY(accel_extrapolate(dtype, off(est, o), off(acc_y, o), off(acc_x, o), part, acc_alpha + f0, n_img(), nf,
                                      s == 0 ? ACC_FRESH : 0, cur()));
            RL_TRY(est_spectrum(f0, nf));
        }
        const Iter it{f0, nf, first, from_ones, /* drop_spectrum */ pair};
        RL_TRY(tv_on() ? tv_iterate(it, /* have_sum */ false, /* rebuild_spectrum */ false) : iterate_chunk(it));   // (est = y_s: the sum is not of it)
        HIP_TRY(accel_reduce(dtype, off(est, o), off(acc_y, o), off(acc_g, o), part, n_img(), nf,
                             (from_ones ? ACC_Y_ONES : 0) | (s > 0 ? ACC_HAVE_PREV : 0), cur()));
        return RL_OK;
    }
    // ---- Poisson I-divergence and the stopping rule (stop_kernels.hpp; rl_deconv_divergence, rl_deconv_iterate_until).  Allocated on
    // first use: the divergence's per-workgroup partials and the frames' D, and -- iterate_until -- the latched estimates and the
    // frames' state, double buffered by check parity.
    double *stop_part = nullptr, *stop_d = nullptr;   // [B][stop_blocks(n_frame)], [B]
    void* stop_result = nullptr;                       // [B][ny][nx]
    StopFrame* stop_state = nullptr;                   // [2][B]
    size_t n_frame() const { return (size_t)V * n_img(); }   // values of one frame's measurement: all its views
    int ensure_divergence() {
        if (!stop_part) RL_TRY(alloc(&stop_part, (size_t)B * stop_blocks(n_frame(), dtype_size(dtype)) * sizeof(double)));
        if (!stop_d) RL_TRY(alloc(&stop_d, (size_t)B * sizeof(double)));
        return RL_OK;
    }
    int ensure_latch() {
        if (!stop_result) RL_TRY(alloc(&stop_result, (size_t)B * n_img() * dtype_size(dtype)));
        if (!stop_state) RL_TRY(alloc(&stop_state, 2 * (size_t)B * sizeof(StopFrame)));
        return RL_OK;
    }
    // scratch = H(est) -- rl_forward's launches, reading the estimate where it is -- and the partials of D(meas || scratch) of every frame
    int divergence_partials() {
        if (sep) {
            RL_TRY(sep_forward(est, scratch, sep_tmp(), B));
        } else {
            RL_TRY(forward_pass(est, scratch, B, spec_a, spec_b, nullptr));
            spec_valid = false;
        }
        HIP_TRY(stop_divergence(dtype, meas, scratch, stop_part, n_frame(), B, cur()));
        return RL_OK;
    }
    bool spec_valid = false;   // spec_a holds rowFFT(est)
    long iterations = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_iter_ms = 0, last_sim_ms = 0;

    enum ColKind { COL_H, COL_HT_VIEW, COL_HT_FUSED };
    // One Richardson-Lucy iteration on frames [f0, f0 + nf), as its four passes and their launches are told of it.
    // first: the estimate is 1 (just filled) -- H(estimate) is spec_ones for every frame, so the column pass of H is skipped and
    //   ROW_RATIO reads the shared spectra (bit for bit what the pass would write);
    // from_ones: (study builds) the ratio of the iteration that starts from estimate = 1 is measurement / H(1), data scale: its
    //   ratio-type spectra carry q_est;
    // drop_spectrum: ROW_UPDATE does not transform the new estimate forward again (pair loop: the last iteration of a long run).
    // est_one: the estimate is 1 and was NOT filled -- ROW_UPDATE takes it as 1 instead of reading it (RowParams::est_one).
    struct Iter { int f0, nf; bool first, from_ones, drop_spectrum; bool est_one = false; };
    // scale of a ratio-type spectrum (ROW_RATIO's output, the H_t columns' input); it == nullptr: a launch outside the loop (rl_adjoint)
    float ratio_scale(const Iter* it) const { return it && it->from_ones ? q_est : q_ratio; }
    // H_t inside a `ratio - 1` iteration: the spectra of residuals (rl_adjoint's input is an image)
    bool residual(ColKind kind, const Iter* it) const { return it && kind != COL_H && sub(); }
    // ---- total-variation regularisation (tv_kernels.hpp, rl_deconv_set_tv): per frame the weights w of the point at hand in one image
    // buffer and the float64 per-workgroup partials of sum est -- allocated when the mode is first switched on.  tv_sum_valid: the
    // partials are of the estimate as it stands (APPLY left them); everything else that writes est clears it.
    double tv_lambda = 0.0, tv_eps_rel = 0.1;
    void* tv_w = nullptr;
    double* tv_part = nullptr;
    bool tv_sum_valid = false;
    bool tv_on() const { return tv_lambda > 0.0; }
    int ensure_tv() {
        if (!tv_w) RL_TRY(alloc(&tv_w, (size_t)B * n_img() * dtype_size(dtype)));
        if (!tv_part) RL_TRY(alloc(&tv_part, (size_t)B * acc_blocks() * sizeof(double)));
        return RL_OK;
    }
    // The regularised step on the frames of `it`: [SUM unless the partials are of the point at hand] -> WEIGHT -> the plan's iteration
    // -> APPLY.  The step from ones has w = 1 exactly (s = 1, every difference 0): no WEIGHT, APPLY only leaves the sum.
    // rebuild_spectrum: the loop reads rowFFT(est), and the spectrum ROW_UPDATE stored is of psi(x), not of psi(x) w.
    int tv_iterate(const Iter& it, bool have_sum, bool rebuild_spectrum) {
        const size_t o = (size_t)it.f0 * n_img();
        double* part = tv_part + (size_t)it.f0 * acc_blocks();
        if (!it.from_ones) {
            if (!have_sum) HIP_TRY(tv_apply(dtype, off(est, o), nullptr, part, ny, nx, it.nf, TV_SUM_ONLY, cur()));
            HIP_TRY(tv_weight(dtype, off(est, o), off(tv_w, o), part, tv_lambda, tv_eps_rel, ny, nx, it.nf, cur()));
            if (rebuild_spectrum) RL_TRY(est_spectrum(it.f0, it.nf));
        }
        RL_TRY(iterate_chunk(it));
        HIP_TRY(tv_apply(dtype, off(est, o), it.from_ones ? nullptr : off(tv_w, o), part, ny, nx, it.nf, it.from_ones ? TV_SUM_ONLY : 0, cur()));
        return RL_OK;
    }
    // ---- frame pairs (conv_kernels.hpp rowpair_body; RLSTED_PAIR): two frames ride through one complex image, the
    // Richardson-Lucy loop of a single-view plan then runs on spectra [pairs][ny][lx] -- no Hermitian packing /
    // splitting around the row transforms.  The simulation and the H / H_t calls keep the per-frame layout.
    bool pair = false;          // the loop that runs: pair_layout && the batch's partners are of comparable brightness (choose_loop)
    bool pair_layout = false;   // the plan holds the pair buffers (psf_hat_pair, spec_ones_pair)
    // A pair's two frames share one complex transform, so f32 rounding error scales with the BRIGHTER partner: a dim frame
    // next to one 1e5 times brighter would carry ~1e5 times its own error through H.  Frames are paired only while every
    // pair's levels (sums of the object / measurement images) are within kPairMaxRatio of each other
    // (RLSTED_PAIR_MAX_RATIO); otherwise the plan runs its per-frame loop, which every pair plan also holds.
    std::vector<double> obj_level, meas_level;   // per frame (host): sum of the object / of the measurement over its views
    bool levels_ok(const std::vector<double>& lv) const {
        if ((int)lv.size() != B) return true;    // nothing known yet
        for (int f = 0; f + 1 < B; f += 2) {
            const double lo = std::min(lv[f], lv[f + 1]), hi = std::max(lv[f], lv[f + 1]);
            if (lo == 0.0 && hi == 0.0) continue;   // two empty frames
            if (!(lo > 0.0) || !std::isfinite(hi) || hi > opt.pair_max_ratio * lo) return false;
        }
        return true;
    }
    void choose_loop(const std::vector<double>& lv) {
        const bool want = pair_layout && levels_ok(lv);
        if (want != pair) {
            pair = want;
            spec_valid = false;   // spec_a holds the other layout's spectra
        }
    }
    // ---- state transitions, named after tests/plan_model.py
    // set_measurement, for a measurement the plan draws from its object: the frames' levels follow the object's, and no pixel is
    // negative (Poisson draws + 1e-9; an earlier upload's negative pixels are gone: sub()).  What else a caller sets differs.
    void set_measurement_from_object() {
        meas_level = obj_level;
        choose_loop(meas_level);
        meas_negative = false;
    }
    // set_estimate: est holds a point with no history; the next iterate rebuilds rowFFT(estimate)
    int set_estimate() {
        est_ready = true;
        spec_valid = false;
        tv_sum_valid = false;
        return accel_reset();
    }
    // The measurement buffer was handed out (rl_deconv_device_ptr which = 1) and may have been written on the device: the per-frame
    // sums are recomputed there before the next run decides between the pair loop and the per-frame loop.
    bool meas_external = false;
    int refresh_meas_levels() {
        if (!meas_external) return RL_OK;
        RL_TRY(ensure_stage());
        std::vector<double> sums((size_t)B * V);
        HIP_TRY(aux_image_sums(dtype, meas, n_img(), (size_t)B * V, stage_sums, ctx->stream));
        HIP_TRY(hipMemcpyAsync(sums.data(), stage_sums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        meas_level.assign((size_t)B, 0.0);
        for (size_t i = 0; i < sums.size(); ++i) meas_level[i / V] += sums[i];
        choose_loop(meas_level);
        RL_TRY(scan_meas_negative());
        meas_external = false;
        return RL_OK;
    }
    // does the measurement on the device hold a negative pixel?  (multi-view plans only: see sub())
    int scan_meas_negative() {
        meas_negative = false;
        if (V < 2 || !sub_one) return RL_OK;
        RL_TRY(ensure_stage());
        int flag = 0;
        HIP_TRY(aux_any_negative(dtype, meas, (size_t)B * V * n_img(), (int*)stage_aux, ctx->stream));
        HIP_TRY(hipMemcpyAsync(&flag, stage_aux, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        meas_negative = flag != 0;
        return RL_OK;
    }
    void *psf_hat_pair = nullptr, *psf_hat_pair_re = nullptr;   // psf_hat at full width: [lx][ly] (transposed layout)
    void* spec_ones_pair = nullptr;                              // column-transformed spectrum of a pair of ones frames
    // Row pitch of a pair spectrum (complex elements): lx, or lx + 32 for the long rows (lx >= 1152).  A pitch of exactly lx
    // makes the row stride (lx * 8 bytes in f32: 18432 / 36864) an EVEN multiple of 256 bytes, and the column kernels' tile
    // rows -- one 64-byte segment per row -- then fall on a fraction of the memory channels; + 256 bytes makes it an odd
    // multiple.  Worth 2-4 % on the long rows, costs 3 % at lx = 576 (4608-byte rows: left alone).
    int pair_pitch = 0;
    size_t n_spec_pair() const { return spec_image_elems(ny, pair_pitch); }
    void* pair_spec(int f0) const { return (char*)spec_a + (size_t)(f0 / 2) * n_spec_pair() * 2 * dtype_size(dtype); }
    // ---- column / row launches.  Layout of the spectra: HALF -- per frame, [ny][pitch] with kx columns -- or PAIR -- two frames in
    // one complex image, [ny][pair_pitch] with lx columns.
    enum Layout { HALF, PAIR };
    // what the column launches share; in_sb / in_sv / order / residual / xs_in / xs_out are their callers' to change
    template <typename T>
    ColParams<T> col_params(Layout lay, ColKind kind, int mode, const void* in, void* out, int images, const Iter* it) {
        ColParams<T> p;
        p.in = (const cx<T>*)in;
        p.out = (cx<T>*)out;
        p.psf_hat = (const cx<T>*)(lay == PAIR ? psf_hat_pair : psf_hat);
        p.psf_hat_re = (const T*)(lay == PAIR ? psf_hat_pair_re : psf_hat_re);
        p.qscale = kind == COL_H ? q_est : ratio_scale(it);
        p.tw = (const cx<T>*)twy;
        p.ny = ny; p.kx = lay == PAIR ? lx : kx; p.pitch = lay == PAIR ? pair_pitch : pitch; p.V = V;
        p.mode = mode;
        p.in_sb = 1; p.in_sv = 0;
        p.images = images;
        p.order = opt.col_order;
        return p;
    }
    // grid: the tiles of p.kx columns x p.images.  cont: second launch of one pass (TimedLaunch)
    template <typename T>
    int launch_col(const ColParams<T>& p, ColKind kind, bool cont = false) {
        const int C = ty->C[dtype];
        const unsigned gx = (unsigned)((p.kx + C - 1) / C), gy = (unsigned)p.images;
        {
            TimedScope t(this, kind == COL_H ? TK_COL_H : TK_COL_HT, true, cont);
            HIP_TRY(ty->launch_col(dtype, &p, gx, gy, cur()));
        }
        if (rl::debug_sync()) {
            hipError_t e = hipStreamSynchronize(cur());
            if (e != hipSuccess)
                return fail(RL_ERR_HIP, "column kernel L=" + std::to_string(ly) + " mode " + std::to_string(p.mode) + " grid " +
                                            std::to_string(gx) + "x" + std::to_string(gy) + ": " + hipGetErrorString(e));
        }
        return RL_OK;
    }
    // kind: COL_H (pair spectrum -> V images; in place when V == 1), COL_HT_VIEW (V == 1, in place) or COL_HT_FUSED
    // (V images summed in the Fourier domain -> pair spectrum)
    template <typename T>
    int col_pair_t(const void* in, void* out, int pairs, ColKind kind, const Iter* it) {
        ColParams<T> p = col_params<T>(PAIR, kind, V == 1 ? COL_PER_IMAGE : (kind == COL_H ? COL_H_MULTI : COL_HT_SUM), in, out, pairs, it);
        p.residual = residual(kind, it) ? 1 : 0;
        return launch_col(p, kind);
    }
    int col_pair(const void* in, void* out, int pairs, ColKind kind, const Iter* it = nullptr) {
        const size_t sp = n_spec_pair() * 2 * dtype_size(dtype);
        const size_t in_per = kind == COL_H ? 1 : (size_t)V, out_per = kind == COL_H ? (size_t)V : 1;
        for (int p0 = 0; p0 < pairs; p0 += kMaxGridY) {
            const int np = std::min((int)kMaxGridY, pairs - p0);
            const void* i = (const char*)in + (size_t)p0 * in_per * sp;
            void* o = (char*)out + (size_t)p0 * out_per * sp;
            RL_TRY(dtype == RL_F32 ? col_pair_t<float>(i, o, np, kind, it) : col_pair_t<double>(i, o, np, kind, it));
        }
        return RL_OK;
    }
    // One row launch.  HALF: `images` launch rows (grid.y).  PAIR: `images` frames (even, or the batch's last odd one), a launch row
    // per (pair, view); spectra and images start at the launch's first pair.
    template <typename T>
    int row_t(Layout lay, int mode, int images, const void* spec_in, void* spec_out, const void* src, void* dst, const void* nrm,
              const void* scale, int views, int in_mod, const Iter* it) {
        RowParams<T> p;
        p.in_mod = in_mod;
        p.sub_one = sub() ? 1 : 0;
        p.est_one = mode == ROW_UPDATE && it && it->est_one ? 1 : 0;
        p.unresolved = unresolved;
        p.qscale = mode == ROW_RATIO ? ratio_scale(it) : q_est;
        p.spec_in = (const cx<T>*)spec_in;
        p.spec_out = (cx<T>*)spec_out;
        p.src = (const T*)src;
        p.dst = (T*)dst;
        p.norm = (const T*)nrm;
        p.scale = (const T*)scale;
        p.tw = (const cx<T>*)twx;
        p.ny = ny; p.nx = nx; p.pitch = lay == PAIR ? pair_pitch : pitch; p.V = views;
        p.frames = images;
        const int Q = tx->Q[dtype];
        const unsigned gx = (unsigned)(((ny + 1) / 2 + Q - 1) / Q), gy = (unsigned)(lay == PAIR ? (images + 1) / 2 * views : images);
        {
            TimedScope t(this, mode == ROW_RATIO ? TK_RATIO : mode == ROW_UPDATE ? TK_UPDATE : mode == ROW_FWD ? TK_FWD : TK_INV);
            HIP_TRY(lay == PAIR ? tx->launch_row_pair(dtype, mode, &p, gy, cur()) : tx->launch_row(dtype, mode, &p, gx, gy, cur()));
        }
        if (rl::debug_sync()) {
            hipError_t e = hipStreamSynchronize(cur());
            if (e != hipSuccess)
                return fail(RL_ERR_HIP, std::string(lay == PAIR ? "pair " : "") + "row kernel mode " + std::to_string(mode) + " L=" +
                                            std::to_string(lx) + " grid " + std::to_string(lay == PAIR ? 1u : gx) + "x" + std::to_string(gy) +
                                            ": " + hipGetErrorString(e));
        }
        return RL_OK;
    }
    // views > 1 (ROW_RATIO of a multi-view plan): one launch image per (pair, view); spectra [pair][view], images [frame][view]
    int row_pair(int mode, int frames, const void* spec_in, void* spec_out, const void* src, void* dst, const void* nrm, int in_mod = 0,
                 int views = 1, const Iter* it = nullptr) {
        const size_t sp = n_spec_pair() * 2 * dtype_size(dtype), im = n_img() * dtype_size(dtype);
        const int step = 2 * ((int)kMaxGridY / views);
        for (int f0 = 0; f0 < frames; f0 += step) {
            const int nf = std::min(step, frames - f0);
            const void* si = spec_in ? (const char*)spec_in + (in_mod > 0 ? 0 : (size_t)(f0 / 2) * views * sp) : nullptr;
            void* so = spec_out ? (char*)spec_out + (size_t)(f0 / 2) * views * sp : nullptr;
            const void* sr = src ? (const char*)src + (size_t)f0 * views * im : nullptr;
            void* ds = dst ? (char*)dst + (size_t)f0 * im : nullptr;
            RL_TRY(dtype == RL_F32 ? row_t<float>(PAIR, mode, nf, si, so, sr, ds, nrm, nullptr, views, in_mod, it)
                                   : row_t<double>(PAIR, mode, nf, si, so, sr, ds, nrm, nullptr, views, in_mod, it));
        }
        return RL_OK;
    }

    // ---- separable strategy (sep_kernels.hip): every view rank 1 (p = u v^T) and small -> direct row + column stencils
    // instead of the FFT path.  RLSTED_SEP: 0 never, 1 (default) when py + px <= 16 (the measured
    // crossover, profiles/r02/separable_vs_fft.json -- the FFT path's cost does not depend on the PSF size), 2 whenever rank 1.
    bool sep = false;
    void *sep_u = nullptr, *sep_v = nullptr;   // [V][py], [V][px] in the plan's dtype
    void *sep_uf = nullptr, *sep_vf = nullptr; // flipped, zero padded to multiples of 8: the one-kernel form's taps
    bool sep_one = false;                      // both passes in one kernel (RLSTED_SEP_ONE, see deconv_build)
    bool sep_direct = false;                   // the one-kernel form as a direct 2-D stencil: PSFs that are not rank 1 (RLSTED_DIRECT)
    int sep2d_(int mode, const void* in, const void* aux, const void* nrm, void* dst, int frames) {
        const bool multi = mode == SEP_SUM_ || mode == SEP_UPDATE_;
        for (int f0 = 0; f0 < frames; f0 += 65535) {
            const int n = std::min(65535, frames - f0);
            const size_t img = n_img() * dtype_size(dtype), in_off = (size_t)f0 * (multi ? V : 1) * img, out_off = (size_t)f0 * (multi ? 1 : V) * img;
            HIP_TRY(sep2d(dtype, opt.sep_th, mode, (const char*)in + in_off, sep_uf, sep_vf, aux ? (const char*)aux + out_off : nullptr, nrm,
                          (char*)dst + out_off, n, ny, nx, py, px, V, cur()));
        }
        return RL_OK;
    }
    void* sep_tmp() const { return spec_b; }    // row-pass results [B*V][ny][nx] (the spectrum buffer is free in this mode)
    int sep_rows_(const void* in, void* out, int images, int in_div) {
        for (int i0 = 0; i0 < images; i0 += 65535 / V * V) {   // grid.z pieces of whole frames
            const int n = std::min(65535 / V * V, images - i0);
            HIP_TRY(sep_rows(dtype, (const char*)in + (size_t)(i0 / in_div) * n_img() * dtype_size(dtype),
                             (char*)out + (size_t)i0 * n_img() * dtype_size(dtype), sep_v, n, ny, nx, px, V, in_div, cur()));
        }
        return RL_OK;
    }
    // mode, tmp [count*(multi ? V : 1)] -> dst [count]; aux: the measurement for SEP_RATIO_
    int sep_cols_(int mode, const void* tmp, const void* aux, const void* nrm, void* dst, int count) {
        const bool multi = mode == SEP_SUM_ || mode == SEP_UPDATE_;
        const int step = multi ? 65535 : 65535 / V * V;
        for (int i0 = 0; i0 < count; i0 += step) {
            const int n = std::min(step, count - i0);
            const size_t in_off = (size_t)i0 * (multi ? V : 1) * n_img() * dtype_size(dtype), out_off = (size_t)i0 * n_img() * dtype_size(dtype);
            HIP_TRY(sep_cols(dtype, mode, (const char*)tmp + in_off, sep_u, aux ? (const char*)aux + out_off : nullptr, nrm,
                             (char*)dst + out_off, n, ny, nx, py, V, cur()));
        }
        return RL_OK;
    }
    // H of nf frames: x [nf] -> out [nf*V] (clamped); tmp: the row-pass results of these frames (their part of sep_tmp())
    int sep_forward(const void* x, void* out, void* tmp, int nf) {
        if (sep_one) return sep2d_(SEP_STORE_, x, nullptr, nullptr, out, nf);
        RL_TRY(sep_rows_(x, tmp, nf * V, V));
        return sep_cols_(SEP_STORE_, tmp, nullptr, nullptr, out, nf * V);
    }
    int sep_iterate(int f0, int nf) {   // ref:520-531
        void* e = off(est, (size_t)f0 * n_img());
        void* ratio = off(scratch, (size_t)f0 * V * n_img());
        void* tmp = off(sep_tmp(), (size_t)f0 * V * n_img());
        if (sep_one) {
            RL_TRY(sep2d_(SEP_RATIO_, e, off(meas, (size_t)f0 * V * n_img()), nullptr, ratio, nf));
            return sep2d_(SEP_UPDATE_, ratio, nullptr, norm, e, nf);
        }
        RL_TRY(sep_rows_(e, tmp, nf * V, V));
        RL_TRY(sep_cols_(SEP_RATIO_, tmp, off(meas, (size_t)f0 * V * n_img()), nullptr, ratio, nf * V));
        RL_TRY(sep_rows_(ratio, tmp, nf * V, 1));
        return sep_cols_(SEP_UPDATE_, tmp, nullptr, norm, e, nf);
    }

    // ---- in-situ kernel timing (rl_deconv_time_cycle): an event pair around every launch of one whole
    // cycle, on the stream the launch goes to, with the slice streams overlapping as in production
    enum TimedKind { TK_COL_H = 0, TK_RATIO, TK_COL_HT, TK_UPDATE, TK_FWD, TK_INV, TK_POISSON, TK_COUNT };
    struct TimedLaunch { int kind; hipEvent_t a, b; bool cont; };   // cont: second launch of one pass (its time adds to the pass)
    bool timing = false;
    std::vector<TimedLaunch> timed;
    std::vector<hipEvent_t> event_pool;
    size_t events_used = 0;
    hipEvent_t pool_event() {
        if (events_used == event_pool.size()) {
            hipEvent_t e = nullptr;
            if (handles.event(&e, hipEventDefault) != RL_OK) return nullptr;
            event_pool.push_back(e);
        }
        return event_pool[events_used++];
    }
    // usage: { TimedScope t(this, kind); launch; }.  ext: the launch goes through fft_kernels.hip's
    // rl_launch, which stamps the kernel's own begin / end on the events (what a kernel trace shows);
    // otherwise the events are recorded on the stream around the launch(es).
    struct TimedScope {
        rl_deconv* h; hipEvent_t a = nullptr, b = nullptr; int kind; bool ext; bool cont = false;
        TimedScope(rl_deconv* h_, int kind_, bool ext_ = true, bool cont_ = false) : h(h_), kind(kind_), ext(ext_), cont(cont_) {
            if (!h->timing || !(a = h->pool_event()) || !(b = h->pool_event())) return;
            if (ext) {
                launch_timing().start = a;
                launch_timing().stop = b;
            } else {
                (void)hipEventRecord(a, h->cur());
            }
        }
        ~TimedScope() {
            if (!a || !b) return;
            if (ext) {
                const bool used = launch_timing().start == nullptr;   // rl_launch consumed them
                launch_timing().start = launch_timing().stop = nullptr;
                if (!used) return;
            } else {
                (void)hipEventRecord(b, h->cur());
            }
            h->timed.push_back({kind, a, b, cont});
        }
    };

    size_t n_img() const { return (size_t)ny * nx; }
    size_t n_spec() const { return spec_image_elems(ny, pitch); }   // complex elements of one spectrum image

    // KernelTable::col_multi: bit 0 COL_H_MULTI, bit 1 COL_HT_SUM (a table without them: V per-image column launches).
    // wave_private_y(): the Fourier-domain view sum exists
    bool wave_private_y() const { return (ty->col_multi[dtype] & 2) != 0; }
    bool h_multi() const { return (ty->col_multi[dtype] & 1) != 0; }
    // The split column pass (conv_kernels.hpp COL_SPLIT_*; f32 multi-view plans on the long column transforms): H transforms a frame's
    // spectrum once for its V views, H_t sums the views' products before one inverse transform (RLSTED_COL_SPLIT=0: A/B knob).
    // H goes through it from three views on: with two the forward half saved (1 + V against 2 V column transforms) does not pay
    // for parking the spectrum -- measured, 2048^2: 2 views 429 (split) against 449 frames/s, 4 views 269 against 258
    bool split_h() const { return V >= 3; }
    bool col_split() const { return opt.col_split && dtype == RL_F32 && V > 1 && ty->split_tile_elems > 0; }
    size_t n_spec_x() const { return (size_t)((kx + ty->C[RL_F32] - 1) / ty->C[RL_F32]) * ty->split_tile_elems; }
    // one half of the split pass over `images` launch rows
    int col_split_launch(int mode, const void* in, void* out, const void* xs_in, void* xs_out, int images, ColKind kind, bool cont,
                         const Iter* it) {
        ColParams<float> p = col_params<float>(HALF, kind, mode, in, out, images, it);
        p.xs_in = (const cx<float>*)xs_in;
        p.xs_out = (cx<float>*)xs_out;
        p.order = 1;
        return launch_col(p, kind, cont);
    }
    // kind COL_H: `in` = the frames' spectra -> out = frames * V images; COL_HT_FUSED: in = frames * V images -> out = frames
    // xs: this slice's part of spec_x (frames * V images of n_spec_x() elements)
    int col_split_pass(const void* in, void* out, void* xs, int frames, ColKind kind, const Iter* it = nullptr) {
        const size_t sp = n_spec() * 2 * sizeof(float), sx = n_spec_x() * 2 * sizeof(float);
        const int step = std::max(1, kMaxGridY / V);
        for (int f0 = 0; f0 < frames; f0 += step) {
            const int nf = std::min(step, frames - f0);
            void* x = (char*)xs + (size_t)f0 * V * sx;
            if (kind == COL_H) {
                RL_TRY(col_split_launch(COL_SPLIT_FWD, (const char*)in + (size_t)f0 * sp, nullptr, nullptr, x, nf, kind, false, it));
                RL_TRY(col_split_launch(COL_SPLIT_INV, nullptr, (char*)out + (size_t)f0 * V * sp, x, nullptr, nf * V, kind, true, it));
            } else {
                RL_TRY(col_split_launch(COL_SPLIT_FWD, (const char*)in + (size_t)f0 * V * sp, nullptr, nullptr, x, nf * V, kind, false, it));
                RL_TRY(col_split_launch(COL_SPLIT_INV_SUM, nullptr, (char*)out + (size_t)f0 * sp, x, nullptr, nf, kind, true, it));
            }
        }
        return RL_OK;
    }
    bool psf_transposed() const { return ty->psf_transposed[dtype] != 0; }   // psf_hat is [view][Kx][Ly]
    template <typename T>
    int col_t(const void* in, void* out, int frames, ColKind kind, const Iter* it) {
        int mode = COL_PER_IMAGE, gy = frames * V;
        if (V > 1 && kind == COL_H && h_multi()) {
            mode = COL_H_MULTI;
            gy = frames;
        } else if (V > 1 && kind == COL_HT_FUSED && wave_private_y()) {
            mode = COL_HT_SUM;
            gy = frames;
        } else if (kind == COL_HT_FUSED && V > 1) {
            return fail(RL_ERR_STATE, "internal: fused H_t needs a wave-private column transform");
        }
        ColParams<T> p = col_params<T>(HALF, kind, mode, in, out, gy, it);
        p.in_sb = kind == COL_H ? 1 : V;
        p.in_sv = kind == COL_H ? 0 : 1;
        p.residual = residual(kind, it) ? 1 : 0;
        return launch_col(p, kind);
    }
    // grid.y carries the image index of a launch: at most kMaxGridY images per launch, larger batches
    // are launched in pieces (whole frames each) with the pointers moved on
    static constexpr int kMaxGridY = 65535;
    int col(const void* in, void* out, int frames, ColKind kind, const Iter* it = nullptr) {
        const size_t sp = n_spec() * 2 * dtype_size(dtype);   // bytes of one spectrum image
        const size_t in_per = kind == COL_H ? 1 : (size_t)V, out_per = kind == COL_HT_FUSED ? 1 : (size_t)V;
        const int step = std::max(1, kMaxGridY / V);
        for (int f0 = 0; f0 < frames; f0 += step) {
            const int nf = std::min(step, frames - f0);
            const void* i = (const char*)in + (size_t)f0 * in_per * sp;
            void* o = (char*)out + (size_t)f0 * out_per * sp;
            RL_TRY(dtype == RL_F32 ? col_t<float>(i, o, nf, kind, it) : col_t<double>(i, o, nf, kind, it));
        }
        return RL_OK;
    }
    int row(int mode, unsigned gy, const void* spec_in, void* spec_out, const void* src, void* dst, const void* nrm,
            const void* scale = nullptr, int views = -1, int in_mod = 0, const Iter* it = nullptr) {
        if (views < 0) views = V;
        const size_t sp = n_spec() * 2 * dtype_size(dtype), im = n_img() * dtype_size(dtype);
        const bool multi = mode == ROW_UPDATE || mode == ROW_ADJ;   // `views` input spectra per image
        const unsigned piece = in_mod > 0 ? (unsigned)(kMaxGridY / in_mod * in_mod) : (unsigned)kMaxGridY;
        for (unsigned g0 = 0; g0 < gy; g0 += piece) {
            const unsigned ng = std::min(piece, gy - g0);
            // (kMaxGridY is a multiple of every in_mod in use only by accident: a shared input is not moved on,
            // and the image index restarts at 0 in each piece -- so pieces must start on a multiple of in_mod)
            const void* si = spec_in ? (const char*)spec_in + (in_mod > 0 ? 0 : (size_t)g0 * (multi ? (size_t)views : 1) * sp) : nullptr;
            void* so = spec_out ? (char*)spec_out + (size_t)g0 * sp : nullptr;
            const void* sr = src ? (const char*)src + (size_t)g0 * im : nullptr;
            void* ds = dst ? (char*)dst + (size_t)g0 * im : nullptr;
            const void* sc = scale ? (const char*)scale + (size_t)g0 * dtype_size(dtype) : nullptr;
            RL_TRY(dtype == RL_F32 ? row_t<float>(HALF, mode, (int)ng, si, so, sr, ds, nrm, sc, views, in_mod, it)
                                   : row_t<double>(HALF, mode, (int)ng, si, so, sr, ds, nrm, sc, views, in_mod, it));
        }
        return RL_OK;
    }

    // Host float64 <-> plan dtype.  The conversion (and the brightness scaling) runs on the
    // device: the host array goes over PCIe as it is, in slices of at most kStageElems
    // doubles, through a device staging buffer.
    static constexpr size_t kStageMax = (size_t)16 << 20;   // at most 128 MiB of float64
    size_t kStageElems = 0;        // elements of the staging buffer: the plan's largest transfer, capped (a 128-square sweep plan: 4 MB)
    double* stage_dev = nullptr;   // [kStageElems] + per-frame sums / targets
    double* stage_aux = nullptr;   // [B] per-frame targets
    double* stage_sums = nullptr;  // [B * V] per-image sums (+ scratch: aux_sums_elems)
    int ensure_stage() {
        if (stage_dev) return RL_OK;
        kStageElems = std::max(n_img(), std::min(kStageMax, (size_t)B * V * n_img()));
        RL_TRY(alloc(&stage_dev, kStageElems * sizeof(double)));
        RL_TRY(alloc(&stage_aux, (size_t)B * sizeof(double), UNCOUNTED));
        RL_TRY(alloc(&stage_sums, aux_sums_elems((size_t)B * V) * sizeof(double), UNCOUNTED));
        return RL_OK;
    }
    // images: `count` images of n_img() pixels; target (host, per image) may be nullptr
    // sums_out (host, optional): the images' sums as uploaded (before any scaling)
    int upload_images(const double* src, void* dst, size_t count, const double* target, std::vector<double>* sums_out = nullptr) {
        RL_TRY(ensure_stage());
        const size_t n = n_img();
        if (n > kStageElems) return fail(RL_ERR_UNSUPPORTED, "image larger than the staging buffer");   // (cannot happen: the buffer holds an image at least)
        const size_t per = kStageElems / n;
        if (sums_out) sums_out->assign(count, 0.0);
        if (target) HIP_TRY(hipMemcpyAsync(stage_aux, target, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        for (size_t f0 = 0; f0 < count; f0 += per) {
            const size_t nf = f0 + per <= count ? per : count - f0;
            HIP_TRY(hipMemcpyAsync(stage_dev, src + f0 * n, nf * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(aux_scale_convert(dtype, stage_dev, (char*)dst + f0 * n * dtype_size(dtype), n, nf,
                                      target ? stage_aux + f0 : nullptr, stage_sums + f0, ctx->stream, target != nullptr || sums_out != nullptr));
            if (sums_out) HIP_TRY(hipMemcpyAsync(sums_out->data() + f0, stage_sums + f0, nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));   // the staging buffer is reused by the next slice
        }
        return RL_OK;
    }
    int upload(const double* src, void* dst, size_t n) {
        if (n % n_img() == 0) return upload_images(src, dst, n / n_img(), nullptr);
        return fail(RL_ERR_INVALID, "internal: upload of a partial image");
    }
    int download(const void* src, double* dst, size_t n) {
        if (dtype == RL_F64) {
            HIP_TRY(hipMemcpyAsync(dst, src, n * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            return RL_OK;
        }
        RL_TRY(ensure_stage());
        for (size_t o = 0; o < n; o += kStageElems) {
            const size_t m = o + kStageElems <= n ? kStageElems : n - o;
            HIP_TRY(aux_to_f64(dtype, (const char*)src + o * dtype_size(dtype), stage_dev, m, ctx->stream));
            HIP_TRY(hipMemcpyAsync(dst + o, stage_dev, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
        return RL_OK;
    }

    char* off(void* base, size_t elems) const { return (char*)base + elems * dtype_size(dtype); }
    // frames of a slice of the batch (cycle_schedule.hpp: the rules and what they measured)
    int chunk_frames() const {
        return rl::chunk_frames({B, V, n_img(), n_spec(), dtype_size(dtype), one_buffer(), accel != RL_ACCEL_NONE, tv_on(), pair, opt.chunk_mb_set,
                                 opt.chunk_mb, opt.lanes, ty->C[dtype], kx});
    }
    // rowFFT(est) of frames [f0, f0 + nf) in the layout of the loop at hand (a stencil plan keeps no spectrum)
    int est_spectrum(int f0, int nf) {
        if (pair) return row_pair(ROW_FWD, nf, nullptr, pair_spec(f0), off(est, (size_t)f0 * n_img()), nullptr, nullptr);
        if (!sep) return row(ROW_FWD, (unsigned)nf, nullptr, est_spec(f0), off(est, (size_t)f0 * n_img()), nullptr, nullptr);
        return RL_OK;
    }
    // estimate = 1 (ref:522).  with_spectrum: also spec_a = rowFFT(estimate); the first iteration does not need
    // it when it takes H(1) from spec_ones (iterate_chunk(first = true)).
    int start_estimate_chunk(int f0, int nf, bool with_spectrum = true) {
        HIP_TRY(aux_fill(dtype, off(est, (size_t)f0 * n_img()), (size_t)nf * n_img(), 1.0, cur()));
        return with_spectrum ? est_spectrum(f0, nf) : RL_OK;
    }
    int ensure_lanes() {
        if (fork) return RL_OK;
        RL_TRY(handles.event(&fork));
        // (equal priorities: lane 0 at the highest stream priority and lane 1 at the lowest measured 17.2 k against 18.1 k frames/s)
        for (int l = 0; l < opt.lanes; ++l) {
            RL_TRY(handles.stream(&lane[l].stream));
            for (hipEvent_t* e : {&lane[l].done, &lane[l].drawn, &lane[l].begun, &lane[l].drawn_ahead}) RL_TRY(handles.event(e));
        }
        return handles.event(&rates_ready);
    }
    // ---- one iteration = four passes (stencil plans: sep_iterate).  Each pass picks its variant from the plan: the pair loop -- the
    // whole iteration in the pair spectra, in place --, one buffer -- one view: every pass maps a spectrum onto itself (a column tile /
    // a row pair is read completely before it is written), so the whole iteration runs in spec_a: a third less working set per frame
    // for the Infinity Cache, and stores that hit lines just read -- or spec_a -> spec_b (V spectra per frame) -> spec_a.
    bool one_buffer() const { return V == 1 && opt.inplace; }
    void* est_spec(int f0) const { return pair ? pair_spec(f0) : off(spec_a, (size_t)f0 * n_spec() * 2); }   // rowFFT(estimate)
    // H(estimate), then the ratios' spectra
    void* ratio_spec(int f0) const { return pair || one_buffer() ? est_spec(f0) : off(spec_b, (size_t)f0 * V * n_spec() * 2); }
    void* parked(int f0) const { return off(spec_x, (size_t)f0 * V * n_spec_x() * 2); }   // the slice's part of spec_x
    // The H_t columns sum the views in the Fourier domain: one inverse column + one inverse row transform per frame, ROW_UPDATE reads
    // one spectrum -- through the split pass (1 + V and V + 1 column transforms per frame instead of 2 V and V + 1 on one register set)
    // or COL_HT_SUM.  Otherwise (f64 plans, RLSTED_FUSE_VIEWS=0) V per-view launches and the pre-summed update.
    bool ht_fused() const { return fuse_views && V > 1 && (col_split() || wave_private_y()); }
    int pass_h(const Iter& it) {        // H(estimate), column part
        if (it.first) return RL_OK;
        if (pair) return col_pair(est_spec(it.f0), ratio_spec(it.f0), (it.nf + 1) / 2, COL_H, &it);
        if (col_split() && split_h()) return col_split_pass(est_spec(it.f0), ratio_spec(it.f0), parked(it.f0), it.nf, COL_H, &it);
        return col(est_spec(it.f0), ratio_spec(it.f0), it.nf, COL_H, &it);   // (a split plan of two views: V whole-pass launches, nothing parked on this side)
    }
    int pass_ratio(const Iter& it) {    // measurement / H(estimate)
        void* r = ratio_spec(it.f0);
        const void* m = off(meas, (size_t)it.f0 * V * n_img());
        if (pair) return row_pair(ROW_RATIO, it.nf, it.first ? spec_ones_pair : r, r, m, nullptr, nullptr, it.first ? 1 : 0, 1, &it);
        return row(ROW_RATIO, (unsigned)(it.nf * V), it.first ? spec_ones : r, r, m, nullptr, nullptr, nullptr, -1, it.first ? V : 0, &it);
    }
    int pass_ht(const Iter& it) {       // H_t, column part
        void* r = ratio_spec(it.f0);
        if (pair) return col_pair(r, r, (it.nf + 1) / 2, COL_HT_VIEW, &it);
        if (!ht_fused()) return col(r, r, it.nf, COL_HT_VIEW, &it);
        if (col_split()) return col_split_pass(r, est_spec(it.f0), parked(it.f0), it.nf, COL_HT_FUSED, &it);
        return col(r, est_spec(it.f0), it.nf, COL_HT_FUSED, &it);
    }
    int pass_update(const Iter& it) {   // est *= H_t / norm, and rowFFT(est) for the next iteration
        void *e = off(est, (size_t)it.f0 * n_img()), *s = est_spec(it.f0);
        if (pair) return row_pair(ROW_UPDATE, it.nf, s, it.drop_spectrum ? nullptr : s, nullptr, e, norm, 0, 1, &it);
        if (ht_fused()) return row(ROW_UPDATE, (unsigned)it.nf, s, s, nullptr, e, norm, nullptr, 1, 0, &it);
        return row(ROW_UPDATE, (unsigned)it.nf, ratio_spec(it.f0), s, nullptr, e, norm, nullptr, -1, 0, &it);
    }
    int iterate_chunk(const Iter& it) {
        if (sep) return sep_iterate(it.f0, it.nf);
        RL_TRY(pass_h(it));
        RL_TRY(pass_ratio(it));
        RL_TRY(pass_ht(it));
        return pass_update(it);
    }
    // noiseless = H(obj) on the device, for rl_deconv_set_object.  Not forward_slice(0, B): a split plan's simulation goes through the
    // split column pass, whose sums round differently from these whole-pass launches (the last bits of noiseless differ).
    int forward_object() {
        if (sep) return sep_forward(obj, noiseless, sep_tmp(), B);
        return forward_pass(obj, noiseless, B, spec_a, spec_b, nullptr);
    }
    // out [n * V] = H(x [n]) on the FFT path: ROW_FWD into the spectrum space a [n], the column pass a -> b [n * V], ROW_INV.
    // xs: the parking space [n * V] of the split column pass; nullptr: the whole pass (forward_object: the two differ in the last bits)
    int forward_pass(const void* x, void* out, int n, void* a, void* b, void* xs) {
        RL_TRY(row(ROW_FWD, (unsigned)n, nullptr, a, x, nullptr, nullptr));
        RL_TRY(xs ? col_split_pass(a, b, xs, n, COL_H) : col(a, b, n, COL_H));
        return row(ROW_INV, (unsigned)(n * V), b, nullptr, nullptr, out, nullptr);
    }
    // noiseless = H(obj) on a slice
    int forward_slice(int f0, int nf) { return forward_frames(f0, nf, off(obj, (size_t)f0 * n_img()), off(noiseless, (size_t)f0 * V * n_img())); }
    // out [nf * V] = H(x [nf]) in the spectrum space of the slice that starts at frame f0 (nf: at most that slice's frames)
    int forward_frames(int f0, int nf, const void* x, void* out) {
        if (sep) return sep_forward(x, out, off(sep_tmp(), (size_t)f0 * V * n_img()), nf);
        void* sb = off(spec_b, (size_t)f0 * V * n_spec() * 2);
        // (frame pairs: the other lane's slice iterates in spec_a in the pair layout, whose slice boundaries are not
        // this layout's -- the simulation then stays in spec_b, in place)
        void* sa = !pair ? off(spec_a, (size_t)f0 * n_spec() * 2) : sb;
        return forward_pass(x, out, nf, sa, sb, col_split() ? parked(f0) : nullptr);   // (a split plan: the split pass)
    }
    // ---- shared simulation (object_classes.hpp): frames that carry the same object are one class -- the benchmark's batch and a
    // sweep's seeds are one object many times over -- and a simulate + deconvolve cycle computes H(object) ONCE per class that its
    // sharing slices hold (forward_classes, at the start of the cycle) instead of every frame's.  The classes' objects and rates
    // live in two compact buffers indexed by class; the Poisson sampler of a sharing slice reads every frame's rates through
    // rate_of.  `noiseless` itself is then not written: it is filled from the compact rates when somebody asks for it
    // (expand_noiseless).  Which slices share is share_layout's rule (representatives at most half the slice's frames); the others
    // simulate every frame as they always did.  RLSTED_SHARE_OBJECTS=0: off.
    std::vector<int> obj_class;            // class of every frame of the object as it was set; empty: not known, nothing is shared
    int n_classes = 0;
    std::vector<SliceShare> share_slices;  // the layout for slices of share_cf frames (0: none built for the object at hand)
    int share_cf = 0;
    std::vector<uint32_t> share_reps, share_rate;   // host copies of the lists below
    struct ShareLists { const unsigned *rep_frames, *rate_of; };   // device, [B] each: the plan's own or those of a batch slot
    ShareLists share_lists{nullptr, nullptr};
    unsigned* share_dev = nullptr;         // [2][B] the plan's own lists
    void *obj_c = nullptr, *noiseless_c = nullptr;   // [share_cap] objects, [share_cap * V] rates
    // spectrum space of the class simulation, its own: the slices' parts of spec_a / spec_b / spec_x belong to the lanes' loops
    void *cls_spec_a = nullptr, *cls_spec_b = nullptr, *cls_spec_x = nullptr;   // [share_cap], [share_cap * V], [share_cap * V] (split plans)
    size_t share_cap = 0;
    int share_classes = 0;                 // compact images in use: the classes the sharing slices of the layout hold
    int last_sim_images = 0;               // images H was computed for in the last cycle (rl_deconv_simulated_images)
    bool noiseless_sparse = false;         // the last simulation left (some) slices' rates in noiseless_c only
    int last_shared_slices = 0, last_slices = 0;
    int grouped_draws = 0, last_grouped_draws = 0;   // slices of this / the last cycle that drew through k_poisson_groups (rl_deconv_grouped_draws)
    int last_draws_ahead = 0;              // slices of the last cycle whose draw went to the context's stream (rl_deconv_draws_ahead)
    bool share_possible() const { return opt.share_objects && !sep && (int)obj_class.size() == B && n_classes < B; }
    // The layout for slices of cf frames from obj_class, on the host: share_slices and the two lists.  Returns the compact images.
    size_t layout_share(int cf) {
        share_cf = 0;
        noiseless_sparse = false;   // (whatever an earlier layout left is replaced by the simulation that follows)
        share_classes = 0;
        share_layout(obj_class, cf, share_slices, share_reps, share_rate);
        return (size_t)class_layout(obj_class, cf, share_slices, share_reps, share_rate);
    }
    // ... and on the device: its lists -- `staged`: already there (rl_batch_submit puts them into the chunk's block), otherwise
    // uploaded here -- and the representatives' objects gathered from obj.  On the context's stream; not while lanes are open.
    int build_share(int cf, const ShareLists* staged) { return place_share(cf, layout_share(cf), staged); }
    int place_share(int cf, size_t total, const ShareLists* staged) {
        if (total > share_cap) {   // (grow only; in groups of 8 images)
            HIP_TRY(hipDeviceSynchronize());
            share_cap = 0;
            RL_TRY(release(&obj_c));
            RL_TRY(release(&noiseless_c));
            RL_TRY(release(&cls_spec_a));
            RL_TRY(release(&cls_spec_b));
            RL_TRY(release(&cls_spec_x));
            const size_t cap = (total + 7) / 8 * 8, sp = n_spec() * 2 * dtype_size(dtype);
            RL_TRY(alloc(&obj_c, cap * n_img() * dtype_size(dtype), SLACK));
            RL_TRY(alloc(&noiseless_c, cap * V * n_img() * dtype_size(dtype), SLACK));
            if (!pair_layout) RL_TRY(alloc(&cls_spec_a, cap * sp, SLACK));   // (a pair plan simulates in place unless its frames' levels forbid pairs: forward_classes)
            RL_TRY(alloc(&cls_spec_b, cap * V * sp, SLACK));
            if (col_split()) {
                const size_t parked_bytes = cap * V * n_spec_x() * 2 * dtype_size(dtype);
                RL_TRY(alloc(&cls_spec_x, parked_bytes));
                HIP_TRY(hipMemsetAsync(cls_spec_x, 0, parked_bytes, ctx->stream));
            }
            share_cap = cap;
        }
        if (staged) {
            share_lists = *staged;
        } else {
            if (!share_dev) RL_TRY(alloc(&share_dev, 2 * (size_t)B * sizeof(unsigned), UNCOUNTED));
            if (total) HIP_TRY(hipMemcpyAsync(share_dev, share_reps.data(), total * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(share_dev + B, share_rate.data(), (size_t)B * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
            share_lists = {share_dev, share_dev + B};
        }
        HIP_TRY(aux_gather_images(dtype, obj, obj_c, share_lists.rep_frames, n_img(), total, 1, ctx->stream));
        if (!staged) HIP_TRY(hipStreamSynchronize(ctx->stream));   // the host lists are the plan's to change again
        share_cf = cf;
        share_classes = (int)total;
        return RL_OK;
    }
    // noiseless_c [n * V] = H(obj_c [n]): the launches forward_frames runs over a slice's frames (the split pass on a split plan:
    // see forward_object), in the class simulation's own spectrum space
    int forward_classes(int n) {
        void* sb = cls_spec_b;
        if (!pair && !cls_spec_a) {   // a pair plan whose frames at hand run the per-frame loop (choose_loop): first use
            RL_TRY(alloc(&cls_spec_a, share_cap * n_spec() * 2 * dtype_size(dtype), SLACK));
            HIP_TRY(hipStreamSynchronize(ctx->stream));   // (the zeroed slack, before another stream's kernels read past the end)
        }
        void* sa = !pair ? cls_spec_a : sb;   // (as forward_frames does)
        return forward_pass(obj_c, noiseless_c, n, sa, sb, col_split() ? cls_spec_x : nullptr);
    }
    // the object was (or may have been) replaced: nothing is known about its frames until somebody classifies them
    void forget_classes() {
        obj_class.clear();
        n_classes = 0;
        share_cf = 0;
        share_classes = 0;
    }
    // every frame's rates into `noiseless`, where a shared simulation left them in the compact buffer (on the context's stream)
    int expand_noiseless() {
        if (!noiseless_sparse) return RL_OK;
        const int cf = share_cf;
        for (int sl = 0, f0 = 0; f0 < B && cf > 0; f0 += cf, ++sl) {
            const int nf = f0 + cf <= B ? cf : B - f0;
            if (share_slices[(size_t)sl].nrep == 0) continue;
            HIP_TRY(aux_gather_images(dtype, noiseless_c, off(noiseless, (size_t)f0 * V * n_img()), share_lists.rate_of + f0, n_img(),
                                      (size_t)nf * V, (unsigned)V, ctx->stream));
        }
        noiseless_sparse = false;
        return RL_OK;
    }
    // Behind a run that failed: the context's stream continues after every lane, and nothing of that run is left for a later one
    // to wait for -- it is all in front of whatever the context's stream takes next.  (A draw that the failed cycle enqueued and
    // no lane waited for is on the context's stream itself.)
    int join_lanes() {
        cycle_state = CycleState{};
        for (const Lane& l : lane) {
            if (!l.stream) continue;
            HIP_TRY(hipEventRecord(l.done, l.stream));
            HIP_TRY(hipStreamWaitEvent(ctx->stream, l.done, 0));
        }
        return RL_OK;
    }
    int join_open_lanes() { return cycle_state.lanes_open ? join_lanes() : RL_OK; }   // after a failed cycle between deferred joins
    // the Poisson draw of a whole cycle: one seed for the batch, or -- rl_batch_submit -- a Philox key per frame (device arrays of B entries)
    struct Draw { int rng_kind; uint64_t seed; const unsigned long long* key_seeds; const unsigned* key_ids; };
    // ---- iteration checkpoints (rl_batch_submit_checkpoints, checkpoint_kernels.hpp): after the iteration that completes k_list[j] a
    // slice casts its frames' estimates to out[j] and leaves their six sums against obj in trace[j] -- both already at the chunk's
    // first task, either may be NULL -- on the slice's own stream, for the chunk's nt real frames only.  The per-workgroup partials
    // [B][blocks][6] are the plan's: a slice writes its own frames' part, and launches that reuse it follow each other in stream order.
    struct Checkpoints { const int* k_list; int n_k; void* const* out; int out_dtype; double* const* trace; int nt; };
    double* cp_part = nullptr;
    int ensure_checkpoint_part() {
        if (cp_part) return RL_OK;
        return alloc(&cp_part, (size_t)B * checkpoint_blocks(n_img(), dtype_size(dtype)) * kCheckpointFields * sizeof(double));
    }
    int take_checkpoint(const Checkpoints& cp, int j, int f0, int nf) {
        const int frames = std::min(f0 + nf, cp.nt) - f0;
        void* dst = cp.out ? cp.out[j] : nullptr;
        double* tr = cp.trace ? cp.trace[j] : nullptr;
        if (frames <= 0 || (!dst && !tr)) return RL_OK;
        const size_t o = (size_t)f0 * n_img();
        double* part = tr ? cp_part + (size_t)f0 * checkpoint_blocks(n_img(), dtype_size(dtype)) * kCheckpointFields : nullptr;
        HIP_TRY(checkpoint_take(dtype, off(est, o), off(obj, o), cp.out_dtype, dst ? (char*)dst + o * dtype_size(cp.out_dtype) : nullptr, part,
                                n_img(), frames, cur()));
        if (tr) HIP_TRY(checkpoint_totals(dtype, part, n_img(), frames, tr + (size_t)f0 * kCheckpointFields, cur()));
        return RL_OK;
    }
    // ---- a run over the slices (cycle_schedule.hpp decides what goes to which stream and behind which event; here it is enqueued)
    struct Run { int k; bool restart; const Draw* draw; const Checkpoints* cp; int cf; };
    hipStream_t stream_of(int s) const { return s == kCtxStream ? ctx->stream : lane[s].stream; }
    hipEvent_t event_of(const StreamOp& op) const {
        const Lane& l = lane[op.lane];
        switch (op.event) {
            case EventKind::FORK: return fork;
            case EventKind::RATES_READY: return rates_ready;
            case EventKind::DONE: return l.done;
            case EventKind::DRAWN: return l.drawn;
            case EventKind::BEGUN: return l.begun;
            case EventKind::DRAWN_AHEAD: return l.drawn_ahead;
            case EventKind::NONE: break;
        }
        return nullptr;
    }
    // A slice's Poisson draw.  shared: every frame draws from its class's rates, which the class simulation left in the compact buffer.
    // ahead: on the context's stream, opt.draw_grid workgroups wide and without a work list.
    int draw_slice(const Draw& d, int sl, int f0, int nf, bool shared, bool ahead) {
        void* ws = ahead ? nullptr : (char*)slice_ws + (size_t)sl * slice_ws_stride;   // this slice's Poisson work list
        TimedScope t(this, TK_POISSON, false);   // (records on cur())
        const hipError_t e = aux_poisson(dtype, shared ? noiseless_c : off(noiseless, (size_t)f0 * V * n_img()), off(meas, (size_t)f0 * V * n_img()),
                                         (unsigned)n_img(), (unsigned)(nf * V), (unsigned)(f0 * V), d.seed, d.rng_kind, ws, cur(),
                                         d.key_seeds ? d.key_seeds + f0 : nullptr, d.key_ids ? d.key_ids + f0 : nullptr, (unsigned)V,
                                         shared ? share_lists.rate_of + f0 : nullptr, ahead ? (unsigned)opt.draw_grid : (unsigned)kPoissonGrid,
                                         opt.poisson_groups);
        if (aux_poisson_groups(opt.poisson_groups, d.rng_kind, shared)) ++grouped_draws;
        return e == hipSuccess ? RL_OK : fail(RL_ERR_HIP, std::string("Poisson kernels: ") + hipGetErrorString(e));
    }
    // (start the estimate of a slice and) its k iterations, with their checkpoints
    int loop_slice(const Run& r, int f0, int nf) {
        const int k = r.k;
        const bool restart = r.restart;
        const bool shortcut = restart && opt.ones_shortcut && spec_ones && k > 0 && !sep;
        // The plain loop's first iteration reads neither the estimate's spectrum (shortcut) nor -- est_one -- the estimate, and its
        // ROW_UPDATE writes every pixel of it: nothing is filled.  The accelerated and the regularised steps read est themselves.
        const bool ones_first = shortcut && !accel && !tv_on();
        if (restart && !ones_first) RL_TRY(start_estimate_chunk(f0, nf, !shortcut));
        // Frame pairs: the last iteration of a run of >= 4 does not transform its estimate forward again (1 of 2 row
        // transforms of that launch, the spectrum store); an rl_deconv_iterate that continues rebuilds it with one ROW_FWD.
        const bool drop = pair && k >= 4;
        int cp_next = 0;   // (est holds x_{i+1} behind every kind of step: the accelerated one ends with its REDUCE, the regularised one with its APPLY)
        for (int i = 0; i < k; ++i) {
            if (accel) RL_TRY(accel_step(f0, nf, acc_steps + i, shortcut && i == 0, restart && i == 0));
            else if (tv_on()) RL_TRY(tv_iterate({f0, nf, shortcut && i == 0, restart && i == 0, /* drop_spectrum */ pair}, i > 0 || tv_sum_valid, true));
            else RL_TRY(iterate_chunk({f0, nf, shortcut && i == 0, restart && i == 0, drop && i == k - 1, ones_first && i == 0}));
            if (r.cp && cp_next < r.cp->n_k && r.cp->k_list[cp_next] == i + 1) RL_TRY(take_checkpoint(*r.cp, cp_next++, f0, nf));
        }
        return RL_OK;
    }
    int enqueue(const StreamOp& op, const Run& r) {
        const int f0 = op.slice * r.cf, nf = f0 + r.cf <= B ? r.cf : B - f0;
        active = stream_of(op.stream);   // (what the launch helpers of a WORK use)
        switch (op.op) {
            case OpKind::WAIT: HIP_TRY(hipStreamWaitEvent(active, event_of(op), 0)); return RL_OK;
            case OpKind::RECORD: HIP_TRY(hipEventRecord(event_of(op), active)); return RL_OK;
            case OpKind::WORK: break;
        }
        switch (op.work) {
            case WorkKind::CLASS_SIM: return forward_classes(share_classes);
            case WorkKind::SIMULATE_SLICE: return forward_slice(f0, nf);
            case WorkKind::DRAW_IN_LANE: return draw_slice(*r.draw, op.slice, f0, nf, op.shared, false);
            case WorkKind::DRAW_AHEAD: return draw_slice(*r.draw, op.slice, f0, nf, op.shared, true);
            case WorkKind::LOOP: return loop_slice(r, f0, nf);
            case WorkKind::NONE: break;
        }
        return fail(RL_ERR_STATE, "internal: a stream operation without a kind");
    }
    // (optionally restart from est = 1 and) run k iterations, slice by slice.  draw: one whole simulate + deconvolve cycle -- each
    // slice first computes noiseless = H(obj) and draws its measurement.  cycle_follows: another cycle follows at once (rl_deconv_bench_cycles).
    int run_slices(int k, bool restart, const Draw* draw = nullptr, bool cycle_follows = false, const Checkpoints* cp = nullptr) {
        const int cf = chunk_frames();
        if (accel && restart) RL_TRY(accel_reset());   // each run from ones (a task of rl_batch_run included) starts a fresh history
        // the slices' representatives (a layout for another slice size is rebuilt; not between cycles whose lanes are still running)
        if (draw && share_possible() && share_cf != cf && !cycle_state.lanes_open) RL_TRY(build_share(cf, nullptr));
        CycleInputs in;
        in.B = B; in.cf = cf; in.lanes = opt.lanes; in.V = V;
        in.draws = draw != nullptr;
        in.share = share_possible() && share_cf == cf;
        in.share_classes = share_classes;
        in.share_slices = share_slices.data();
        in.draw_ahead = opt.draw_ahead;
        in.cycle_follows = cycle_follows;
        in.before = cycle_state;
        cycle_schedule(in, schedule);
        if (schedule.forks) RL_TRY(ensure_lanes());
        if (draw) {   // one Poisson work list per slice: slices on different lanes run at the same time
            const size_t stride = (aux_poisson_workspace_bytes((size_t)cf * V * n_img()) + 255) / 256 * 256;
            if (slice_ws_bytes < stride * schedule.slices) {
                HIP_TRY(hipDeviceSynchronize());
                slice_ws_bytes = 0;
                RL_TRY(release(&slice_ws));
                RL_TRY(alloc(&slice_ws, stride * schedule.slices));
                slice_ws_bytes = stride * schedule.slices;
            }
            slice_ws_stride = stride;
        }
        struct ActiveGuard {   // whatever path leaves this function, the launch helpers are back on the context's stream
            hipStream_t& a;
            ~ActiveGuard() { a = nullptr; }
        } active_guard{active};
        const Run run{k, restart, draw, cp, cf};
        grouped_draws = 0;
        int rc = RL_OK;   // the first failure: no further work is enqueued behind it, the join is
        for (const StreamOp& op : schedule.ops) {
            if (rc != RL_OK && !op.join) continue;
            const int r = enqueue(op, run);
            if (rc == RL_OK) rc = r;
        }
        active = nullptr;
        if (rc != RL_OK) {
            const std::string keep = rl::last_error();
            if (!schedule.joins) (void)join_lanes();   // (lanes that were to stay open)
            cycle_state = CycleState{};
            rl::last_error() = keep;
            return rc;
        }
        cycle_state = schedule.after;
        if (draw) {
            last_draws_ahead = schedule.draws_ahead;
            last_grouped_draws = grouped_draws;
            noiseless_sparse = schedule.shared_slices > 0;
            last_shared_slices = schedule.shared_slices;
            last_slices = schedule.slices;
            last_sim_images = schedule.sim_images;
        }
        if (restart) {
            est_ready = true;
            spec_valid = true;
            iterations = 0;
        }
        if (pair && k >= 4) spec_valid = false;   // the last iteration left no spectrum behind
        if (accel) {
            spec_valid = false;   // (a plain iterate after a change of mode rebuilds it; an accelerated one transforms y)
            acc_steps += k;
        }
        if (tv_on()) spec_valid = false;   // (APPLY changed est after ROW_UPDATE stored its spectrum; a TV step transforms its own point)
        if (k > 0 || restart) tv_sum_valid = tv_on() && !accel && k > 0;   // (accelerated: est is x_k, the next point y_k is formed from it)
        iterations += k;
        return RL_OK;
    }
};

namespace rl {
// the context a plan was created on (ctx.hpp): what stack_api.cpp, which sees the plan through the C ABI only, enqueues on
rl_ctx* plan_ctx(rl_deconv* h) { return h ? h->ctx : nullptr; }
}  // namespace rl

extern "C" {

const char* rl_last_error(void) { return rl::last_error().c_str(); }
int rl_version(void) { return 100; }

int rl_device_count(int* count) {
    if (!count) return fail(RL_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(RL_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return RL_OK;
}

int rl_host_alloc(size_t bytes, void** out) {
    if (!out) return fail(RL_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (bytes == 0) return fail(RL_ERR_INVALID, "bytes == 0");
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return RL_OK;
}

int rl_host_free(void* p) {
    if (p) HIP_TRY(hipHostFree(p));
    return RL_OK;
}

int rl_fft_length_for(int n) {
    for (int L : kLengths)
        if (L >= n) return L;
    return 0;
}

// A sweep deals its plan groups to several contexts of a GPU (sweep.py), each with a stream of its own plus its plans' slice and copy
// streams.  The HIP runtime maps a process's streams onto 4 hardware queues unless GPU_MAX_HW_QUEUES says otherwise; with 8 the
// small launches of neighbouring groups overlap further (BASELINE config 4, 1152 tasks: 29.7 -> 26.4-26.8 ms on 4-6 contexts,
// profiles/r04/sweep_hw_queues.log).  The runtime reads the variable when it initialises -- at this process's first HIP call --
// so the default is set when the library is loaded, and only if the user has not set it.
__attribute__((constructor)) static void rl_runtime_defaults() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

int rl_ctx_create(int device, rl_ctx** out) {
    if (!out) return fail(RL_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(RL_ERR_INVALID, "no such device");
    HIP_TRY(hipSetDevice(device));
    rl_ctx* c = new rl_ctx;
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(RL_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    *out = c;
    return RL_OK;
}

int rl_ctx_destroy(rl_ctx* c) {
    if (!c) return RL_OK;
    (void)hipSetDevice(c->device);
    for (auto& kv : c->tw) (void)hipFree(kv.second);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return RL_OK;
}

int rl_ctx_synchronize(rl_ctx* c) {
    if (!c) return fail(RL_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RL_OK;
}

int rl_chunk_bytes(rl_ctx* c, int which, size_t bytes) {
    size_t* cap = c ? c->chunk_cap(which) : nullptr;
    if (!cap || bytes < 1) return fail(RL_ERR_INVALID, "NULL context, an unknown chunk cap or a cap of 0 bytes");
    *cap = bytes;
    return RL_OK;
}

int rl_chunks_run(rl_ctx* c, int which) { return c && which >= 0 && which < RL_CHUNK_COUNT ? c->chunks_run[which] : 0; }

int rl_deconv_destroy(rl_deconv* h) {
    if (!h) return RL_OK;
    (void)hipSetDevice(h->ctx->device);
    // nothing of this plan may still be running when its buffers go away (slice and copy streams included)
    (void)hipStreamSynchronize(h->ctx->stream);
    for (hipStream_t s : h->handles.streams) (void)hipStreamSynchronize(s);
    for (const rl_deconv::Owned& o : h->owned) (void)hipFree(o.p);
    for (rl_deconv::BatchSlot& sl : h->bslot)
        if (sl.host) (void)hipHostFree(sl.host);
    for (hipEvent_t e : h->handles.events) (void)hipEventDestroy(e);
    for (hipStream_t s : h->handles.streams) (void)hipStreamDestroy(s);
    delete h;
    return RL_OK;
}

// PSF spectra by direct DFT of the (py x px) support in float64 on the device: `width` spectrum columns at row pitch `pitch` into
// `hat` (transposed: [view][width][ly]).  re != nullptr: also their real parts, in a buffer of the plan's, and
// *imag_ratio = max |im| / max |z| of the spectrum.
static int build_psf_hat(rl_deconv* h, const double* psfs, void* hat, int width, int pitch, int transposed, void** re, double* imag_ratio) {
    rl_ctx* ctx = h->ctx;
    const size_t V = (size_t)h->V, np = V * h->py * h->px;
    {
        TempBuffers tmp;
        void *wy = nullptr, *wx = nullptr, *psf_dev = nullptr, *s1 = nullptr;
        RL_TRY(ctx->plain_twiddles(h->ly, &wy));
        RL_TRY(ctx->plain_twiddles(h->lx, &wx));
        RL_TRY(tmp.get(&psf_dev, np * 8));
        RL_TRY(tmp.get(&s1, V * h->py * width * 16));
        HIP_TRY(hipMemcpyAsync(psf_dev, psfs, np * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(aux_psf_spectrum(h->dtype, (const double*)psf_dev, wx, wy, s1, hat, h->V, h->py, h->px, h->ly, h->lx, width, pitch,
                                 transposed, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (!re) return RL_OK;
    // (the real parts are allocated once the transform's temporaries are gone: the order decides where the plan's large buffers land in
    // device memory -- 4 % of a 2048^2 x 4 views cycle, profiles/r06/refactor_ab.log)
    TempBuffers tmp;
    const size_t nz = V * (size_t)width * h->ly;
    double* stats = nullptr;
    double hs[2] = {1.0, 1.0};
    RL_TRY(h->alloc(re, nz * dtype_size(h->dtype), rl_deconv::SLACK));
    RL_TRY(tmp.get((void**)&stats, sizeof(hs)));
    HIP_TRY(aux_split_real(h->dtype, hat, nz, *re, stats, ctx->stream));
    HIP_TRY(hipMemcpyAsync(hs, stats, sizeof(hs), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *imag_ratio = hs[1] > 0 ? hs[0] / hs[1] : 0.0;
    return RL_OK;
}

static int deconv_build(rl_deconv* h, const double* psfs) {
    rl_ctx* ctx = h->ctx;
    const int cy_lo = (h->py - 1) / 2, cy_hi = h->py - 1 - cy_lo;
    const int cx_lo = (h->px - 1) / 2, cx_hi = h->px - 1 - cx_lo;
    // wrap-free sizes: L >= n + max(offset below, offset above the PSF centre)
    h->ly = rl_fft_length_for(h->ny + (cy_lo > cy_hi ? cy_lo : cy_hi));
    h->lx = rl_fft_length_for(h->nx + (cx_lo > cx_hi ? cx_lo : cx_hi));
    if (!h->ly || !h->lx)
        return fail(RL_ERR_UNSUPPORTED, "image + PSF half width exceeds the largest built transform length (4608)");
    h->ty = table_for(h->ly);
    h->tx = table_for(h->lx);
    h->kx = h->lx / 2 + 1;
    h->pitch = (h->kx + 7) / 8 * 8;
    RL_TRY(ctx->prepare(h->ty));
    RL_TRY(ctx->prepare(h->tx));
    RL_TRY(ctx->twiddles(h->ty, h->dtype, &h->twy, true));
    RL_TRY(ctx->twiddles(h->tx, h->dtype, &h->twx));
    const size_t es = dtype_size(h->dtype), B = (size_t)h->B, V = (size_t)h->V;
    // (measured, pitch lx against lx + 32: 512^2 18.7 k against 18.1 k frames/s, 2048^2 690 against 716, 4096^2 K = 100 28.0 against 28.6)
    h->pair_pitch = h->lx + (h->lx >= 1152 ? 32 : 0);
    struct Req { void** p; size_t n; };
    const Req reqs[] = {
        {&h->psf_hat, V * h->ly * h->pitch * 2 * es},   // (spec_a: the frames' half spectra or the pairs' full ones)
        {&h->spec_a, std::max(B * h->n_spec(), (B + 1) / 2 * h->n_spec_pair()) * 2 * es},
        {&h->spec_b, B * V * h->n_spec() * 2 * es},   {&h->obj, B * h->n_img() * es},
        {&h->noiseless, B * V * h->n_img() * es},     {&h->meas, B * V * h->n_img() * es},
        {&h->est, B * h->n_img() * es},               {&h->norm, h->n_img() * es},
        {&h->scratch, std::max(B * V * h->n_img() * es, aux_poisson_workspace_bytes(B * V * h->n_img()))}};   // also the Poisson work list
    for (const Req& r : reqs) RL_TRY(h->alloc(r.p, r.n, rl_deconv::SLACK));
    RL_TRY(h->alloc(&h->unresolved, sizeof(unsigned long long), rl_deconv::UNCOUNTED));
    HIP_TRY(hipMemsetAsync(h->unresolved, 0, sizeof(unsigned long long), ctx->stream));
    RL_TRY(h->handles.event(&h->ev0, hipEventDefault));
    RL_TRY(h->handles.event(&h->ev1, hipEventDefault));

    // A point-symmetric PSF (every PSF of the reference: symmetric "to 1e-15") has a real spectrum.
    // Where the imaginary parts are rounding noise (<= 1e-12 of the largest value; in f32 they vanish against
    // the real parts' own rounding) the wave-private column kernels multiply by the real parts alone: half the
    // multiplier bytes per column launch.  RLSTED_REAL_PSF=0 keeps the complex multiplier.
    RL_TRY(build_psf_hat(h, psfs, h->psf_hat, h->kx, h->pitch, h->ty->psf_transposed[h->dtype],
                         h->psf_transposed() && h->opt.real_psf ? &h->psf_hat_re : nullptr, &h->psf_hat_imag_ratio));
    if (h->psf_hat_imag_ratio > 1e-12) RL_TRY(h->release(&h->psf_hat_re));
    // The split column pass parks B * V column spectra (24 MB per 2048^2 image).  The set-up below runs it on ONE frame (H(1)); the
    // full allocation follows the strategy selection further down: a plan that ends on the separable stencils never touches it.
    if (h->col_split()) {
        const size_t n = V * h->n_spec_x() * 2 * es;
        RL_TRY(h->alloc(&h->spec_x, n, rl_deconv::UNCOUNTED));
        HIP_TRY(hipMemsetAsync(h->spec_x, 0, n, ctx->stream));
    }
    // H_t(ones), line_sted_tools.py:589-592: sum_v clamp(conv(ones, psf_v))
    HIP_TRY(aux_fill(h->dtype, h->est, h->n_img(), 1.0, ctx->stream));
    {
        // (study builds: the spectra of a frame of ones have DC = pixels x sum(psf), not the data's)
        const float keep_q = h->q_est;
        double psf_sum = 1.0;
        for (size_t v = 0; v < V; ++v) {
            double t = 0.0;
            for (size_t i = 0; i < (size_t)h->py * h->px; ++i) t += psfs[v * h->py * h->px + i];
            psf_sum = std::max(psf_sum, t);
        }
        if (h->opt.q_exp_est_set) h->q_est = std::ldexp(1.0f, 14 - (int)std::ceil(std::log2((double)h->n_img() * psf_sum)) - 1);
        RL_TRY(h->row(ROW_FWD, 1, nullptr, h->spec_a, h->est, nullptr, nullptr));
        RL_TRY(h->col(h->spec_a, h->spec_b, 1, rl_deconv::COL_H));
        RL_TRY(h->row(ROW_ADJ, 1, h->spec_b, nullptr, nullptr, h->norm, nullptr));
        h->q_est = keep_q;
        // spec_b now holds the column-transformed spectra of H(1), one per view: every frame's first iteration
        const size_t ones_bytes = V * h->n_spec() * 2 * es;
        RL_TRY(h->alloc(&h->spec_ones, ones_bytes, rl_deconv::SLACK));
        HIP_TRY(hipMemcpyAsync(h->spec_ones, h->spec_b, ones_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // ---- f32 plans: the normaliser to float64 rounding from the PSFs' integral images (aux_box_norm) ----
    if (h->dtype == RL_F32) {
        std::vector<double> integ;
        box_integral_images(psfs, V, h->py, h->px, integ);   // sep_taps.hpp
        TempBuffers tmp;
        double* integ_dev = nullptr;
        RL_TRY(tmp.get((void**)&integ_dev, integ.size() * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(integ_dev, integ.data(), integ.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(aux_box_norm(h->dtype, integ_dev, h->norm, h->V, h->py, h->px, h->ny, h->nx, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    // ---- strategy selection: direct separable stencils when every view is rank 1 and small (py + px <= 16: the measured
    // crossover, profiles/r02/separable_vs_fft.json) ----
    const int sep_mode = h->opt.sep;
    if (sep_mode > 0 && (sep_mode > 1 || h->py + h->px <= 16) && sep_two_pass_fits(h->dtype, h->py, h->px)) {
        const size_t py = h->py, px = h->px;
        std::vector<double> u, vv;
        const bool rank1 = sep_rank1_factors(psfs, V, py, px, u, vv);   // sep_taps.hpp
        if (rank1) {
            RL_TRY(h->upload_taps(&h->sep_u, u));
            RL_TRY(h->upload_taps(&h->sep_v, vv));
            h->sep = true;
            // RLSTED_SEP_ONE: 0 two passes, 1 (default) one kernel up to 24 taps a side (beyond, the two-pass form is
            // faster: profiles/r02/separable_vs_fft.json), 2 one kernel whenever the tile fits LDS
            const bool want_one = h->opt.sep_one >= 2 || (h->opt.sep_one == 1 && std::max(py, px) <= 24);
            if (want_one && sep2d_fits(h->dtype, h->opt.sep_th, h->py, h->px, (int)V)) {
                std::vector<double> uf, vf;
                sep_flipped_taps(u, vv, V, py, px, uf, vf);
                RL_TRY(h->upload_taps(&h->sep_uf, uf));
                RL_TRY(h->upload_taps(&h->sep_vf, vf));
                h->sep_one = true;
            }
            // H_t(ones) through the same stencils (ref:589-592); the V copies of ones live in scratch
            HIP_TRY(aux_fill(h->dtype, h->scratch, V * h->n_img(), 1.0, ctx->stream));
            if (h->sep_one) {
                RL_TRY(h->sep2d_(SEP_SUM_, h->scratch, nullptr, nullptr, h->norm, 1));
            } else {
                RL_TRY(h->sep_rows_(h->scratch, h->sep_tmp(), (int)V, 1));
                RL_TRY(h->sep_cols_(SEP_SUM_, h->sep_tmp(), nullptr, nullptr, h->norm, 1));
            }
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
    }
    // ---- ... or a direct 2-D stencil when the views are small but not rank 1 (sep_kernels.hip k_sep2d DIRECT): py * px multiply-adds per
    // pixel and view, all of one sign for a non-negative PSF -- the relative accuracy an FFT convolution cannot give a dark region
    // (DESIGN.md section 3b).  RLSTED_DIRECT: 0 never, 1 (default) up to 49 taps (where it is also the faster
    // path), 2 whenever the tile fits LDS (f32 plans on sparse samples with PSFs up to ~15 x 15: 2x the FFT path's time at 11 x 11).
    {
        const int direct_mode = h->opt.direct;
        if (!h->sep && sep_mode > 0 && direct_mode > 0 && (direct_mode > 1 || h->py * h->px <= 49) && h->py * h->px <= 1024 &&
            direct2d_fits(h->dtype, h->opt.sep_th, h->py, h->px, (int)V)) {
            std::vector<double> f;
            sep_direct_taps(psfs, V, h->py, h->px, f);
            RL_TRY(h->upload_taps(&h->sep_uf, f));
            h->sep = h->sep_one = h->sep_direct = true;      // (sep_vf stays null: that is how sep2d tells the two forms apart)
            HIP_TRY(aux_fill(h->dtype, h->scratch, V * h->n_img(), 1.0, ctx->stream));
            RL_TRY(h->sep2d_(SEP_SUM_, h->scratch, nullptr, nullptr, h->norm, 1));      // H_t(ones) through the same stencil (ref:589-592)
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
    }
    if (h->col_split()) {   // (the one-frame parking space of the set-up -> the plan's, unless the stencils took over)
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        RL_TRY(h->release(&h->spec_x));
        if (!h->sep) {
            const size_t n = B * V * h->n_spec_x() * 2 * es;
            RL_TRY(h->alloc(&h->spec_x, n));
            HIP_TRY(hipMemsetAsync(h->spec_x, 0, n, ctx->stream));
        }
    }
    // ---- frame pairs for the Richardson-Lucy loop (single view, even batch, wave-private lengths) ----
    // Default: f32 plans (the throughput mode).  f64 plans keep every frame's arithmetic independent of its neighbour in the
    // batch (a pair's two frames share rounding errors: 1e-16-level differences with the partner frame).
    // Multi-view plans: built and tested (RLSTED_PAIR=1), no gain (512^2, 4 views: 30.0 ms per 64 frames x 20 iterations either
    // way -- the multi-view column kernels set the pace), so the default pairs single-view plans only.
    // Long transforms (L >= 1152, one workgroup-synchronous row transform per workgroup): built and tested too, 2048^2 -3.5 %,
    // 4096^2 -12 % time per iteration -- but the per-frame loop's Hermitian split averages the two mirrored halves of every
    // row spectrum, the pair loop does not, and where f32 has no margin left that shows: white noise at 2048^2, K = 20,
    // 8.8e-6 -> 1.05e-5 against the f64 plan.  Default there: per frame (RLSTED_PAIR=1 pairs them).
    const bool pair_views_ok = V == 1 && h->opt.inplace && h->B >= 2;   // (a single frame has no partner -- and the set-up below fills two frames of ones)
    // an odd batch leaves its last pair half empty: allowed where the pair spectra still fit the per-frame buffers
    if (h->opt.pair && !h->sep && pair_views_ok && h->tx->launch_row_pair && h->psf_transposed()) {
        double imag_ratio = 0;
        RL_TRY(h->alloc(&h->psf_hat_pair, V * (size_t)h->lx * h->ly * 2 * es, rl_deconv::SLACK));
        // (the half-width spectra are real: so are the full ones)
        RL_TRY(build_psf_hat(h, psfs, h->psf_hat_pair, h->lx, h->lx, 1, h->psf_hat_re ? &h->psf_hat_pair_re : nullptr, &imag_ratio));
        h->pair = h->pair_layout = true;
        // H(1 + i) of a pair of ones frames, column part (one spectrum per view): what every pair's first iteration reads
        const size_t ones_bytes = V * h->n_spec_pair() * 2 * es;
        RL_TRY(h->alloc(&h->spec_ones_pair, ones_bytes, rl_deconv::SLACK));
        HIP_TRY(aux_fill(h->dtype, h->est, 2 * h->n_img(), 1.0, ctx->stream));
        RL_TRY(h->row_pair(ROW_FWD, 2, nullptr, h->spec_a, h->est, nullptr, nullptr));
        RL_TRY(h->col_pair(h->spec_a, V == 1 ? h->spec_a : h->spec_b, 1, rl_deconv::COL_H));
        HIP_TRY(hipMemcpyAsync(h->spec_ones_pair, V == 1 ? h->spec_a : h->spec_b, ones_bytes, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return RL_OK;
}

int rl_deconv_create(rl_ctx* ctx, const double* psfs, int n_psf, int py, int px, int batch, int ny, int nx, int dtype,
                     rl_deconv** out) {
    return rl_deconv_create_with(ctx, psfs, n_psf, py, px, batch, ny, nx, dtype, nullptr, out);
}

int rl_deconv_create_with(rl_ctx* ctx, const double* psfs, int n_psf, int py, int px, int batch, int ny, int nx, int dtype,
                          const char* options, rl_deconv** out) {
    if (!ctx || !psfs || !out) return fail(RL_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (n_psf < 1 || py < 1 || px < 1 || batch < 1 || ny < 1 || nx < 1) return fail(RL_ERR_INVALID, "non-positive size");
    if (!dtype_ok(dtype)) return fail(RL_ERR_INVALID, "dtype must be RL_F32 or RL_F64");
    if (n_psf > rl_deconv::kMaxGridY) return fail(RL_ERR_UNSUPPORTED, "more than 65535 views");
    OptionLookup lookup;
    std::string bad;
    if (!lookup.parse(options, &bad)) return fail(RL_ERR_INVALID, bad);
    const PlanOptions opt = plan_options(lookup, dtype, n_psf, (int)kPoissonGrid, RL_SPEC_QUANT);
    if (const std::string* name = lookup.unasked()) return fail(RL_ERR_INVALID, "option '" + *name + "' is no switch of a plan");
    HIP_TRY(hipSetDevice(ctx->device));
    rl_deconv* h = new rl_deconv;
    h->ctx = ctx;
    h->V = n_psf; h->py = py; h->px = px; h->B = batch; h->ny = ny; h->nx = nx; h->dtype = dtype;
    h->opt = opt;
    if (h->opt.q_exp_est_set) h->q_est = std::ldexp(1.0f, 14 - h->opt.q_exp_est);
    if (h->opt.q_exp_ratio_set) h->q_ratio = std::ldexp(1.0f, 14 - h->opt.q_exp_ratio);
    h->fuse_views = h->opt.fuse_views < 0 ? dtype == RL_F32 : h->opt.fuse_views != 0;
    {   // ratio - 1 needs H_t(ones) == the normaliser: every PSF value >= 0 (and not the 16-bit storage study, whose scales assume ratio spectra)
        bool nonneg = true;
        for (size_t i = 0; i < (size_t)n_psf * py * px && nonneg; ++i) nonneg = psfs[i] >= 0.0;
        // (RLSTED_FUSE_VIEWS=0 selects the reference's per-view clamp in H_t: `ratio - 1` clamps the view sum, so it is off then)
        const bool per_view_clamp = n_psf > 1 && h->opt.fuse_views == 0;
        h->sub_one = h->opt.sub_one && nonneg && !per_view_clamp;
    }
    int r = deconv_build(h, psfs);
    if (r != RL_OK) {
        std::string keep = rl::last_error();
        rl_deconv_destroy(h);
        rl::last_error() = keep;
        return r;
    }
    *out = h;
    return RL_OK;
}

int rl_deconv_info(const rl_deconv* h, int* ly, int* lx, int* pitch, size_t* device_bytes) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    if (ly) *ly = h->ly;
    if (lx) *lx = h->lx;
    if (pitch) *pitch = h->pitch;
    if (device_bytes) *device_bytes = h->bytes;
    return RL_OK;
}

int rl_deconv_set_object(rl_deconv* h, const double* obj, const double* total_brightness) {
    if (!h || !obj) return fail(RL_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->ctx->device));
    // :505-506  obj *= total_brightness / obj.sum(), per frame, on the device
    RL_TRY(h->upload_images(obj, h->obj, (size_t)h->B, total_brightness, &h->obj_level));
    if (total_brightness) h->obj_level.assign(total_brightness, total_brightness + h->B);   // the frames' sums after scaling
    // Frames with the same pixels and the same target are the same object on the device too: a frame's scale is target / sum, and
    // its sum is taken in an order that depends on the frame alone (k_frame_sums; which of its two forms runs is decided by the
    // frame size, the same for every piece of an upload: pieces of 128 MiB hold at most 16 frames of the size that takes the chunked one).
    h->forget_classes();
    if (h->opt.share_objects && !h->sep) h->n_classes = classify_by_pixels(obj, h->n_img(), h->B, total_brightness, h->obj_class);
    HIP_TRY(hipEventRecord(h->ev0, h->ctx->stream));
    RL_TRY(h->forward_object());
    h->noiseless_sparse = false;
    if (h->share_possible()) RL_TRY(h->build_share(h->chunk_frames(), nullptr));
    HIP_TRY(hipEventRecord(h->ev1, h->ctx->stream));
    HIP_TRY(hipEventSynchronize(h->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->last_sim_ms = ms;
    h->have_obj = true;
    h->spec_valid = false;
    return RL_OK;
}

int rl_deconv_simulate(rl_deconv* h, int rng_kind, uint64_t seed) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    if (!h->have_obj) return fail(RL_ERR_STATE, "rl_deconv_set_object has not been called");
    if (rng_kind != RL_RNG_NONE && rng_kind != RL_RNG_PHILOX) return fail(RL_ERR_INVALID, "unknown rng_kind");
    HIP_TRY(hipSetDevice(h->ctx->device));
    RL_TRY(h->expand_noiseless());
    HIP_TRY(aux_poisson(h->dtype, h->noiseless, h->meas, (unsigned)h->n_img(), (unsigned)(h->B * h->V), 0, seed, rng_kind,
                        h->scratch, h->ctx->stream));
    HIP_TRY(hipStreamSynchronize(h->ctx->stream));
    h->set_measurement_from_object();
    h->have_meas = true;
    h->meas_external = false;
    h->est_ready = false;
    return RL_OK;
}

int rl_deconv_simulate_keyed(rl_deconv* h, int rng_kind, const uint64_t* seeds, const uint32_t* image_ids) {
    if (!h || !seeds || !image_ids) return fail(RL_ERR_INVALID, "NULL argument");
    if (!h->have_obj) return fail(RL_ERR_STATE, "rl_deconv_set_object has not been called");
    if (rng_kind != RL_RNG_NONE && rng_kind != RL_RNG_PHILOX) return fail(RL_ERR_INVALID, "unknown rng_kind");
    for (int f = 0; f < h->B; ++f)   // image index = id * V + view must fit the 32-bit Philox counter word
        if ((uint64_t)image_ids[f] * (uint64_t)h->V + (uint64_t)h->V > 0xffffffffull) return fail(RL_ERR_INVALID, "image id too large");
    HIP_TRY(hipSetDevice(h->ctx->device));
    if (!h->key_seeds) RL_TRY(h->alloc(&h->key_seeds, (size_t)h->B * sizeof(uint64_t), rl_deconv::UNCOUNTED));
    if (!h->key_ids) RL_TRY(h->alloc(&h->key_ids, (size_t)h->B * sizeof(uint32_t), rl_deconv::UNCOUNTED));
    HIP_TRY(hipMemcpyAsync(h->key_seeds, seeds, (size_t)h->B * sizeof(uint64_t), hipMemcpyHostToDevice, h->ctx->stream));
    HIP_TRY(hipMemcpyAsync(h->key_ids, image_ids, (size_t)h->B * sizeof(uint32_t), hipMemcpyHostToDevice, h->ctx->stream));
    RL_TRY(h->expand_noiseless());
    HIP_TRY(aux_poisson(h->dtype, h->noiseless, h->meas, (unsigned)h->n_img(), (unsigned)(h->B * h->V), 0, 0, rng_kind,
                        h->scratch, h->ctx->stream, (const unsigned long long*)h->key_seeds, (const unsigned*)h->key_ids,
                        (unsigned)h->V));
    HIP_TRY(hipStreamSynchronize(h->ctx->stream));   // the host arrays may go away
    h->set_measurement_from_object();
    h->have_meas = true;
    h->meas_external = false;
    h->est_ready = false;
    return RL_OK;
}

int rl_deconv_set_measurement(rl_deconv* h, const double* noisy) {
    if (!h || !noisy) return fail(RL_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->ctx->device));
    {
        std::vector<double> sums;
        RL_TRY(h->upload_images(noisy, h->meas, (size_t)h->B * h->V, nullptr, &sums));
        h->meas_level.assign((size_t)h->B, 0.0);
        for (size_t i = 0; i < sums.size(); ++i) h->meas_level[i / h->V] += sums[i];
        h->choose_loop(h->meas_level);
        RL_TRY(h->scan_meas_negative());      // (an uploaded measurement may hold negative pixels: sub())
    }
    h->meas_external = false;
    h->have_meas = true;
    h->est_ready = false;
    return RL_OK;
}

// rl_deconv_set_measurement without the upload: the caller wrote the buffer of rl_deconv_device_ptr(which = 1) on the device
// (rl_tile_gather).  The frames' levels and the negative-pixel flag are measured there before the next run (refresh_meas_levels).
int rl_deconv_measurement_written(rl_deconv* h) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    h->meas_level.clear();
    h->meas_external = true;
    h->have_meas = true;
    h->est_ready = false;
    return RL_OK;
}

int rl_deconv_set_estimate(rl_deconv* h, const double* estimate) {
    if (!h || !estimate) return fail(RL_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->ctx->device));
    RL_TRY(h->upload(estimate, h->est, (size_t)h->B * h->n_img()));
    return h->set_estimate();
}

int rl_deconv_set_acceleration(rl_deconv* h, int mode) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    if (mode != RL_ACCEL_NONE && mode != RL_ACCEL_BIGGS_ANDREWS) return fail(RL_ERR_INVALID, "unknown acceleration mode");
    if (mode == h->accel) return RL_OK;
    HIP_TRY(hipSetDevice(h->ctx->device));
    if (mode != RL_ACCEL_NONE) RL_TRY(h->ensure_accel());
    h->accel = mode;
    h->spec_valid = false;
    return h->accel_reset();
}

int rl_deconv_get_alpha(rl_deconv* h, double* out) {
    if (!h || !out) return fail(RL_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->ctx->device));
    if (!h->acc_alpha) {
        std::fill(out, out + h->B, 0.0);
        return RL_OK;
    }
    HIP_TRY(hipMemcpyAsync(out, h->acc_alpha, (size_t)h->B * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
    HIP_TRY(hipStreamSynchronize(h->ctx->stream));
    return RL_OK;
}

int rl_deconv_set_tv(rl_deconv* h, double lambda, double eps_rel) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    if (!(lambda >= 0.0 && lambda <= 0.25)) return fail(RL_ERR_INVALID, "lambda must be in [0, 0.25]");
    if (!(eps_rel > 0.0) || !std::isfinite(eps_rel)) return fail(RL_ERR_INVALID, "eps_rel must be positive and finite");
    HIP_TRY(hipSetDevice(h->ctx->device));
    if (lambda > 0.0) RL_TRY(h->ensure_tv());
    if ((lambda > 0.0) != h->tv_on()) h->spec_valid = false;
    h->tv_lambda = lambda;
    h->tv_eps_rel = eps_rel;
    return RL_OK;
}

int rl_deconv_get_tv(const rl_deconv* h, double* lambda, double* eps_rel) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    if (lambda) *lambda = h->tv_lambda;
    if (eps_rel) *eps_rel = h->tv_eps_rel;
    return RL_OK;
}

int rl_deconv_reset_estimate(rl_deconv* h) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    h->est_ready = false;
    return RL_OK;
}

// rl_deconv_iterate between its events: k iterations on the whole batch, from ones if the plan holds no estimate
static int iterate_batch(rl_deconv* h, int k) {
    bool restart = !h->est_ready;
    // H / H_t were called in between: rebuild rowFFT(est) (an accelerated or a regularised plan transforms its point inside the loop instead)
    if (!restart && !h->spec_valid && !h->sep && !h->accel && !h->tv_on()) {
        RL_TRY(h->est_spectrum(0, h->B));
        h->spec_valid = true;
    }
    return h->run_slices(k, restart);
}

static int finish_timed(rl_deconv* h) {
    HIP_TRY(hipEventRecord(h->ev1, h->ctx->stream));
    HIP_TRY(hipEventSynchronize(h->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->last_iter_ms = ms;
    return RL_OK;
}

int rl_deconv_iterate(rl_deconv* h, int k) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    if (k < 0) return fail(RL_ERR_INVALID, "k < 0");
    if (!h->have_meas) return fail(RL_ERR_STATE, "no measurement: call rl_deconv_simulate or rl_deconv_set_measurement");
    HIP_TRY(hipSetDevice(h->ctx->device));
    RL_TRY(h->refresh_meas_levels());
    HIP_TRY(hipEventRecord(h->ev0, h->ctx->stream));
    RL_TRY(iterate_batch(h, k));
    return finish_timed(h);
}

int rl_deconv_divergence(rl_deconv* h, double* out) {
    if (!h || !out) return fail(RL_ERR_INVALID, "NULL argument");
    if (!h->have_meas) return fail(RL_ERR_STATE, "no measurement: call rl_deconv_simulate or rl_deconv_set_measurement");
    if (!h->est_ready) return fail(RL_ERR_STATE, "no estimate: call rl_deconv_iterate or rl_deconv_set_estimate");
    HIP_TRY(hipSetDevice(h->ctx->device));
    RL_TRY(h->ensure_divergence());
    RL_TRY(h->divergence_partials());
    HIP_TRY(stop_totals(h->dtype, h->stop_part, h->n_frame(), h->B, h->stop_d, h->ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, h->stop_d, (size_t)h->B * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
    HIP_TRY(hipStreamSynchronize(h->ctx->stream));
    return RL_OK;
}

int rl_deconv_iterate_until(rl_deconv* h, int k_max, int check_every, int rule, double threshold, int* iterations_out,
                            double* divergence_out, int* stopped_out) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    if (k_max < 1 || check_every < 1) return fail(RL_ERR_INVALID, "k_max and check_every must be at least 1");
    if (rule != RL_STOP_DISCREPANCY && rule != RL_STOP_RELATIVE) return fail(RL_ERR_INVALID, "unknown stopping rule");
    if (threshold != threshold) return fail(RL_ERR_INVALID, "threshold is nan");
    if (!h->have_meas) return fail(RL_ERR_STATE, "no measurement: call rl_deconv_simulate or rl_deconv_set_measurement");
    HIP_TRY(hipSetDevice(h->ctx->device));
    RL_TRY(h->ensure_divergence());
    RL_TRY(h->ensure_latch());
    RL_TRY(h->refresh_meas_levels());
    hipStream_t s = h->ctx->stream;
    HIP_TRY(hipEventRecord(h->ev0, s));
    std::vector<StopFrame> state((size_t)h->B);
    for (int done = 0, check = 0; done < k_max; ++check) {
        const int c = std::min(check_every, k_max - done);
        RL_TRY(iterate_batch(h, c));   // (every lane has joined the context's stream when it returns)
        done += c;
        RL_TRY(h->divergence_partials());
        const StopFrame* prev = h->stop_state + (size_t)(check & 1) * h->B;
        StopFrame* next = h->stop_state + (size_t)((check + 1) & 1) * h->B;
        HIP_TRY(stop_latch(h->dtype, h->est, h->stop_result, h->stop_part, prev, next, h->n_img(), h->n_frame(), h->B, rule, threshold, done,
                           check > 0 ? 1 : 0, s));
        HIP_TRY(hipMemcpyAsync(state.data(), next, state.size() * sizeof(StopFrame), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        bool all = true;
        for (const StopFrame& f : state) all = all && f.stopped != 0;
        if (all) break;
    }
    // the latched estimates become the plan's estimate, as a set estimate does: a point without history
    HIP_TRY(hipMemcpyAsync(h->est, h->stop_result, (size_t)h->B * h->n_img() * dtype_size(h->dtype), hipMemcpyDeviceToDevice, s));
    RL_TRY(h->set_estimate());
    for (int f = 0; f < h->B; ++f) {
        if (iterations_out) iterations_out[f] = state[f].iterations;
        if (divergence_out) divergence_out[f] = state[f].d_latched;
        if (stopped_out) stopped_out[f] = state[f].stopped;
    }
    return finish_timed(h);
}

#define RL_GETTER(name, buf, count, need, what)                                   \
    int name(rl_deconv* h, double* out) {                                         \
        if (!h || !out) return fail(RL_ERR_INVALID, "NULL argument");             \
        if (!(need)) return fail(RL_ERR_STATE, what " is not available yet");     \
        HIP_TRY(hipSetDevice(h->ctx->device));                                    \
        return h->download(h->buf, out, (count));                                 \
    }
RL_GETTER(rl_deconv_get_object, obj, (size_t)h->B* h->n_img(), h->have_obj, "object")
int rl_deconv_get_noiseless(rl_deconv* h, double* out) {
    if (!h || !out) return fail(RL_ERR_INVALID, "NULL argument");
    if (!h->have_obj) return fail(RL_ERR_STATE, "noiseless measurement is not available yet");
    HIP_TRY(hipSetDevice(h->ctx->device));
    RL_TRY(h->expand_noiseless());   // (a shared simulation keeps one image per class and slice)
    return h->download(h->noiseless, out, (size_t)h->B * h->V * h->n_img());
}
RL_GETTER(rl_deconv_get_measurement, meas, (size_t)h->B* h->V* h->n_img(), h->have_meas, "measurement")
RL_GETTER(rl_deconv_get_estimate, est, (size_t)h->B* h->n_img(), h->est_ready, "estimate")
RL_GETTER(rl_deconv_get_normalization, norm, h->n_img(), true, "normalization")

int rl_forward(rl_deconv* h, const double* x, double* out) {
    if (!h || !x || !out) return fail(RL_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->ctx->device));
    // overwrites spec_a / spec_b; the estimate itself is kept (spec_a is rebuilt by the next iterate)
    void* xin = h->scratch;   // first B images of scratch
    RL_TRY(h->upload(x, xin, (size_t)h->B * h->n_img()));
    if (h->sep) {
        // xin lives in scratch.  Two passes: the row pass has consumed xin before the column pass writes scratch.
        // One kernel: its workgroups read halos of xin while others store -- the result goes to the (idle) spectrum buffer.
        void* res = h->sep_one ? h->sep_tmp() : h->scratch;
        RL_TRY(h->sep_forward(xin, res, h->sep_tmp(), h->B));
        return h->download(res, out, (size_t)h->B * h->V * h->n_img());
    }
    RL_TRY(h->forward_pass(xin, h->scratch, h->B, h->spec_a, h->spec_b, nullptr));
    h->spec_valid = false;
    return h->download(h->scratch, out, (size_t)h->B * h->V * h->n_img());
}

int rl_adjoint(rl_deconv* h, const double* y, double* out, int normalize) {
    if (!h || !y || !out) return fail(RL_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->ctx->device));
    RL_TRY(h->upload(y, h->scratch, (size_t)h->B * h->V * h->n_img()));
    if (h->sep && h->sep_one) {
        RL_TRY(h->sep2d_(SEP_SUM_, h->scratch, nullptr, normalize ? h->norm : nullptr, h->spec_a, h->B));
        return h->download(h->spec_a, out, (size_t)h->B * h->n_img());
    }
    if (h->sep) {
        RL_TRY(h->sep_rows_(h->scratch, h->sep_tmp(), h->B * h->V, 1));
        RL_TRY(h->sep_cols_(SEP_SUM_, h->sep_tmp(), nullptr, normalize ? h->norm : nullptr, h->spec_a, h->B));
        return h->download(h->spec_a, out, (size_t)h->B * h->n_img());
    }
    // row transform of every view image: run ROW_FWD with V folded into the frame index
    RL_TRY(h->row(ROW_FWD, (unsigned)(h->B * h->V), nullptr, h->spec_b, h->scratch, nullptr, nullptr));
    RL_TRY(h->col(h->spec_b, h->spec_b, h->B, rl_deconv::COL_HT_VIEW));
    RL_TRY(h->row(ROW_ADJ, (unsigned)h->B, h->spec_b, nullptr, nullptr, h->scratch, normalize ? h->norm : nullptr));
    h->spec_valid = false;
    return h->download(h->scratch, out, (size_t)h->B * h->n_img());
}

int rl_deconv_last_ms(const rl_deconv* h, double* iterate_ms, double* simulate_ms) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    if (iterate_ms) *iterate_ms = h->last_iter_ms;
    if (simulate_ms) *simulate_ms = h->last_sim_ms;
    return RL_OK;
}

int rl_deconv_bench_cycles(rl_deconv* h, int k, int reps, int rng_kind, uint64_t seed, double* total_ms) {
    if (!h || !total_ms) return fail(RL_ERR_INVALID, "NULL argument");
    if (!h->have_obj) return fail(RL_ERR_STATE, "rl_deconv_set_object has not been called");
    if (k < 0 || reps < 1) return fail(RL_ERR_INVALID, "bad k / reps");
    HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    h->set_measurement_from_object();   // every cycle draws its measurement from the object (before the first slice iterates: sub())
    HIP_TRY(hipEventRecord(h->ev0, s));
    for (int r = 0; r < reps; ++r) {
        // per slice of the batch: noiseless = H(obj), noisy = Poisson(noiseless) + 1e-9, est = 1,
        // k iterations -- the same values as rl_deconv_simulate + rl_deconv_iterate over the batch
        const rl_deconv::Draw draw{rng_kind, seed + (uint64_t)r, nullptr, nullptr};
        const int rc = h->run_slices(k, true, &draw, r + 1 < reps);
        if (rc != RL_OK) {
            const std::string keep = rl::last_error();
            h->join_open_lanes();
            rl::last_error() = keep;
            return rc;
        }
        h->have_meas = true;
    }
    HIP_TRY(hipEventRecord(h->ev1, s));
    HIP_TRY(hipEventSynchronize(h->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *total_ms = ms;
    return RL_OK;
}


int rl_deconv_strategy(const rl_deconv* h, int* separable, int* real_psf_spectrum, int* split_column_pass, int* frame_pairs) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    if (frame_pairs) *frame_pairs = h->pair ? 1 : 0;
    if (separable) *separable = h->sep ? (h->sep_direct ? 2 : 1) : 0;
    if (real_psf_spectrum) *real_psf_spectrum = h->psf_hat_re ? 1 : 0;
    if (split_column_pass) *split_column_pass = !h->sep && !h->pair && h->col_split() ? 1 : 0;
    return RL_OK;
}

int rl_deconv_object_classes(const rl_deconv* h, int* classes, int* shared_slices, int* slices) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    if (classes) *classes = (int)h->obj_class.size() == h->B ? h->n_classes : 0;
    if (shared_slices) *shared_slices = h->last_shared_slices;
    if (slices) *slices = h->last_slices;
    return RL_OK;
}

int rl_deconv_draws_ahead(const rl_deconv* h, int* slices) {
    if (!h || !slices) return fail(RL_ERR_INVALID, "NULL argument");
    *slices = h->last_draws_ahead;
    return RL_OK;
}

int rl_deconv_grouped_draws(const rl_deconv* h, int* slices) {
    if (!h || !slices) return fail(RL_ERR_INVALID, "NULL argument");
    *slices = h->last_grouped_draws;
    return RL_OK;
}

int rl_deconv_simulated_images(const rl_deconv* h, int* images) {
    if (!h || !images) return fail(RL_ERR_INVALID, "NULL argument");
    *images = h->last_sim_images;
    return RL_OK;
}

int rl_deconv_unresolved(rl_deconv* h, unsigned long long* count, int reset) {
    if (!h || !count) return fail(RL_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->ctx->device));
    // (the slices of a run are joined into the context's stream before a run returns: everything counted so far is ordered before this copy)
    HIP_TRY(hipMemcpyAsync(count, h->unresolved, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->ctx->stream));
    if (reset) HIP_TRY(hipMemsetAsync(h->unresolved, 0, sizeof(unsigned long long), h->ctx->stream));
    HIP_TRY(hipStreamSynchronize(h->ctx->stream));
    return RL_OK;
}

int rl_deconv_dims(const rl_deconv* h, int* batch, int* n_psf, int* ny, int* nx) {
    if (!h) return fail(RL_ERR_INVALID, "handle is NULL");
    if (batch) *batch = h->B;
    if (n_psf) *n_psf = h->V;
    if (ny) *ny = h->ny;
    if (nx) *nx = h->nx;
    return RL_OK;
}

// rl_batch_submit and rl_batch_submit_checkpoints: `ck` (its k_list ends with k_iters; out / trace are the caller's arrays, offset
// chunk by chunk here) replaces the cast of the final estimate by the checkpoints inside the slices' loops
static int batch_submit(rl_deconv* h, const rl_task* tasks, int n_tasks, int k_iters, int rng_kind, void* dev_out, int out_dtype,
                        const rl_deconv::Checkpoints* ck) {
    if (!h || (!tasks && n_tasks > 0)) return fail(RL_ERR_INVALID, "NULL argument");
    if (n_tasks < 0 || k_iters < 0) return fail(RL_ERR_INVALID, "negative count");
    if (rng_kind != RL_RNG_NONE && rng_kind != RL_RNG_PHILOX) return fail(RL_ERR_INVALID, "unknown rng_kind");
    if (dev_out && !dtype_ok(out_dtype)) return fail(RL_ERR_INVALID, "out_dtype must be RL_F32 or RL_F64");
    for (int t = 0; t < n_tasks; ++t) {
        if (!tasks[t].object) return fail(RL_ERR_INVALID, "task without an object");
        if ((uint64_t)tasks[t].image_id * (uint64_t)h->V + (uint64_t)h->V > 0xffffffffull) return fail(RL_ERR_INVALID, "image id too large");
    }
    HIP_TRY(hipSetDevice(h->ctx->device));
    RL_TRY(h->ensure_batch_slots());
    const int B = h->B;
    const size_t n = h->n_img();
    hipStream_t s = h->ctx->stream;
    std::vector<void*> ck_out;
    std::vector<double*> ck_trace;
    if (ck && ck->trace) RL_TRY(h->ensure_checkpoint_part());
    for (int t0 = 0; t0 < n_tasks; t0 += B) {
        const int nt = std::min(B, n_tasks - t0);
        rl_deconv::BatchSlot& sl = h->bslot[h->batch_chunks++ % 2];
        if (sl.used) HIP_TRY(hipEventSynchronize(sl.freed));   // the chunk before last has consumed this block
        double* tb = (double*)sl.host;
        uint64_t* seeds = (uint64_t*)(tb + B);
        uint32_t* ids = (uint32_t*)(seeds + B);
        uint32_t* idx = ids + B;
        uint32_t* lists = idx + B;   // [2][B]: ShareLists
        double* objs = (double*)(sl.host + h->slot_header_bytes());
        bool scaled = true;
        std::vector<double> level((size_t)B, 0.0);
        std::vector<const double*> uniq;
        for (int f = 0; f < B; ++f) {   // a short last chunk repeats its last task (the plan's batch is fixed)
            const rl_task& t = tasks[t0 + std::min(f, nt - 1)];
            size_t u = 0;
            while (u < uniq.size() && uniq[u] != t.object) ++u;     // (a handful of distinct objects per chunk)
            if (u == uniq.size()) {
                uniq.push_back(t.object);
                memcpy(objs + u * n, t.object, n * sizeof(double));
            }
            idx[f] = (uint32_t)u;
            tb[f] = t.total_brightness;
            scaled = scaled && t.total_brightness > 0;
            seeds[f] = t.seed;
            ids[f] = t.image_id;
        }
        // the frames' levels (what pairs frames of comparable brightness, rl_deconv::choose_loop) are known on the host: the
        // targets, or -- unscaled objects -- their sums
        if (scaled) {
            for (int f = 0; f < B; ++f) level[f] = tb[f];
        } else {
            std::vector<double> usum(uniq.size(), 0.0);
            for (size_t u = 0; u < uniq.size(); ++u)
                for (size_t i = 0; i < n; ++i) usum[u] += objs[u * n + i];
            for (int f = 0; f < B; ++f) level[f] = usum[idx[f]];
        }
        h->obj_level = level;
        h->set_measurement_from_object();   // (the chunk draws its own measurement)
        // tasks that share an object and a target are one class (object_classes.hpp); the lists of the slices' representatives ride in the header
        h->forget_classes();
        if (h->opt.share_objects && !h->sep) h->n_classes = classify_by_index(idx, scaled ? tb : nullptr, B, h->obj_class);
        const bool share = h->share_possible();
        const int cf = h->chunk_frames();
        const size_t share_total = share ? h->layout_share(cf) : 0;
        if (share) {
            std::copy(h->share_reps.begin(), h->share_reps.end(), lists);
            std::copy(h->share_rate.begin(), h->share_rate.end(), lists + B);
        }
        const size_t used = h->slot_header_bytes() + uniq.size() * n * sizeof(double);
        HIP_TRY(hipMemcpyAsync(sl.dev, sl.host, used, hipMemcpyHostToDevice, h->copy_stream));
        HIP_TRY(hipEventRecord(sl.uploaded, h->copy_stream));
        HIP_TRY(hipStreamWaitEvent(s, sl.uploaded, 0));
        const double* d_tb = (const double*)sl.dev;
        const unsigned long long* d_seeds = (const unsigned long long*)(d_tb + B);
        const unsigned* d_ids = (const unsigned*)(d_seeds + B);
        const unsigned* d_idx = d_ids + B;
        const double* d_objs = (const double*)(sl.dev + h->slot_header_bytes());
        double* d_sums = (double*)(sl.dev + (h->slot_host_bytes() + 7) / 8 * 8);
        // :505-506  obj *= total_brightness / obj.sum(), per frame, on the device
        HIP_TRY(aux_scale_convert_indexed(h->dtype, d_objs, d_idx, uniq.size(), h->obj, n, (size_t)B, scaled ? d_tb : nullptr, d_sums, s));
        if (share) {
            const rl_deconv::ShareLists staged{d_idx + B, d_idx + 2 * B};
            RL_TRY(h->place_share(cf, share_total, &staged));
        }
        h->have_obj = true;
        const rl_deconv::Draw draw{rng_kind, 0, d_seeds, d_ids};
        rl_deconv::Checkpoints cp{};
        if (ck) {   // the chunk's part of every checkpoint's destination
            cp = *ck;
            cp.nt = nt;
            if (ck->out) {
                ck_out.assign(ck->out, ck->out + ck->n_k);
                for (void*& p : ck_out)
                    if (p) p = (char*)p + (size_t)t0 * n * dtype_size(out_dtype);
                cp.out = ck_out.data();
            }
            if (ck->trace) {
                ck_trace.assign(ck->trace, ck->trace + ck->n_k);
                for (double*& p : ck_trace)
                    if (p) p += (size_t)t0 * kCheckpointFields;
                cp.trace = ck_trace.data();
            }
        }
        const int rc = h->run_slices(k_iters, true, &draw, false, ck ? &cp : nullptr);   // per slice: H(obj), keyed Poisson draws, estimate = 1, k iterations
        HIP_TRY(hipEventRecord(sl.freed, s));
        sl.used = true;
        RL_TRY(rc);
        h->have_meas = true;
        if (dev_out && !ck)
            HIP_TRY(aux_cast(h->dtype, h->est, out_dtype, (char*)dev_out + (size_t)t0 * n * dtype_size(out_dtype), (size_t)nt * n, s));
    }
    return RL_OK;
}

int rl_batch_submit(rl_deconv* h, const rl_task* tasks, int n_tasks, int k_iters, int rng_kind, void* dev_out, int out_dtype) {
    return batch_submit(h, tasks, n_tasks, k_iters, rng_kind, dev_out, out_dtype, nullptr);
}

int rl_batch_submit_checkpoints(rl_deconv* h, const rl_task* tasks, int n_tasks, const int* k_list, int n_k, int rng_kind,
                                void* const* dev_out, int out_dtype, double* const* trace_dev) {
    if (!k_list) return fail(RL_ERR_INVALID, "NULL k_list");
    if (n_k < 1 || k_list[0] < 1) return fail(RL_ERR_INVALID, "k_list must hold at least one count >= 1");
    for (int j = 1; j < n_k; ++j)
        if (k_list[j] <= k_list[j - 1]) return fail(RL_ERR_INVALID, "k_list must be strictly increasing");
    const rl_deconv::Checkpoints ck{k_list, n_k, dev_out, dev_out ? out_dtype : RL_F64, trace_dev, 0};
    // (batch_submit checks the rest; `dev_out` there only stands for "out_dtype is used")
    return batch_submit(h, tasks, n_tasks, k_list[n_k - 1], rng_kind, (void*)dev_out, out_dtype, &ck);
}

int rl_batch_run(rl_deconv* h, const rl_task* tasks, int n_tasks, int k_iters, int rng_kind, double* estimates_out) {
    if (!h || (!tasks && n_tasks > 0)) return fail(RL_ERR_INVALID, "NULL argument");
    if (n_tasks < 0 || k_iters < 0) return fail(RL_ERR_INVALID, "negative count");
    HIP_TRY(hipSetDevice(h->ctx->device));
    const size_t need = (size_t)n_tasks * h->n_img() * dtype_size(h->dtype);
    if (estimates_out && need > h->batch_out_bytes) {
        HIP_TRY(hipStreamSynchronize(h->ctx->stream));
        h->batch_out_bytes = 0;
        RL_TRY(h->release(&h->batch_out));
        RL_TRY(h->alloc(&h->batch_out, need, rl_deconv::UNCOUNTED));
        h->batch_out_bytes = need;
    }
    RL_TRY(rl_batch_submit(h, tasks, n_tasks, k_iters, rng_kind, estimates_out ? h->batch_out : nullptr, h->dtype));
    if (estimates_out && n_tasks > 0) return h->download(h->batch_out, estimates_out, (size_t)n_tasks * h->n_img());   // ONE download
    HIP_TRY(hipStreamSynchronize(h->ctx->stream));
    return RL_OK;
}

int rl_device_alloc(rl_ctx* ctx, size_t bytes, void** dev_out) {
    if (!ctx || !dev_out) return fail(RL_ERR_INVALID, "NULL argument");
    *dev_out = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMalloc(dev_out, bytes ? bytes : 1));
    return RL_OK;
}

int rl_device_free(rl_ctx* ctx, void* dev) {
    if (!ctx) return fail(RL_ERR_INVALID, "ctx is NULL");
    if (!dev) return RL_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // nothing queued may still write it
    HIP_TRY(hipFree(dev));
    return RL_OK;
}

int rl_device_upload(rl_ctx* ctx, void* dev, int dtype, size_t n_elements, const double* host) {
    if (!ctx || (n_elements && (!dev || !host))) return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(dtype)) return fail(RL_ERR_INVALID, "dtype must be RL_F32 or RL_F64");
    HIP_TRY(hipSetDevice(ctx->device));
    if (dtype == RL_F64) {
        HIP_TRY(hipMemcpyAsync(dev, host, n_elements * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return RL_OK;
    }
    const size_t piece = std::min(n_elements, (size_t)16 << 20);
    double* w = nullptr;
    RL_TRY(ctx->psf_workspace(piece, &w));
    for (size_t o = 0; o < n_elements; o += piece) {
        const size_t m = std::min(piece, n_elements - o);
        HIP_TRY(hipMemcpyAsync(w, host + o, m * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(aux_cast(RL_F64, w, RL_F32, (char*)dev + o * 4, m, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return RL_OK;
}

int rl_device_download(rl_ctx* ctx, const void* dev, int dtype, size_t n_elements, double* host_out) {
    if (!ctx || (n_elements && (!dev || !host_out))) return fail(RL_ERR_INVALID, "NULL argument");
    if (!dtype_ok(dtype)) return fail(RL_ERR_INVALID, "dtype must be RL_F32 or RL_F64");
    HIP_TRY(hipSetDevice(ctx->device));
    if (dtype == RL_F64) {
        HIP_TRY(hipMemcpyAsync(host_out, dev, n_elements * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return RL_OK;
    }
    // f32: widened on the device through the context's float64 scratch, in pieces of at most 128 MiB
    const size_t piece = std::min(n_elements, (size_t)16 << 20);
    double* w = nullptr;
    RL_TRY(ctx->psf_workspace(piece, &w));
    for (size_t o = 0; o < n_elements; o += piece) {
        const size_t m = std::min(piece, n_elements - o);
        HIP_TRY(aux_to_f64(RL_F32, (const char*)dev + o * 4, w, m, ctx->stream));
        HIP_TRY(hipMemcpyAsync(host_out + o, w, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return RL_OK;
}

int rl_deconv_device_ptr(rl_deconv* h, int which, void** ptr, size_t* n_elements, int* dtype) {
    if (!h || !ptr) return fail(RL_ERR_INVALID, "NULL argument");
    void* p = nullptr;
    size_t n = 0;
    switch (which) {
        case 0:   // (the caller may write the estimate: the sums RL-TV keeps of it are void)
            p = h->est;
            n = (size_t)h->B * h->n_img();
            h->tv_sum_valid = false;
            break;
        case 1:
            p = h->meas;
            n = (size_t)h->B * h->V * h->n_img();
            // The caller may write a measurement straight into this buffer: what the host knows about the frames' levels (the
            // pairing guard, choose_loop) is then void -- the next run recomputes them from the buffer (refresh_meas_levels).
            h->meas_level.clear();
            h->meas_external = true;
            break;
        case 2:   // (a shared simulation left one image per class: every frame's is written now)
            HIP_TRY(hipSetDevice(h->ctx->device));
            RL_TRY(h->expand_noiseless());
            p = h->noiseless;
            n = (size_t)h->B * h->V * h->n_img();
            break;
        case 3:   // (the caller may write the objects: which frames carry the same one is no longer known)
            HIP_TRY(hipSetDevice(h->ctx->device));
            RL_TRY(h->expand_noiseless());
            h->forget_classes();
            p = h->obj;
            n = (size_t)h->B * h->n_img();
            break;
        case 4:
            if (!h->tv_w) return fail(RL_ERR_STATE, "no RL-TV weights: rl_deconv_set_tv has not switched the mode on");
            p = h->tv_w;
            n = (size_t)h->B * h->n_img();
            break;
        default: return fail(RL_ERR_INVALID, "which must be 0..4");
    }
    *ptr = p;
    if (n_elements) *n_elements = n;
    if (dtype) *dtype = h->dtype;
    return RL_OK;
}

int rl_deconv_time_cycle(rl_deconv* h, int k, int rng_kind, uint64_t seed, double* avg_ms, double* launches, double* frames_per_launch) {
    if (!h || !avg_ms) return fail(RL_ERR_INVALID, "NULL argument");
    if (!h->have_obj) return fail(RL_ERR_STATE, "rl_deconv_set_object has not been called");
    if (k < 0) return fail(RL_ERR_INVALID, "k < 0");
    if (h->sep) return fail(RL_ERR_UNSUPPORTED, "per-kernel timing covers the FFT strategy; this plan runs the separable stencils");
    HIP_TRY(hipSetDevice(h->ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    h->set_measurement_from_object();
    h->timed.clear();
    h->events_used = 0;
    h->timing = true;
    const rl_deconv::Draw draw{rng_kind, seed, nullptr, nullptr};
    int rc = h->run_slices(k, true, &draw);
    h->timing = false;
    hipError_t e = hipDeviceSynchronize();
    RL_TRY(rc);
    HIP_TRY(e);
    h->have_meas = true;
    double sum[rl_deconv::TK_COUNT] = {0}, cnt[rl_deconv::TK_COUNT] = {0};
    for (const auto& t : h->timed) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, t.a, t.b));
        sum[t.kind] += ms;
        if (!t.cont) cnt[t.kind] += 1;
    }
    for (int i = 0; i < rl_deconv::TK_COUNT; ++i) {
        avg_ms[i] = cnt[i] > 0 ? sum[i] / cnt[i] : 0.0;
        if (launches) launches[i] = cnt[i];
    }
    avg_ms[7] = 0.0;   // (was the fused loop's slot; the arrays keep their 8 entries)
    if (launches) launches[7] = 0.0;
    if (frames_per_launch) *frames_per_launch = (double)h->chunk_frames();
    return RL_OK;
}

int rl_deconv_time_kernels(rl_deconv* h, int reps, double* avg_ms) {
    if (!h || !avg_ms) return fail(RL_ERR_INVALID, "NULL argument");
    if (!h->have_meas) return fail(RL_ERR_STATE, "no measurement");
    if (reps < 1) return fail(RL_ERR_INVALID, "reps < 1");
    if (h->sep) return fail(RL_ERR_UNSUPPORTED, "per-kernel timing covers the FFT strategy; this plan runs the separable stencils");
    HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    if (!h->est_ready) {
        RL_TRY(h->start_estimate_chunk(0, h->B));
        h->est_ready = true;
        h->spec_valid = true;
        h->iterations = 0;
    }
    // one untimed iteration so that every buffer holds realistic data
    RL_TRY(h->iterate_chunk({0, h->B, false, false, false}));
    ++h->iterations;
    // the RL kernels are timed on the launch shape the RL loop uses: one slice of the batch, and through the loop's own four passes
    const rl_deconv::Iter it{0, h->chunk_frames(), false, false, false};
    avg_ms[6] = (double)it.nf;
    for (int which = 0; which < 6; ++which) {
        HIP_TRY(hipEventRecord(h->ev0, s));
        for (int r = 0; r < reps; ++r) {
            switch (which) {
                case 0: RL_TRY(h->pass_h(it)); break;
                case 1: RL_TRY(h->pass_ratio(it)); break;
                case 2: RL_TRY(h->pass_ht(it)); break;
                case 3: RL_TRY(h->pass_update(it)); break;
                case 4: RL_TRY(h->row(ROW_FWD, (unsigned)h->B, nullptr, h->spec_a, h->obj, nullptr, nullptr)); break;
                case 5: HIP_TRY(aux_poisson(h->dtype, h->noiseless, h->meas, (unsigned)h->n_img(), (unsigned)(h->B * h->V), 0, 1, RL_RNG_PHILOX, h->scratch, s)); break;
            }
        }
        HIP_TRY(hipEventRecord(h->ev1, s));
        HIP_TRY(hipEventSynchronize(h->ev1));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
        avg_ms[which] = (double)ms / reps;
    }
    // the repeated launches trashed the RL state on purpose; force a clean restart
    h->est_ready = false;
    h->spec_valid = false;
    h->tv_sum_valid = false;
    return RL_OK;
}

}  // extern "C"

