/* rlsted.h -- C ABI of librlsted.so: MI355X (gfx950) implementation of the
 * rescan line-STED image-formation + Richardson-Lucy hot path.
 *
 * The reference (AndrewGYork/rescan_line_sted) has no FFI or plugin interface
 * for this path: its boundary is the Python module namespace
 * figure_generation/line_sted_tools.py.  Each entry point below states which
 * reference function (file:line) it stands in for; the Python mirror of that
 * module (rescan_line_sted_amd/line_sted_tools.py) binds them with ctypes (see
 * INTEGRATION.md).
 *
 * Conventions: every function returns 0 on success and a negative code on
 * failure, after which rl_last_error() describes the failure (thread local).
 * No exceptions cross the boundary.  Host buffers are caller owned, row major,
 * C contiguous.  Handles are opaque.  One call in flight per context.
 *
 * All image-like host arrays are float64 (the reference's dtype); the
 * arithmetic type on the device is chosen per plan (RL_F32 / RL_F64).  The
 * one exception is the acquired-stack path (rl_stack_run): raw camera frames
 * go in and estimates come out in the types its parameters name.
 */
#ifndef RLSTED_H
#define RLSTED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RL_OK 0
#define RL_ERR_INVALID -1     /* bad argument */
#define RL_ERR_HIP -2         /* HIP runtime error (no device, launch failure, OOM...) */
#define RL_ERR_UNSUPPORTED -3 /* size / mode not built */
#define RL_ERR_STATE -4       /* call sequence error (e.g. iterate before data) */

#define RL_F32 0
#define RL_F64 1

/* Poisson generator selection for rl_deconv_simulate */
#define RL_RNG_NONE 0      /* noisy = noiseless + 1e-9 (no noise)                       */
#define RL_RNG_PHILOX 1    /* device Philox4x32-10 counter RNG, bit-exact vs oracle twin */

typedef struct rl_ctx rl_ctx;
typedef struct rl_deconv rl_deconv;
typedef struct rl_comm rl_comm;

const char* rl_last_error(void);
int rl_version(void);
int rl_device_count(int* count);

/* Page-locked host memory for the buffers handed to the calls below: the float64 arrays of the reference's
 * call surface (line_sted_tools.py:496-531: obj, noisy_measurement, estimate are host numpy arrays) then cross
 * PCIe by direct DMA instead of through the runtime's pageable-copy staging.
 * Purely optional: every entry point accepts ordinary host pointers.                                        */
int rl_host_alloc(size_t bytes, void** out);
int rl_host_free(void* p);

/* One context per GPU: owns the stream and the per-length twiddle tables. */
int rl_ctx_create(int device, rl_ctx** out);
int rl_ctx_destroy(rl_ctx* ctx);
int rl_ctx_synchronize(rl_ctx* ctx);

/* The host calls that cut their work into chunks keep the workspace of one chunk under a cap in bytes, held by the context.  The
 * RESULTS DO NOT DEPEND ON THE CAP: every item's arithmetic is a function of the item alone, in a fixed order, and what a call
 * carries from one chunk to the next (rl_fig3_scan's running sum) makes the same additions in the same order.  At least one item
 * runs per chunk, whatever the cap.  which, and the default:
 *   RL_CHUNK_REGISTER_SUMS  rl_register_sums, rl_affine_sums, the sums of rl_register_estimate: the partials of the pairs in
 *                           flight; 256 MiB
 *   RL_CHUNK_SHIFT          rl_shift_images, the refine passes' shifts of rl_register_estimate: the float64 intermediates of the
 *                           images in flight; 512 MiB
 *   RL_CHUNK_XCORR          rl_register_xcorr: the spectra, kept rows and windows of the pairs in flight; 32 MiB
 *   RL_CHUNK_RING           rl_ring_stats, rl_ring_sector_stats: the two spectra of the pairs in flight, and the sector results of
 *                           the pairs in flight; 256 MiB
 *   RL_CHUNK_FIG3           rl_fig3_scan: one float64 image stack of the positions in flight (the call holds three); 512 MiB
 *   RL_CHUNK_WARP           rl_warp_images (the cap of rl_warp_chunk_bytes); 512 MiB
 *   RL_CHUNK_BEADS          rl_find_peaks (the cap of rl_find_peaks_chunk_bytes); 256 MiB
 * rl_chunk_bytes sets the cap of `which` for the later calls on this context.  RL_ERR_INVALID, the cap unchanged: a NULL ctx, a
 * `which` that is none of the above, 0 bytes.
 * rl_chunks_run: the trips the chunk loop under that cap made in the most recent call on this context that has such a loop; 0
 * before any such call, and for a NULL ctx or an unknown `which`.  A host counter: nothing on the device knows of it.
 * rl_register_estimate counts its first sums stage under RL_CHUNK_REGISTER_SUMS and the shift launches of its last refine pass
 * under RL_CHUNK_SHIFT (left as it was when no pass shifts anything). */
enum {
    RL_CHUNK_REGISTER_SUMS = 0,
    RL_CHUNK_SHIFT = 1,
    RL_CHUNK_XCORR = 2,
    RL_CHUNK_RING = 3,
    RL_CHUNK_FIG3 = 4,
    RL_CHUNK_WARP = 5,
    RL_CHUNK_BEADS = 6,
    RL_CHUNK_COUNT = 7
};
int rl_chunk_bytes(rl_ctx* ctx, int which, size_t bytes);
int rl_chunks_run(rl_ctx* ctx, int which);

/* Smallest supported transform length >= n (0 if none). */
int rl_fft_length_for(int n);

/* ---- Deconvolver: line_sted_tools.py:478-594 -------------------------------
 * A plan holds `batch` independent frames that share one PSF set (`n_psf`
 * views of shape (1, py, px)) and one image shape (ny, nx).  Replaces
 * Deconvolver.__init__ (:479-494) plus the lazily cached H_t normalisation
 * (:589-592), which is computed here once.                                   */
int rl_deconv_create(rl_ctx* ctx, const double* psfs, int n_psf, int py, int px,
                     int batch, int ny, int nx, int dtype, rl_deconv** out);
/* rl_deconv_create with the plan's switches as an argument.  options: NULL, or a NUL-terminated text of NAME=value entries
 * separated by whitespace; the names are the RLSTED_* environment variables' own, e.g.
 * "RLSTED_PAIR=0 RLSTED_LANES=1".  A switch is taken from options; one that options does not name from the environment; one that
 * neither names has its default.  rl_deconv_create(...) is rl_deconv_create_with(..., NULL, out).
 * RL_ERR_INVALID, with the offender named in rl_last_error and no plan created: an entry without '=', with an empty name or an
 * empty value, a name given twice, and a name that is no switch of a plan (a misspelt one, or the process-wide
 * RLSTED_DEBUG_SYNC).  Variables of the environment that are no switch stay ignored.                                          */
int rl_deconv_create_with(rl_ctx* ctx, const double* psfs, int n_psf, int py, int px,
                          int batch, int ny, int nx, int dtype, const char* options, rl_deconv** out);
int rl_deconv_destroy(rl_deconv* h);

/* Geometry chosen by the plan: ly, lx transform lengths, pitch of spectra. */
int rl_deconv_info(const rl_deconv* h, int* ly, int* lx, int* pitch, size_t* device_bytes);

/* create_data_from_object (:496-512), first half: copy obj [batch][ny][nx],
 * scale each frame so that its sum is total_brightness[f] (NULL: no scaling),
 * noiseless = H(obj).                                                        */
int rl_deconv_set_object(rl_deconv* h, const double* obj, const double* total_brightness);
/* create_data_from_object (:508-511), second half: noisy = Poisson(noiseless)
 * + 1e-9 drawn on the device.  Counter layout: see DESIGN.md "Device Poisson". */
int rl_deconv_simulate(rl_deconv* h, int rng_kind, uint64_t seed);

/* As rl_deconv_simulate, with a Philox key per frame: frame f (all its views v) draws with seed
 * seeds[f] and image index image_ids[f] * n_psf + v (host arrays of n_frames entries).  A frame's
 * noise then depends on (seed, image id, pixel) only -- not on the batch it is simulated in, which
 * is what lets a parameter sweep pack tasks with different seeds into one plan.  With seeds[f] = s
 * and image_ids[f] = f this is rl_deconv_simulate(h, rng_kind, s).                              */
int rl_deconv_simulate_keyed(rl_deconv* h, int rng_kind, const uint64_t* seeds, const uint32_t* image_ids);
/* Inject a measurement [batch][n_psf][ny][nx] instead (load_data_from_tif
 * :514-518, or noise drawn on the host with numpy for figure reproduction).
 * New data (this call, rl_deconv_simulate, rl_deconv_simulate_keyed) starts a new Richardson-Lucy run: the
 * next rl_deconv_iterate begins from ones and rl_deconv_get_estimate fails (RL_ERR_STATE) until then.  The
 * reference keeps its estimate across create_data_from_object (:496-531, it only resets at num_iterations
 * == 0); a caller that wants that reads the estimate before the new data and hands it back with
 * rl_deconv_set_estimate afterwards -- the Deconvolver mirror does (line_sted_tools.py).                 */
int rl_deconv_set_measurement(rl_deconv* h, const double* noisy);

/* iterate (:520-531) K times; the first call starts from estimate = 1.       */
int rl_deconv_iterate(rl_deconv* h, int k);
int rl_deconv_reset_estimate(rl_deconv* h);
/* Deconvolver.estimate is a plain attribute in the reference (:522,530): assigning to it, or replacing
 * the measurement after some iterations (create_data_from_object called again, :496-512), continues
 * from that estimate.  Uploads estimate [batch][ny][nx]; the next rl_deconv_iterate continues from it. */
int rl_deconv_set_estimate(rl_deconv* h, const double* estimate);

/* Biggs-Andrews accelerated Richardson-Lucy (Biggs & Andrews, Appl. Opt. 36, 1766, 1997), per plan, off by default.  Opt in:
 * it departs from the reference's iteration by design.  With psi(y) one reference iteration
 * (:520-531) applied to y, x_0 = ones, per frame and k = 0, 1, ...:
 *     x_{k+1} = psi(y_k)                                                y_0 = x_0
 *     g_k     = x_{k+1} - y_k
 *     a_{k+1} = clamp(sum g_k g_{k-1} / sum g_{k-1} g_{k-1}, 0, 1)      (0 for k = 0, or a denominator that is 0 / not finite)
 *     y_{k+1} = max(x_{k+1} + a_{k+1} (x_{k+1} - x_k), 0)
 * Sums over the frame's ny * nx pixels, accumulated in float64 in a fixed order (no atomics): a frame's result in a float64 plan
 * does not depend on its batch.  The estimate after K iterations is x_K.  The history (x_k, y_k, g_k, the partial sums) spans
 * rl_deconv_iterate calls -- iterate(3) then iterate(2) is iterate(5) -- and restarts with new data (rl_deconv_set_measurement,
 * rl_deconv_simulate*, every chunk of rl_batch_run / rl_batch_submit), rl_deconv_reset_estimate, rl_deconv_set_estimate (a set
 * estimate is an x_k without history: the next step has a = 0) and a change of mode; rl_forward / rl_adjoint leave it alone.
 * The mode applies from the next iterate / batch run on; switching it on allocates three more images per frame.
 * At very low dose the extrapolation reaches the noise-fitting regime in fewer iterations, as plain Richardson-Lucy does later. */
#define RL_ACCEL_NONE 0
#define RL_ACCEL_BIGGS_ANDREWS 1
int rl_deconv_set_acceleration(rl_deconv* h, int mode);
/* out [batch]: the a that formed each frame's last extrapolated point (0 before one). */
int rl_deconv_get_alpha(rl_deconv* h, double* out);

/* Total-variation regularised Richardson-Lucy (RL-TV; Dey et al., Microsc. Res. Tech. 69, 260, 2006), per plan, off by default.
 * Opt in: it departs from the reference's iteration by design.  At low dose plain Richardson-Lucy fits
 * the noise once it runs long enough; the multiplicative TV step keeps the estimate piecewise smooth.  Per frame, with psi the
 * plan's own iteration applied to the point at hand x (the estimate, or the extrapolated y_k when the Biggs-Andrews mode is on: its
 * psi is then this regularised step), n = ny * nx, all arithmetic in the plan's element type T unless stated, contraction off, IEEE
 * sqrt and /:
 *     s      = (sum x) / n                     float64 sum in the fixed order of csrc/accel_kernels.hpp (thread, tree, workgroups);
 *                                              1 exactly for the start from ones
 *     eps2   = T((eps_rel s) (eps_rel s))      formed in float64, rounded once to T
 *     dx[i,j]= x[i,j+1] - x[i,j]  (0 in the last column)       dy[i,j] = x[i+1,j] - x[i,j]  (0 in the last row)
 *     m      = sqrt((dx dx + dy dy) + eps2)    px = dx / m     py = dy / m
 *     div    = ((px[i,j] - px[i,j-1]) + (py[i,j] - py[i-1,j]))   (the subtracted term is 0 in column 0 / row 0)
 *     w      = 1 / (1 - lambda div)
 *     x_new  = psi(x) w
 * Every pixel has |div| <= 2 + sqrt(2): px^2 + py^2 <= 1 and each of the two backward neighbours' components has magnitude <= 1.
 * Accepted: 0 <= lambda <= 0.25 and eps_rel > 0 finite -- the denominator is then >= 0.146 with no clamp; anything else is
 * RL_ERR_INVALID.  lambda == 0 switches the mode off: the plan then runs the plain path bit for bit.  The mode applies from the
 * next iterate / batch run / iterate_until on, on every plan type and both element types; switching it on allocates one more image
 * per frame and the sums' partials (counted in device_bytes).  iterate(a) then iterate(b) is iterate(a + b) bit for bit; a frame's
 * result in a float64 plan does not depend on its batch; rl_forward / rl_adjoint / rl_deconv_divergence in between change nothing.
 * CONDITIONING: the step is an explicit TV flow.  It amplifies differences in x -- rounding differences between two builds or
 * element types included -- unless lambda max(x) / (eps_rel mean(x)) is well below 1/4: lambda = 0.01, eps_rel = 0.1 on natural
 * images is stable (a 1e-7 relative perturbation per iteration moves the K = 200 result by 5e-7, less than it moves plain
 * Richardson-Lucy); lambda >= 0.03, eps_rel <= 0.03, or sparse emitters on black are not (1e-2 .. 1e-1), and the result is then
 * reproducible only on one build and element type.  rl_deconv_get_tv: the values in force (lambda 0: off);
 * either pointer may be NULL. */
int rl_deconv_set_tv(rl_deconv* h, double lambda, double eps_rel);
int rl_deconv_get_tv(const rl_deconv* h, double* lambda, double* eps_rel);

/* How well the current estimate explains the data: the Poisson I-divergence D(m || p) = sum m log(m / p) - m + p of every frame,
 * out [batch], with m the stored measurement and p = H(estimate) -- the quantity Richardson-Lucy minimises.  Computed on the
 * device: p is what rl_forward returns for the current estimate (the same launches, reading the estimate where it is), nothing
 * but the batch's doubles crosses PCIe.  Per frame over the N = n_psf * ny * nx stored values of its views, each converted to
 * float64 before any arithmetic, a pixel's term is
 *     p > 0          :  ((m > 0 ? m * log(m / p) : 0) - m) + p          (log: the float64 device log)
 *     p <= 0 or nan  :  m > 0 ? 0 : -m     a prediction the plan could not resolve is a neutral pixel, as in the iteration's ratio
 *                                          (rl_deconv_unresolved: ratio 1 means m = p, whose term is 0)
 * summed in float64 in a fixed order (no atomics): the frame's values are vectors of 16 bytes dealt to workgroups of 256 threads
 * in equal runs (the split depends on N and the element type alone); a thread adds its terms in increasing order, a workgroup
 * its threads' sums in a binary tree, the frame its workgroups' sums in increasing order (csrc/stop_kernels.hpp).  A frame's D in
 * a float64 plan does not depend on its batch.  Needs a measurement and an estimate (RL_ERR_STATE otherwise).  Leaves the
 * estimate, the measurement and the Biggs-Andrews history alone: iterate(a), divergence, iterate(b) gives the estimate of
 * iterate(a), forward(x), iterate(b) bit for bit.  Works on every plan type; its buffers (the partial sums) are allocated on
 * first use and counted in device_bytes.  Synchronises the plan's stream. */
int rl_deconv_divergence(rl_deconv* h, double* out);

/* Richardson-Lucy with a stopping rule per frame.  DEFINED as this sequence of the calls above, and equal to it bit for bit:
 * starting like rl_deconv_iterate (from ones if the plan holds no estimate), repeat { c = min(check_every, k_max - done)
 * iterations on the whole batch; D of every frame as rl_deconv_divergence forms it; the rule } until every frame has stopped
 * or done == k_max.  With N = n_psf * ny * nx and the threshold t, evaluated in float64 exactly as written:
 *     RL_STOP_DISCREPANCY :  2 * D / N <= t                 (t = 1: the discrepancy principle for Poisson data; Bertero et al.,
 *                                                            Inverse Problems 26, 105004, 2010)
 *     RL_STOP_RELATIVE    :  a previous check of this call exists and D_prev - D <= t * D_prev    (also stops a D that rose)
 * A D -- or a D_prev -- that is nan or infinite never meets a rule.  A frame stops at the first check that meets the rule: its
 * estimate, D and iteration count (counted from the start of this call) of that check are kept on the device; a frame that never
 * stops ends with those of the last check and stopped == 0.  All frames keep iterating until the loop ends (a frame pair's
 * partner does not change under it); stopping only freezes what is reported.  After each check the host reads the batch's
 * stopped flags (one small copy) to end early.  At the end the kept estimates become the plan's estimate (rl_deconv_get_estimate,
 * rl_deconv_device_ptr which = 0), as after rl_deconv_set_estimate: a following rl_deconv_iterate continues from them and the
 * Biggs-Andrews history restarts.  iterations_out, divergence_out, stopped_out: [batch] each, any may be NULL.  k_max < 1,
 * check_every < 1, an unknown rule or a nan threshold: RL_ERR_INVALID; no measurement: RL_ERR_STATE.  rl_deconv_last_ms covers
 * the whole call.  The first call allocates one more image per frame and the frames' state (counted in device_bytes).
 * At fewer than about one photon per pixel the expectation of 2 D / N at the true object falls below 1: the discrepancy rule at
 * t = 1 then stops at the first check -- the threshold is the caller's to choose.
 * Not covered: rl_batch_run / rl_batch_submit take a fixed iteration count (enqueued work, no host in the loop). */
#define RL_STOP_DISCREPANCY 1
#define RL_STOP_RELATIVE 2
int rl_deconv_iterate_until(rl_deconv* h, int k_max, int check_every, int rule, double threshold, int* iterations_out,
                            double* divergence_out, int* stopped_out);

int rl_deconv_get_object(rl_deconv* h, double* out);        /* [batch][ny][nx]        */
int rl_deconv_get_noiseless(rl_deconv* h, double* out);     /* [batch][n_psf][ny][nx] */
int rl_deconv_get_measurement(rl_deconv* h, double* out);   /* [batch][n_psf][ny][nx] */
int rl_deconv_get_estimate(rl_deconv* h, double* out);      /* [batch][ny][nx]        */
int rl_deconv_get_normalization(rl_deconv* h, double* out); /* [ny][nx]               */

/* H (:567-577): x [batch][ny][nx] -> out [batch][n_psf][ny][nx].             */
int rl_forward(rl_deconv* h, const double* x, double* out);
/* H_t (:579-594): y [batch][n_psf][ny][nx] -> out [batch][ny][nx].           */
int rl_adjoint(rl_deconv* h, const double* y, double* out, int normalize);

/* Device time (hipEvents on the plan's stream) of the last rl_deconv_iterate /
 * rl_deconv_set_object+simulate call, in milliseconds.                       */
int rl_deconv_last_ms(const rl_deconv* h, double* iterate_ms, double* simulate_ms);

/* Benchmark entry: run `reps` x (simulate + k iterations) on device-resident
 * data with no host transfers inside the timed region; returns total device ms
 * measured with hipEvents on the plan's stream.                              */
int rl_deconv_bench_cycles(rl_deconv* h, int k, int reps, int rng_kind, uint64_t seed, double* total_ms);

/* Device address of a plan buffer for zero-copy hand-off (e.g. the RCCL gather
 * of final estimates): which = 0 estimate [batch][ny][nx], 1 measurement, 2
 * noiseless [batch][n_psf][ny][nx], 3 object, 4 the RL-TV weights w [batch][ny][nx] of the
 * last regularised step (RL_ERR_STATE before rl_deconv_set_tv switched the mode on).  The buffer stays owned by the
 * plan; *dtype = RL_F32 / RL_F64 element type.  Synchronise the context first.
 * The allocation extends 16 KiB past n_elements (zeroed slack that the row kernels' unconditional 64-lane
 * loads may read and discard): never write there, never assume the next buffer starts right behind. */
int rl_deconv_device_ptr(rl_deconv* h, int which, void** ptr, size_t* n_elements, int* dtype);

/* The caller has written a complete new measurement, all batch * n_psf images, into the buffer of rl_deconv_device_ptr(which = 1)
 * on the device (rl_tile_gather, rl_device_upload, a kernel of its own on the context's stream).  Leaves the plan exactly where
 * rl_deconv_set_measurement leaves it, without the upload: it holds a measurement -- also a plan that never saw
 * rl_deconv_set_measurement or rl_deconv_simulate, which otherwise answers rl_deconv_iterate with RL_ERR_STATE -- and the next
 * Richardson-Lucy run starts from ones.  The frames' levels (the pairing guard of rl_deconv_strategy) and the negative-pixel flag
 * are measured on the device before that run. */
int rl_deconv_measurement_written(rl_deconv* h);

/* Convolution strategy the plan chose for its PSF set: separable == 1: every view
 * is rank 1 (p = u v^T; the 0 / 90 degree line PSFs) and small, H / H_t run as direct row + column stencils;
 * separable == 2: the views are small but not rank 1 and H / H_t run as a direct 2-D stencil (py * px multiply-adds
 * per pixel; RLSTED_DIRECT) -- like the separable form it keeps the relative accuracy of a dark region's prediction;
 * otherwise the FFT path, with real_psf_spectrum != 0 when the (point-symmetric) PSFs' spectra are real and
 * the column kernels multiply by their real parts alone; split_column_pass != 0: a multi-view f32 plan on the long
 * column transforms (L = 2304, 4608), whose column passes are two launches each -- forward half, inverse half, the
 * column spectra parked between them (this slot reported the removed fused kernel of round 2 and was always 0);
 * frame_pairs != 0: the Richardson-Lucy loop transforms frames 2p and 2p+1 as the real and imaginary part of one
 * complex image (single-view f32 plans by default: RLSTED_PAIR) -- a frame's estimate then depends on its partner
 * at f32 rounding level (~1e-7 of the brighter partner's scale).  The answer is the loop that will run on the
 * CURRENT data: a plan built with pairs runs its per-frame loop while any pair's frames differ in level (sum of the
 * object / measurement) by more than a factor of 4 (RLSTED_PAIR_MAX_RATIO), because a dim frame would inherit
 * the rounding error of a bright partner.  Any of the pointers may be NULL.                                  */
int rl_deconv_strategy(const rl_deconv* h, int* separable, int* real_psf_spectrum, int* split_column_pass, int* frame_pairs);

/* Frames that carry the same object are simulated once per cycle.  Two frames are of one class when their
 * float64 input images (rl_deconv_set_object: compared with up to 8 earlier frames; rl_batch_run / rl_batch_submit: the tasks'
 * object pointers) and their brightness targets are the same: their scaled objects are then the same bits on the device, and so
 * is H(object).  A slice of the batch SHARES when the distinct classes within it are at most half its frames.  A simulate +
 * deconvolve cycle (rl_deconv_bench_cycles, rl_batch_run, rl_batch_submit; FFT path) computes H once for each class that its
 * sharing slices hold, before the first slice, and every frame's Poisson draw in such a slice
 * reads its class's rates with the frame's own Philox counters: measurements and estimates are bit for bit those of the
 * per-frame simulation (RLSTED_SHARE_OBJECTS=0).  The noiseless buffer is written in full before it is handed out
 * (rl_deconv_get_noiseless, rl_deconv_device_ptr which = 2); handing out the object buffer (which = 3) ends the sharing until
 * the next object is set.  *classes: classes of the object as last set (0: not known); *shared_slices of *slices: slices of the
 * last cycle that shared.  Any of the pointers may be NULL.                                        */
int rl_deconv_object_classes(const rl_deconv* h, int* classes, int* shared_slices, int* slices);

/* Images H(object) was computed for in the last simulate + deconvolve cycle (rl_deconv_bench_cycles, rl_deconv_time_cycle, the last
 * chunk of rl_batch_run / rl_batch_submit): n_psf per object class that the cycle's sharing slices hold -- a class is simulated once
 * per cycle, however many slices draw from it -- plus n_psf per frame of the slices that do not share.  0 before the first cycle. */
int rl_deconv_simulated_images(const rl_deconv* h, int* images);

/* Slices of the last simulate + deconvolve cycle whose Poisson draw ran ahead of their lane.  A slice that shares its
 * simulation (rl_deconv_object_classes) draws from the class rates alone, so its draw need not wait for its lane.  With
 * RLSTED_DRAW_AHEAD=1 in the environment when the plan is created (default 0: every slice draws at the head of its lane), a plan
 * of several lanes enqueues such a draw on the context's stream, a narrow launch (RLSTED_DRAW_GRID workgroups, default 128) that
 * runs beside the loop of the slice in front on the same lane, at most one slice per lane ahead.  Slices that do not share, the
 * first slice of every lane in a cycle that follows nothing, a lane that holds a single slice, and plans of one lane draw in
 * their lane all the same.  The values do not depend on where or how widely a draw runs -- measurements and estimates are the
 * same bits either way -- and the lanes wait for every draw: the measurement is complete when the call that ran the cycle
 * returns, as it always was.  Measured, the schedule gains at most 1 % and loses 10 - 25 % where the context's stream shares a
 * hardware queue with a lane ("Draws ahead").  0 before the first cycle and whenever the switch is off.   */
int rl_deconv_draws_ahead(const rl_deconv* h, int* slices);

/* Slices of the last simulate + deconvolve cycle whose Poisson draw ran through the frame-group kernel.  The frames of a slice
 * that shares its simulation (rl_deconv_object_classes) draw from few rate images; with the Philox generator such a slice is
 * drawn in groups of 8 frames of one rate image (where the launch has as many) per tile of 256 pixels, and what the sampler
 * derives from the rate alone -- a square root, divisions, two logarithms -- is evaluated once per pixel and run of frames
 * with one rate image instead of once per frame.  Every draw keeps its frame's own key and image id: measurements and estimates are the same bits either way.
 * RLSTED_POISSON_GROUPS=0 in the environment when the plan is created draws every slice through the per-frame kernel.  Slices
 * that do not share and draws with RL_RNG_NONE take the per-frame kernel always.  0 before the first cycle.                    */
int rl_deconv_grouped_draws(const rl_deconv* h, int* slices);

/* Predictions the plan could not resolve.  iterate divides the measurement by H(estimate) clamped at 0 (line_sted_tools.py:575,
 * 524); in exact arithmetic that prediction is positive, but a transform resolves a value to eps * the frame's maximum only, so
 * on sparse emitters over a black background the predictions of the dark region are rounding noise of either sign -- below 1e-7
 * of the maximum for an f32 plan, 1e-16 for a float64 plan (and for the reference, which then divides by zero: inf, nan, the
 * frame lost).  The kernels treat a pixel whose prediction is not positive as neutral (ratio 1) and count it: *count = the lanes
 * of the FFT path's ratio launches that met such a pixel inside the image since the plan was created or the counter last reset
 * (reset != 0 clears it).  0 on data the plan's arithmetic resolves; an f32 plan that counts should be a float64 plan -- its
 * estimates stay finite and non-negative but are no longer within 1e-5 of the float64 result.  The count is a sufficient sign, not
 * a necessary one: rounding noise that happens to be positive everywhere is not counted (a frame of isolated photons, well below
 * one per pixel, can pass with 0).  Synchronises the plan's stream.                                                              */
int rl_deconv_unresolved(rl_deconv* h, unsigned long long* count, int reset);

/* Plan geometry: frames per plan, views per frame, image shape.                */
int rl_deconv_dims(const rl_deconv* h, int* batch, int* n_psf, int* ny, int* nx);

/* ---- parameter sweeps: line_sted_figure_2.py:39-57 ---------------------------
 * The reference's figure script builds one Deconvolver per (PSF set, test image) and runs
 * create_data_from_object + N x iterate on each.  A task is one such simulation for a plan's PSF
 * set and image shape: an object [ny][nx] (host, float64), its total brightness (:505-506; <= 0:
 * no scaling -- then for every task of the call), and the Philox key (seed, image_id) of its noise
 * (rl_deconv_simulate_keyed).  rl_batch_run works through n_tasks tasks in chunks of the plan's
 * batch: objects -> H -> Poisson -> k_iters Richardson-Lucy iterations from estimate = 1, and
 * writes the estimates [n_tasks][ny][nx] to estimates_out (NULL: the last chunk stays in the
 * plan's buffers for rl_gather).  A task's noiseless and noisy measurements do not depend on its position in the
 * list (per-task Philox key); its estimate does not either in f64 plans, and in f32 plans only at rounding level
 * (~1e-7: frame pairs share a transform with their neighbour in the batch -- and only with a neighbour of
 * comparable level, see rl_deconv_strategy).                                                                  */
typedef struct rl_task {
    const double* object;
    double total_brightness;
    uint64_t seed;
    uint32_t image_id;
} rl_task;
int rl_batch_run(rl_deconv* h, const rl_task* tasks, int n_tasks, int k_iters, int rng_kind, double* estimates_out);

/* The same work, ENQUEUED: returns once the tasks' objects are staged (page-locked buffers of the plan, two chunks deep) and
 * every copy and kernel is in the context's stream order -- chunk i + 1 is uploaded on a copy stream while chunk i iterates, and
 * successive calls, on this plan or on other plans of the context, follow each other on the device without the host in
 * between.  The estimates go to DEVICE memory: dev_out [n_tasks][ny][nx] of out_dtype (RL_F32 / RL_F64; rl_device_alloc, or
 * any device pointer of this GPU), NULL: nowhere (the last chunk stays in the plan's buffers).  Nothing of the result may be
 * read, and the plan not destroyed, before rl_ctx_synchronize.  rl_batch_run is this call with a buffer of its own followed by
 * ONE download.  line_sted_figure_2.py:39-57 is a loop of such runs: one per (PSF set, test image).                       */
int rl_batch_submit(rl_deconv* h, const rl_task* tasks, int n_tasks, int k_iters, int rng_kind, void* dev_out, int out_dtype);

/* ---- iteration checkpoints: line_sted_figure_2.py's record_iteration at the save points of logarithmic_progress ------------
 * Richardson-Lucy on Poisson data is semi-convergent: the answer of a sweep is a curve over the iteration count.  This is
 * rl_batch_submit with k_iters = k_list[n_k - 1] -- the same enqueued cycle per task: staging, class sharing, keyed Poisson
 * draws, slices, lanes, every loop, Biggs-Andrews and RL-TV as they are -- that takes the estimate out at every count of
 * k_list (host array, strictly increasing, k_list[0] >= 1) and scores it there.  Nothing is decided on the device: the launch
 * sequence is known on the host when the call is made.
 *   dev_out    NULL, or a host array of n_k device pointers, each NULL or [n_tasks][ny][nx] of out_dtype: checkpoint j of task t is
 *              the estimate after k_list[j] iterations, written where rl_batch_submit with k_list[j] would have written its
 *              result -- and bit for bit what it would have written, for the same tasks on the same plan, on every plan type, both
 *              element types and both opt-in modes (iterate(a) then iterate(b) is iterate(a + b))
 *   trace_dev  NULL, or a host array of n_k device pointers, each NULL or float64 [n_tasks][RL_TRACE_FIELDS]: six sums over the
 *              image's ny * nx pixels, x the estimate at that checkpoint, T the task's scaled object as the plan's object buffer
 *              holds it (the plan's element type), every value widened to float64 before any arithmetic, no contraction:
 *                  0 sum x    1 sum T    2 sum x*x    3 sum T*T    4 sum x*T    5 sum (x-T)*(x-T)
 *              Field 5 is formed per pixel from the difference, not from fields 2 to 4.  The sums run in the fixed order of
 *              csrc/accel_kernels.hpp -- thread in increasing order, binary tree over 256 threads, workgroups in increasing order;
 *              the split is decided by ny * nx and the element type alone; no floating-point atomics -- so a trace is bit-identical
 *              from run to run and a function of the task's estimate and object only.
 * Both pointer arrays are read during the call only.  A checkpoint is taken inside the slice's loop on the lane's stream, behind
 * the iteration that completes k_list[j] (and the accelerated step's reduction); no lane join is added between checkpoints, and
 * the frame-pair loop drops its last spectrum at the last iteration of the run only.  A short last chunk writes its real tasks
 * only.  The plan's state after the call is that of rl_batch_submit with the last count.  The per-workgroup partials are the
 * plan's, allocated on the first call with a trace and counted in rl_deconv_info's device_bytes.
 * RL_ERR_INVALID: NULL handle, NULL tasks with n_tasks > 0, negative n_tasks, NULL k_list, n_k < 1, k_list[0] < 1, a list that
 * is not strictly increasing, an unknown rng_kind, a dev_out with a bad out_dtype, a task without an object, an image id that is
 * too large.                                                                                                                 */
#define RL_TRACE_FIELDS 6
int rl_batch_submit_checkpoints(rl_deconv* h, const rl_task* tasks, int n_tasks, const int* k_list, int n_k, int rng_kind,
                                void* const* dev_out, int out_dtype, double* const* trace_dev);

/* Device memory owned by the caller: the result buffer of a sweep (rl_batch_submit), the operands of rl_comm_gather_device.
 * rl_device_download: n elements of `dtype` -> host float64 (blocking; synchronises the context first).                   */
int rl_device_alloc(rl_ctx* ctx, size_t bytes, void** dev_out);
int rl_device_free(rl_ctx* ctx, void* dev);
int rl_device_download(rl_ctx* ctx, const void* dev, int dtype, size_t n_elements, double* host_out);
/* host float64 -> n elements of `dtype` at a device address of this GPU (a caller's buffer, or a plan buffer handed out by
 * rl_deconv_device_ptr -- the zero-copy way to replace a measurement: the plan re-measures its frames' levels before the next run). */
int rl_device_upload(rl_ctx* ctx, void* dev, int dtype, size_t n_elements, const double* host);
/* Stream-ordered device-to-device copy of `bytes` bytes on the context's stream (it does not wait): what moves a chunk's estimates
 * from a plan buffer into a caller's store.  The ranges must not overlap (RL_ERR_INVALID). */
int rl_device_copy(rl_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);

/* ---- multi-GPU: one process per GPU, frames sharded over ranks -----------------
 * The reference is single process; independent simulations shard with no
 * data-path collective and ONE gather of the results at the end (section 8e).  RCCL over xGMI,
 * loaded on first use.  rl_comm_unique_id on one rank produces RL_COMM_ID_BYTES bytes that every
 * rank passes to rl_comm_create (a collective call: all ranks of the world enter it together).   */
#define RL_COMM_ID_BYTES 128
int rl_comm_unique_id(void* id128);
int rl_comm_create(rl_ctx* ctx, int rank, int world, const void* id128, rl_comm** out);
int rl_comm_destroy(rl_comm* c);
int rl_comm_info(const rl_comm* c, int* rank, int* world);
/* device-synchronise this rank, then meet every other rank (the timing harness' barrier) */
int rl_comm_barrier(rl_comm* c);
/* *value = max over ranks of *value (every rank gets the result)                       */
int rl_comm_allreduce_max(rl_comm* c, double* value);
/* Gather the first counts[r] frames of every rank r's plan buffer `which` (as in
 * rl_deconv_device_ptr) on `root`, rank-major, straight from the device buffers: every rank sends
 * to the root, the root receives on all its links at once.  rl_gather delivers float64 on the
 * root's host (host_out: sum(counts) frames; ignored on other ranks); rl_gather_device leaves the
 * result in a device buffer owned by the communicator (root: *dev_out, valid until the next
 * rl_gather / rl_gather_device of this communicator -- rl_comm_gather_host stages through a buffer of its own and
 * leaves it alone; other ranks: NULL) in the plan's dtype.                                 */
/* The sweep's one gather: counts[r] elements of `dtype` from every rank r's DEVICE buffer dev_local, rank-major
 * into dev_out on the root (device memory of the root's GPU holding sum(counts) elements; ignored elsewhere) -- results of
 * different shapes travel unpadded, in the plan's own arithmetic type.  Synchronises the device on both sides of the transfer. */
int rl_comm_gather_device(rl_comm* c, const void* dev_local, const size_t* counts, int dtype, int root, void* dev_out);
/* n float64 values from `root`'s host buffer into every rank's (the PSF sets of a sweep are built once -- the reference builds
 * them once per figure, line_sted_figure_2.py:66-72 -- and sent to the other ranks).  Collective.                          */
int rl_comm_bcast_host(rl_comm* c, double* buf, size_t n, int root);
int rl_gather(rl_comm* c, rl_deconv* plan, int which, int root, const int* counts, double* host_out);
int rl_gather_device(rl_comm* c, rl_deconv* plan, int which, int root, const int* counts, void** dev_out,
                     size_t* n_elements, int* dtype);
/* The same for host arrays (results that no longer live in a plan, e.g. a sweep's stack of frames
 * of several shapes): counts[r] float64 values of rank r's `local`, rank-major into `out` on root. */
int rl_comm_gather_host(rl_comm* c, const double* local, const size_t* counts, int root, double* out);

/* ---- PSF generation: line_sted_tools.py:75-363, 653-668 ---------------------
 * get_width (:653-668): MINPACK-lmdif fit of A*exp(-(x-mu)^2/(2 sigma^2)) to
 * y[0..n-1] from [1, n/2, 1] with scipy.optimize.curve_fit's defaults; host
 * code, needs no GPU.  p3 = {A, mu, sigma}; *info = MINPACK info (may be NULL). */
int rl_gauss_fit(const double* y, int n, double* p3, int* info);

/* scipy.ndimage.gaussian_filter as the reference uses it (:185-213,260,280):
 * float64, mode 'reflect', radius int(truncate*sigma+0.5), axes with sigma <=
 * 1e-15 skipped.  in/out: host [nz][ny][nx].                                   */
int rl_gaussian_filter(rl_ctx* ctx, const double* in, double* out, int nz, int ny, int nx,
                       const double* sigma3, double truncate);

/* generate_psfs (:168-363) for shape (1, ny, nx).  psf_type 0 = 'point', 1 =
 * 'line'.  rescan_ratio > 0 forces the integer line rescan ratio, <= 0 derives
 * it from the fitted width of the central sted row (:252-256).
 * arrays_out: NULL or [5 (point) | 7 (line)][ny][nx] = excitation, depletion,
 *   excitation_fraction, depletion_fraction, sted, descan_sted, rescan_sted.
 * rows_out:   NULL or [3][nx] central rows of excitation, sted, rescan_sted.
 * scalars_out[10]: 0 ratio used, 1 ideal ratio, 2-4 area sums of excitation /
 *   depletion / sted, 5-7 central-row sums of the same, 8 = 1 when every
 *   central-row maximum equals its array maximum (asserts :105-106,120).      */
int rl_psf_generate(rl_ctx* ctx, int psf_type, int ny, int nx, double excitation_brightness,
                    double depletion_brightness, double blur_sigma, int rescan_ratio,
                    double* arrays_out, double* rows_out, double* scalars_out);

/* The two intermediate arrays of the 'line' branch that generate_psfs(output_dir=...) also writes (:339-341):
 * emission_psf_out [ny][nx] = gaussian_filter(centred delta, blur_sigma) (:258-260) and rescan_unscaled_out
 * [ny][rescan_ratio * nx] = rescanned_signal_cumu, the detector ring before it is rolled and binned (:266-298).
 * rescan_ratio: the integer ratio a previous rl_psf_generate of the same parameters reported (scalars_out[0]); it
 * sizes the second buffer.  Either pointer may be NULL.                                                      */
int rl_psf_generate_line_extras(rl_ctx* ctx, int ny, int nx, double excitation_brightness, double depletion_brightness,
                                double blur_sigma, int rescan_ratio, double* emission_psf_out, double* rescan_unscaled_out);

/* psf_report (:75-166).  report_out[8] = { resolution_improvement_descanned,
 * resolution_improvement_rescanned (NaN for 'point'), excitation_dose,
 * depletion_dose, expected_emission, num_steps n, line rescan ratio, invariant
 * flag as scalars_out[8] above }.  arrays_out as in rl_psf_generate with ny = nx
 * = n = 1 + 2*round(5*sigma) (NULL: scalars only).                             */
int rl_psf_report(rl_ctx* ctx, int psf_type, double excitation_brightness, double depletion_brightness,
                  double steps_per_excitation_psf_width, double pulses_per_position,
                  double* arrays_out, double* report_out);

/* psf_report for n_sets parameter sets in one call (the sweeps of line_sted_figure_1.py:33-48 and
 * line_sted_figure_a1.py:29,64,102,172): one launch per pipeline stage over all sets, the Gaussian fits of
 * all sets on the host in between.  params[n_sets][5] = { psf_type (0 / 1), excitation_brightness,
 * depletion_brightness, steps_per_excitation_psf_width, pulses_per_position }; report_out[n_sets][8] as
 * rl_psf_report, bit for bit; arrays_out: NULL, or n_sets pointers, each NULL or [5 | 7][n][n].        */
int rl_psf_report_batch(rl_ctx* ctx, int n_sets, const double* params, double* report_out, double* const* arrays_out);

/* rotate of line_sted_figure_2.py:264-272 for one [ny][nx] plane (general angles; the
 * caller keeps the script's exact 0 and 90 degree special cases): cubic B-spline
 * rotation about the centre as scipy.ndimage.rotate(order=3, reshape=False), then
 * clipped to [0, 1.1 * max(in)].  Host in / out, float64.                       */
int rl_rotate_psf(rl_ctx* ctx, const double* in, double* out, int ny, int nx, double degrees);
/* The same for a stack [nz][ny][nx] in one call: every plane rotated in its plane, all of them clipped to
 * [0, 1.1 * max(in)] with the maximum of the WHOLE array, as the script's np.clip does (fig2:271).      */
int rl_rotate_psf_stack(rl_ctx* ctx, const double* in, double* out, int nz, int ny, int nx, double degrees);

/* ---- reconstruction quality (line_sted_tools.py:539-547, line_sted_figure_2.py:353-390) ----
 * out[i] = f(|fftshift(fft2(x[i]))| * scale) for n_img real images [n_img][ny][nx] of any
 * size, f(m) = log(1 + m) when log1p != 0, else m.  record_iteration's FT-error history is
 * (x = estimate_k - truth, scale 1, log1p 1); fourier_error of the figure-2 harness
 * (:353-355) is (x = estimate - truth, scale 1/(ny*nx), log1p 0).                      */
int rl_fft2_magnitude(rl_ctx* ctx, const double* x, int n_img, int ny, int nx, double scale, int log1p,
                      double* out);

/* scipy.ndimage.map_coordinates(image, [ys, xs]) with its defaults (order 3, mode 'constant',
 * cval 0, prefilter) for a [ny][nx] image at n points (:381-384): out[n].               */
int rl_spline_sample(rl_ctx* ctx, const double* image, int ny, int nx, const double* ys, const double* xs, int n,
                     double* out);

/* ---- ring statistics: per-ring sums over the 2-D spectra of device-resident image pairs ----
 * What the figure-2 sweep is scored with (the ring RMS of fourier_error, line_sted_figure_2.py:353-355) and the Fourier ring
 * correlation of two noise realisations, without downloading an image.
 *
 * For a pair of real images a, b [ny][nx] and a real scale s: A = fft2(a), B = fft2(s * b), unnormalised DFTs on the exact image
 * grid (numpy.fft.fft2), every value widened to float64 before any arithmetic.
 * Signed frequency of bin (ky, kx): sy = ky <= ny / 2 ? ky : ky - ny, sx likewise.  RING of the bin, in exact integer arithmetic,
 * with q = (sy * nx)^2 + (sx * ny)^2, M = ny * nx, R = n_rings:
 *     ring = isqrt(4 * R^2 * q) / M          (integer division) = floor(2 R * radius / (0.5 cycles per pixel))
 * Bins whose ring is >= R (the corners) belong to no ring.  The default R = rl_ring_count(ny, nx) = min(ny, nx) / 2; for an even
 * square image that ring is floor(sqrt(sy^2 + sx^2)).  (A float formula does not reproduce this: at 160 x 160 float64 moves the eight
 * bins (+-33, +-56), (+-56, +-33), whose radius is exactly 65, one ring down.)  The table is built on the host, once per (ny, nx, n_rings) and context.
 * out[pair][ring][RL_RING_FIELDS], summed over ALL ny * nx bins of the ring:
 *     0  number of bins      1  sum |A|^2      2  sum |B|^2      3  sum Re(A conj(B))      4  sum |A - B|^2
 * in a fixed order (ring_kernels.hpp), no floating-point atomics: bit-identical from run to run, and a pair's result does not
 * depend on the other pairs of the call.
 *
 * a_dev / b_dev: device buffers of this GPU (an rl_device_alloc buffer such as a sweep's results, a plan buffer from
 * rl_deconv_device_ptr) of dtype a_dtype / b_dtype (RL_F32 / RL_F64, they may differ); image i of the pair starts at ELEMENT
 * offset a_offsets[i] / b_offsets[i] (host arrays [n_pairs]; any offset >= 0, no alignment assumed).  a_dev and b_dev may be the
 * same buffer, and many pairs may name the same image.  b_scale: host [n_pairs], or NULL for 1.
 * Pairs are processed in chunks whose working memory stays under a cap (rl_chunk_bytes); the ring table and the workspace are kept in the
 * context and freed with it.  Synchronises the context's stream.
 * RL_ERR_INVALID: a NULL pointer, n_pairs < 1, ny or nx < 2, n_rings < 1, a dtype that is neither, a negative offset;
 * RL_ERR_UNSUPPORTED: ny or nx > 4096 (the transform is the O(n^3) matrix form), n_rings > 16384.                        */
#define RL_RING_FIELDS 5
int rl_ring_count(int ny, int nx);
int rl_ring_stats(rl_ctx* ctx, const void* a_dev, int a_dtype, const int64_t* a_offsets, const void* b_dev, int b_dtype,
                  const int64_t* b_offsets, const double* b_scale, int n_pairs, int ny, int nx, int n_rings, double* out);

/* ---- angle-resolved ring statistics: the rings of rl_ring_stats cut into n_sectors = S orientation sectors ----
 * What separates a 2-line scan from a 3-line scan from a point PSF: the error and the ring correlation along one direction.
 * Bin (ky, kx) has the signed frequencies sy, sx of rl_ring_stats; with the integers Y = sy * nx, X = sx * ny (the two that form
 * q) its ring is unchanged.
 * ORIENTATION: theta = atan2(Y, X) folded into [0, pi): (Y, X) is replaced by (-Y, -X) when Y < 0 or (Y = 0 and X < 0).  theta is
 * measured from +kx towards +ky in physical cycles per pixel (the angle_degrees of error_vs_spatial_frequency); a bin and its
 * Hermitian partner -k have the same theta.
 * SECTOR of the bin:  sector = floor(S * theta / pi + 1/2) mod S.  Sector j is centred on j * 180 / S degrees and half-open,
 * [centre - 90 / S, centre + 90 / S) degrees; S = 2 * num_angles puts the figure's best angle in the middle of sector 0 and its
 * worst angle in the middle of sector 1.  The DC bin has no orientation and belongs to sector 0.
 * EXACTNESS: a bin lies exactly on a boundary only when that boundary is a multiple of 45 degrees (the tangent of any other
 * boundary angle is irrational): for odd S the boundary at 90 degrees (bins with X = 0), for S = 2 mod 4 those at 45 and 135
 * degrees (bins with |Y| = |X|).  These ties are decided in integers (Y = 0, X = 0, |Y| = |X|) and by the half-open rule go to
 * the upper sector.  Everywhere else the host builder uses long double, and if a bin that is no tie comes closer to a boundary
 * than 2^-30 (in units of S * theta / pi) the call fails with RL_ERR_UNSUPPORTED rather than guessing.  The device never
 * computes an angle.  The table is built on the host, once per (ny, nx, n_rings, n_sectors) and context.
 * out[pair][ring][sector][RL_RING_FIELDS]: the five fields of rl_ring_stats summed over the bins of the cell (ring, sector), in
 * a fixed order (ring_kernels.hpp), bit-identical from run to run and independent of the other pairs of the call.  An empty
 * cell is five zeros, never nan.  Because -k shares k's cell, every cell's sums are those of a real image pair, like a ring's.
 * Every other rule is that of rl_ring_stats: offsets, dtypes, b_scale, chunking under the workspace cap (the result chunk is S
 * times as large), the 4096 limit, the error codes; and RL_ERR_INVALID: n_sectors < 1;  RL_ERR_UNSUPPORTED: n_sectors > 64.   */
int rl_ring_sector_stats(rl_ctx* ctx, const void* a_dev, int a_dtype, const int64_t* a_offsets, const void* b_dev, int b_dtype,
                         const int64_t* b_offsets, const double* b_scale, int n_pairs, int ny, int nx, int n_rings,
                         int n_sectors, double* out);

/* ---- ensemble statistics: per-pixel mean, variance, squared bias and mean squared error over groups of images ----
 * What the noise realisations of one (object, PSF set) operating point of a sweep say together, without downloading an image:
 * the error of the ensemble split into what the blur leaves (bias^2) and what the noise adds (variance).
 * Group g is the n = group_ptr[g + 1] - group_ptr[g] images of n_pixels contiguous values of src_dtype (RL_F32 / RL_F64) at the
 * ELEMENT offsets member_offsets[group_ptr[g] .. group_ptr[g + 1]) of src_dev (host arrays; any offset >= 0, no alignment
 * assumed; groups may differ in size and an image may be listed in many groups; no cap on n).  truth_dev: NULL, or a device
 * buffer of truth_dtype whose n_pixels values at element offset truth_offsets[g], times truth_scale[g] (NULL: 1), are the
 * group's true image s t.  Per pixel, every value widened to float64 before any arithmetic, no contraction, the members
 * x_0 ... x_{n-1} in list order:
 *     mean = ((((0 + x_0) + x_1) + ...) + x_{n-1}) / n
 *     ss   = sum_m (x_m - mean)^2                      a second pass over the members, same order
 *     var  = n > 1 ? ss / (n - 1) : 0
 *     bias = mean - s t,  b2 = bias * bias
 *     mse  = (sum_m (x_m - s t)^2) / n                 (= b2 + (n - 1) / n var, up to rounding)
 * Without a truth b2 = mse = 0.
 * mean_dev, var_dev: device float64 [n_groups][n_pixels], either may be NULL; neither may overlap the member images.
 * out: host [n_groups][RL_ENSEMBLE_FIELDS], sums over the group's pixels:
 *     0  n      1  sum mean      2  sum var      3  sum b2      4  sum mse      5  sum (s t)^2
 * in a fixed order (ensemble_kernels.hpp) that n_pixels and src_dtype alone decide, no floating-point atomics: bit-identical
 * from run to run, and a group's numbers do not depend on the other groups of the call.
 * The tables and the partial sums live in a workspace kept in the context and freed with it.  Synchronises the context's stream.
 * RL_ERR_INVALID: a NULL ctx / src_dev / member_offsets / group_ptr / out, n_groups < 1, group_ptr[0] < 0, an empty or
 * decreasing group_ptr range, n_pixels < 1, a dtype that is neither, a negative offset, truth_dev without truth_offsets, a map
 * that overlaps the member images.                                                                                          */
#define RL_ENSEMBLE_FIELDS 6
int rl_ensemble_stats(rl_ctx* ctx, const void* src_dev, int src_dtype, const int64_t* member_offsets, const int32_t* group_ptr,
                      int n_groups, const void* truth_dev, int truth_dtype, const int64_t* truth_offsets,
                      const double* truth_scale, size_t n_pixels, double* mean_dev, double* var_dev, double* out);

/* ---- tiled Richardson-Lucy: images of any size as overlapping tiles of an ordinary plan ----
 * An image axis of n pixels is cut into tiles of `tile` pixels that overlap by at least `overlap`; every tile is deconvolved as a
 * frame of a plan of the tile's shape, zero-extended at its border exactly as an image is at its own, and the estimates are
 * blended with weights that are 0 in a margin of `margin` pixels at every interior tile edge and ramp linearly to 1 across the
 * rest of the overlap.  Plain Richardson-Lucy from ones moves information 2 * (max(py, px) / 2) pixels
 * per iteration, so with margin >= 2 * k * (max(py, px) / 2) the blend of k-iteration tile estimates IS the whole-image estimate
 * up to rounding; smaller margins trade accuracy for speed.  Biggs-Andrews and RL-TV use per-frame sums: they run per tile.
 *
 * rl_tile_axis (host only): 0 < overlap < tile.  n <= tile: one tile of n pixels at 0.  Otherwise s = tile - overlap,
 * *count = ceil((n - tile) / s) + 1 tiles of `tile` pixels at origins[i] = (i * (n - tile)) / (*count - 1) (integer division):
 * the first at 0, the last at n - tile, none overhangs.  origins: *count values, or NULL to ask for the count alone.
 * rl_tile_weights (host only): 0 <= margin, 2 * margin < overlap; origins as rl_tile_axis gave them (any non-decreasing list from
 * 0 to n - t whose neighbours overlap by more than 2 * margin is accepted; t = min(tile, n)).  Raw weight of tile i at local j:
 *     min(1, left, right),   left  = clamp((j - margin + 0.5) / R, 0, 1),       R  = origins[i-1] + t - origins[i] - 2 margin   (i > 0)
 *                            right = clamp((t - margin - j - 0.5) / R', 0, 1),  R' = origins[i] + t - origins[i+1] - 2 margin   (i < count-1)
 * weights_out [count][t]: the raw weight over the sum of the raw weights of all tiles covering that pixel (summed in increasing i;
 * positive everywhere, or RL_ERR_INVALID) -- per pixel the weights sum to 1.  first_out, count_out [n] (both or neither): first
 * covering tile and number of covering tiles of every pixel; more than two tiles may cover one.  Any output may be NULL. */
int rl_tile_axis(int n, int tile, int overlap, int* count, int* origins);
int rl_tile_weights(int n, int tile, int overlap, int margin, int count, const int* origins, double* weights_out, int* first_out,
                    int* count_out);
/* rl_tile_gather: windows of src_dev [F][V][NY][NX] (src_dtype) -> dst_dev [n_slots][V][ty][tx] (dst_dtype), a plan's measurement
 * buffer (rl_deconv_device_ptr which = 1 of a plan of n_slots frames of ty x tx; then rl_deconv_measurement_written).  slots: host,
 * n_slots triples (frame, a_y, a_x), the window's frame and origin; frame = -1: a filler, written with ones, so that a short last
 * chunk never iterates on stale data.  A plain copy, one rounding at most (f64 -> f32).  Enqueued on the context's stream; writes
 * exactly n_slots * V * ty * tx values (never the slack behind a plan buffer).
 * RL_ERR_INVALID: a NULL argument, a dtype that is neither, F / V / NY / NX / n_slots < 1, a tile larger than the image, a frame
 * outside -1 .. F - 1, a window that overhangs the image, dst overlapping src.
 * rl_tile_blend: tiles_dev [F][ny_tiles][nx_tiles][ty][tx] (tiles_dtype; tiles frame-major, then tile row, then tile column) ->
 * out_dev [F][NY][NX] (out_dtype):
 *     out[f][gy][gx] = sum_iy sum_ix (wy[iy][gy - origins_y[iy]] * wx[ix][gx - origins_x[ix]]) * tile value
 * over the covering tiles, in float64, from 0.0, iy ascending outside, ix ascending inside, each term (wy * wx) * (double)e, no
 * contraction, no atomics: a float64 output is bit-identical from run to run, an f32 output is that value rounded once.
 * origins_y / origins_x, wy [ny_tiles][ty] / wx [nx_tiles][tx]: host arrays (rl_tile_axis, rl_tile_weights); the coverage tables
 * are computed in the call and staged with them in a workspace kept in the context.  Synchronises the context's stream.
 * RL_ERR_INVALID: a NULL argument, a dtype that is neither, a count < 1, a tile larger than the image, an origin outside
 * 0 .. N - t or decreasing, a pixel no tile covers, out overlapping the tiles. */
int rl_tile_gather(rl_ctx* ctx, const void* src_dev, int src_dtype, int F, int V, int NY, int NX, const int* slots, int n_slots,
                   int ty, int tx, void* dst_dev, int dst_dtype);
int rl_tile_blend(rl_ctx* ctx, const void* tiles_dev, int tiles_dtype, int F, int NY, int NX, int ny_tiles, int nx_tiles, int ty,
                  int tx, const int* origins_y, const int* origins_x, const double* wy, const double* wx, void* out_dev, int out_dtype);

/* ---- acquired camera stacks: narrow ingest, narrow export, overlapped transfers ----
 * load_data_from_tif (:514-518) hands a measured stack to the Deconvolver; cameras deliver uint16.  These calls move raw frames
 * across PCIe in their own type and turn them into a plan's measurement on the device.
 *
 * rl_ingest: raw_dev holds src_images sensor frames of src_ny rows of src_pitch elements of raw_dtype (RL_RAW_*).  dst_dev
 * [n_slots][V][ny][nx] of dst_dtype (RL_F32 / RL_F64) is a plan's measurement buffer (rl_deconv_device_ptr which = 1; then
 * rl_deconv_measurement_written) or any device buffer of that size.  Slot b, view v is the window of ny x nx pixels at (y0, x0) of
 * source image b * frame_stride + v * view_stride ([F][V] order: V, 1; the [V][F] order that record_data writes: 1, F).  Slots >=
 * n_valid are fillers, written with ones (a short last chunk).  Per pixel, in float64, no contraction:
 *     x = (double)raw;   d = dark_dev ? (double)dark_dev[y][x] : offset      (dark_dev: device float [ny][nx], window coordinates)
 *     v = (x - d) * gain                                                     (two roundings)
 *     saturated += saturation > 0 && x >= saturation
 *     v not finite: invalid += 1, v = 0;     otherwise v < 0: clipped += 1, v = 0
 *     out = (dst type)(v + epsilon)                                          (1e-9 mirrors load_data_from_tif)
 * stats_dev: NULL, or device float64 [n_slots * V][RL_INGEST_FIELDS]: the sum of the stored values (widened to float64; a filler's
 * is ny * nx), then the clipped, saturated and invalid counts.  The sum runs in the fixed order of csrc/ingest_kernels.hpp --
 * thread, binary tree over 256 threads, workgroups in increasing order; the split is decided by ny and nx alone; no atomics -- and
 * is bit-identical from run to run; the counts are exact.  Reads nothing outside the windows, writes exactly n_slots * V * ny * nx
 * values (never the slack behind a plan buffer).  Enqueued on the context's stream.
 * rl_export: est_dev [n][ny][nx] of est_dtype (RL_F32 / RL_F64) -> out_dev of out_dtype (RL_OUT_*): y = (double)e * scale; f32 /
 * f64: y rounded once; u16: rint(y), ties to even, nan and y <= 0 give 0, y > 65535 gives 65535 and is counted.  stats_dev: NULL,
 * or device float64 [n][RL_EXPORT_FIELDS]: the sum of (double)e in the same fixed order, the clamped count.  Enqueued.
 * RL_ERR_INVALID (no kernel is launched): a NULL ctx / source / destination, an unknown dtype, a count < 1 (n_valid: outside 0 ..
 * n_slots), a window that overhangs the sensor frame, a source image outside 0 .. src_images - 1 for a valid slot, gain not finite
 * or <= 0, offset, scale or saturation nan, epsilon < 0 or not finite, a destination that overlaps a source. */
#define RL_RAW_U8 0
#define RL_RAW_U16 1
#define RL_RAW_I16 2
#define RL_RAW_F32 3
#define RL_OUT_F32 0
#define RL_OUT_F64 1
#define RL_OUT_U16 2
#define RL_ORDER_FRAME_VIEW 0
#define RL_ORDER_VIEW_FRAME 1
#define RL_INGEST_FIELDS 4
#define RL_EXPORT_FIELDS 2
int rl_ingest(rl_ctx* ctx, const void* raw_dev, int raw_dtype, int src_images, int src_ny, int src_pitch, int y0, int x0,
              long long frame_stride, long long view_stride, int n_slots, int n_valid, int V, int ny, int nx,
              const float* dark_dev, double offset, double gain, double epsilon, double saturation,
              void* dst_dev, int dst_dtype, double* stats_dev);
int rl_export(rl_ctx* ctx, const void* est_dev, int est_dtype, int n, int ny, int nx, double scale,
              void* out_dev, int out_dtype, double* stats_dev);

/* A stack pipeline on a plan: any number of frames through the plan's batch B, chunk by chunk, with the transfers overlapped.
 * params: the sensor frame (src_ny rows of src_pitch elements, src_nx <= src_pitch of them pixels), the window origin (y0, x0) of the
 * plan's ny x nx image in it, the camera (offset or a host dark map [ny][nx], gain, epsilon, saturation), the order of raw_host --
 * RL_ORDER_FRAME_VIEW [n_frames][V] images, RL_ORDER_VIEW_FRAME [V][n_frames] -- and the output (out_dtype, out_scale).
 * rl_stack_run: raw_host -> out_host [n_frames][ny][nx] of out_dtype after k_iters Richardson-Lucy iterations from ones per frame,
 * in the plan's current modes (Biggs-Andrews, RL-TV).  Two slots, each a page-locked raw block, a device raw buffer, a device out
 * buffer and a page-locked out block; a copy-in and a copy-out stream beside the context's.  Chunk i + 1 is uploaded before chunk i
 * iterates; the context's stream runs rl_ingest, rl_deconv_measurement_written, rl_deconv_reset_estimate, rl_deconv_iterate and
 * rl_export; chunk i is downloaded while chunk i + 1 iterates.  Page-locked raw_host / out_host (rl_host_alloc) are copied to and
 * from directly, pageable ones through the slots' blocks.  A short last chunk is filled with ones frames.  ingest_stats
 * [n_frames][V][RL_INGEST_FIELDS], export_stats [n_frames][RL_EXPORT_FIELDS], times_ms [4] = wall time of the call, summed event
 * times of the uploads, of the compute stream's work, of the downloads: host arrays, any may be NULL.  The first failure ends the
 * run; the call then waits for the copies still in flight before it returns, so the caller may let go of its arrays.  An array is
 * copied directly only if its first and its last byte are page-locked.  The plan is left as after rl_deconv_iterate on the last
 * chunk; it must outlive the stack.  rl_stack_destroy synchronises the three streams. */
typedef struct rl_stack rl_stack;
typedef struct rl_stack_params {
    int raw_dtype, order, src_ny, src_nx, src_pitch, y0, x0;
    double offset, gain, epsilon, saturation;
    const float* dark;   /* host [ny][nx], or NULL: offset */
    int out_dtype;
    double out_scale;
} rl_stack_params;
int rl_stack_create(rl_deconv* plan, const rl_stack_params* params, rl_stack** out);
int rl_stack_run(rl_stack* st, const void* raw_host, int n_frames, int k_iters, void* out_host, double* ingest_stats,
                 double* export_stats, double* times_ms);
int rl_stack_destroy(rl_stack* st);
/* rl_stack_run_registered: rl_stack_run with every image registered on the device before the iterations (registration.py
 * deconvolve_stack_registered(pipeline=True)).  Per chunk, on the context's stream: the upload waited
 * for, rl_ingest into a staging buffer [B][V][ny][nx] of the plan's dtype (its statistics into the slot as rl_stack_run does),
 * `freed` recorded; chunk 0 only: frame 0's V images copied to the references and, with rp->views and V > 1, views 1 .. V - 1
 * estimated against view 0 (rl_register_estimate); with rp->frames every (f, v) of the chunk but global frame 0 estimated against
 * reference v, the view shift added (fillers: shift 0); rl_shift_images staging -> the plan's measurement buffer, all B V images,
 * order rp->interp, floor = epsilon; the plan's iterations from ones; rl_export into the slot.  Uploads of chunk i + 1 and
 * downloads of chunk i - 1 run on the copy streams as in rl_stack_run.  The estimates are those of the host's loop in
 * deconvolve_stack_registered, bit for bit.  rp: the switches, max_shift 1 .. 32 (margin max_shift + 2), refine >= 0, interp 1 or 3
 * (the search values are checked only when something is estimated).  given_shifts: NULL, or host [n_frames][V][2] applied as they
 * are (no estimate).  register_out: host arrays, all required -- shifts [n_frames][V][2] as applied, fields [n_frames][V][3] = ncc,
 * at_limit, flat of the frame estimates (0 where none ran), view_shifts [V][2], view_fields [V][3], raised [n_frames][V] (pixels
 * raised to epsilon by the shift).  times_ms: NULL or [5] = rl_stack_run's four, then the summed wall time of the estimates.  The
 * staging buffer, the references and (refine > 0) a float64 scratch of B V images are allocated on first use and freed by
 * rl_stack_destroy.  On failure the copies in flight are waited for before it returns.
 * RL_ERR_INVALID (nothing is enqueued): a NULL st / raw_host / rp / out_host / register_out or one of its arrays, n_frames < 1,
 * k_iters < 0, interp neither 1 nor 3, a given shift that is not finite; estimating: max_shift outside 1 .. 32, refine < 0, an
 * interior ny - 2 (max_shift + 2) or nx - 2 (max_shift + 2) below 8. */
typedef struct {
    int views, frames;       /* nonzero: estimate the views on frame 0 / every frame against frame 0 */
    int max_shift, refine;
    int interp;              /* 1 or 3 */
} rl_stack_register;
typedef struct {
    double *shifts, *fields, *view_shifts, *view_fields, *raised;
} rl_stack_register_out;
int rl_stack_run_registered(rl_stack* st, const void* raw_host, int n_frames, int k_iters, const rl_stack_register* rp,
                            const double* given_shifts, void* out_host, double* ingest_stats, double* export_stats,
                            rl_stack_register_out* register_out, double* times_ms);
/* `bytes` bytes of any type from a host array to a device address of this GPU, as they are (raw camera data on its way to
 * rl_ingest outside a pipeline: deconvolve_tiled with a camera).  Blocking: the host array may go away when it returns. */
int rl_device_upload_bytes(rl_ctx* ctx, void* dev, const void* host, size_t bytes);

/* ---- registration of views and frames: translation estimates and sub-pixel shifts on the device ----
 * SIGN CONVENTION: the shift of an image is the displacement d of its content relative to the reference, B[y + d] ~ A[y].  The peak
 * of the correlation surface of rl_register_sums is at d, and rl_shift_images with that d undoes it.
 *
 * rl_register_sums: correlation sums of n_pairs image pairs over a window of integer displacements.  ref_dev / mov_dev: device
 * buffers of dtype ref_dtype / mov_dtype (RL_F32 / RL_F64, they may differ); pair i is the reference image A at ELEMENT offset
 * ref_offsets[i] and the moving image B at mov_offsets[i], both [ny][nx] (host arrays [n_pairs]; any offset >= 0, no alignment
 * assumed; many pairs may share one reference; the buffers may be the same).  R: search radius, 1 .. 32.  M: margin, M >= R, with
 * ny - 2 M >= 8 and nx - 2 M >= 8.  With the interior I = [M, ny - M) x [M, nx - M), for every d = (dy, dx) in [-R, R]^2:
 *     S_b(d) = sum_I B[y+dy][x+dx]      S_bb(d) = sum_I B[y+dy][x+dx]^2      S_ab(d) = sum_I A[y][x] B[y+dy][x+dx]
 * sums_out: host [n_pairs][(2 R + 1)^2][RL_REGISTER_FIELDS] = S_b, S_bb, S_ab at index (dy + R) (2 R + 1) + dx + R;  ref_out: host
 * [n_pairs][2] = S_a = sum_I A, S_aa = sum_I A^2.  Every sum has (ny - 2 M)(nx - 2 M) terms.
 * ARITHMETIC: every value is widened exactly to float64; a product enters its sum through one fused multiply-add.  With
 * W = 2 R + 1, nd = W^2, TY = 16 for R <= 16 and 8 above, G = 1 for nd >= 256 and otherwise the largest power of two with G <= TY
 * and G nd <= 256, h = TY / G: the interior's rows are cut into strips of h rows from y = M on, ceil((ny - 2 M) / TY) G of them (the
 * last may be short or empty), its columns into blocks of 32 from x = M on.  A strip's sum for one d starts at 0.0 and takes the
 * column blocks in increasing order, inside a block the strip's rows in increasing order, inside a row the columns in increasing
 * order, per pixel S_b = S_b + b; S_bb = fma(b, b, S_bb); S_ab = fma(a, b, S_ab).  A pair's sum is (((0.0 + strip_0) + strip_1) +
 * ...) over the strips in increasing order.  S_a and S_aa: per image row from 0.0 over the interior's columns in increasing order
 * (S_a + a; fma(a, a, S_aa)), then (((0.0 + row_M) + row_{M+1}) + ...), followed by + 0.0 for the rows that complete the last TY.
 * No floating-point atomics: bit-identical from run to run, and a pair's result does not depend on the other pairs of the call.
 * Nothing outside an image is read.  Pairs are processed in chunks whose partial sums stay under a cap (rl_chunk_bytes); the workspace is kept
 * in the context and freed with it.  Synchronises the context's stream.
 * RL_ERR_INVALID (no kernel is launched): a NULL argument, a dtype that is neither, n_pairs < 1, R outside 1 .. 32, M < R, an
 * interior smaller than 8 x 8, a negative offset.
 *
 * rl_shift_images: src_dev [n][ny][nx] of src_dtype -> dst_dev [n][ny][nx] of dst_dtype (RL_F32 / RL_F64 each; no overlap):
 *     dst[i] = max(scipy.ndimage.shift(src[i], (-sy_i, -sx_i), order = order, mode = 'mirror'), floor)
 * with shifts: host [n][2] = (sy, sx): dst[i][y][x] samples the spline of image i at (y + sy, x + sx), whole-sample mirror
 * boundaries in the prefilter and in the evaluation; any finite |shift| <= 1e9.  order: 1 or 3.  floor: any double but nan
 * (-infinity: none).  Computed in float64 with one rounding to the destination type.  Along an axis, prefilter and evaluation of a
 * translation are one finite impulse response on the mirror extension: order 1 the taps (1 - t, t), an integer shift the tap 1.0
 * alone -- a bit-exact copy of the displaced pixels; order 3 the 64 taps of csrc/register_kernels.hpp, the prefilter's impulse
 * response sqrt(3) z^|k| (z = sqrt(3) - 2) cut at |k| = 30, where the dropped tail is at most 8.8e-18 max|src| per axis.  The taps
 * are formed on the host in long double; a pixel is g_0 v_0, then fma(g_m, v_m, .) for m = 1, 2, ...; x first, then y.
 * stats_out: NULL, or host [n][RL_SHIFT_FIELDS] = the count of pixels raised to `floor`, the float64 sum of the stored image in
 * the fixed order of csrc/register_kernels.hpp (thread, binary tree over 256 threads, workgroups in increasing order; no atomics).
 * Writes exactly n * ny * nx values.  Images are processed in chunks whose float64 intermediate stays under a cap (rl_chunk_bytes), in the
 * context's workspace.  Synchronises the context's stream.
 * RL_ERR_INVALID (no kernel is launched): a NULL ctx / source / shifts / destination, a dtype that is neither, n, ny or nx < 1, an
 * order that is neither, floor nan, a shift that is not finite or beyond 1e9, a destination that overlaps the source. */
#define RL_REGISTER_FIELDS 3
#define RL_SHIFT_FIELDS 2
int rl_register_sums(rl_ctx* ctx, const void* ref_dev, int ref_dtype, const int64_t* ref_offsets, const void* mov_dev, int mov_dtype,
                     const int64_t* mov_offsets, int n_pairs, int ny, int nx, int R, int M, double* sums_out, double* ref_out);
int rl_shift_images(rl_ctx* ctx, const void* src_dev, int src_dtype, int n, int ny, int nx, const double* shifts, int order,
                    double floor, void* dst_dev, int dst_dtype, double* stats_out);

/* rl_register_xcorr: the coarse stage of the registration -- the cross-correlation of n_pairs image pairs through the transform,
 * for any search radius: a few 2-D FFTs per pair whatever R.  It PROPOSES an integer displacement; rl_register_sums, the exact
 * float64 window, judges it.  Addressing as rl_register_sums: ref_dev / mov_dev device buffers of ref_dtype / mov_dtype (RL_F32 /
 * RL_F64, each its own), pair i = the ny x nx image at element offset ref_offsets[i] / mov_offsets[i] (host arrays, >= 0, no
 * alignment assumed); many pairs may share a reference, the two buffers may be one.  Sign convention as above: the peak is at d
 * with B[y + d] ~ A[y].
 * Per pair: a = A - mean(A), b = B - mean(B), the means over the whole image in float64 (order below), the centred values rounded
 * to float32; both zero-extended to Ly x Lx, Ly the smallest of 64, 192, 256, 576, 1152 with Ly >= ny + R and Lx likewise from nx
 * (the axes independently; equality allowed: no lag |d| <= R wraps around).  For d in [-R, R]^2
 *     C(d) = sum a[y][x] b[y + dy][x + dx]   over the pixels where both lie inside the image (float32 transforms),
 *     v(d) = (double)C(d) / ((ny - |dy|)(nx - |dx|))   -- the overlap normalisation, without which zero extension pulls the peak to 0.
 * The peak is the first maximum of v in row-major order, compared in float64.  On their way into the transform a and b are each
 * scaled by an exact power of two to a norm in [1, 2) (from E_a, E_b below) and the window is scaled back in float64: the packed
 * transform's rounding error is then relative to ||a|| ||b|| however different the two images' brightness, and any input range fits.
 * peaks_out: host [n_pairs][RL_XCORR_FIELDS] = dy, dx, v at the peak, E_a = sum a^2, E_b = sum b^2, sum of v over the window, sum of
 * v^2 over the window.  E_a or E_b not positive: d = (0, 0) and v = 0 (a flat image).  surface_out: NULL, or host
 * [n_pairs][2 R + 1][2 R + 1] float32 = v, index (dy + R, dx + R) -- for tests and diagnostics.
 * FIXED ORDER (csrc/xcorr_kernels.hpp), no atomics: a mean and an energy are 256 strided partial sums (element t, t + 256, ... in
 * increasing order from 0.0; the energy with fma(a, a, .) on the float32-rounded centred value widened again) joined by a halving
 * tree; the window sums run per window row over its columns in increasing order from 0.0 (s + v; q + v v, two roundings), then over the rows
 * in increasing order.  Results are bit-identical from run to run, a pair's result does not depend on the other pairs of the call,
 * and nothing outside an image is read.  Error of C against exact arithmetic: tests/xcorr_reference.py derives
 *     |C_dev - C| <= kappa eps_f32 (log2 Ly + log2 Lx) ||a||_2 ||b||_2.
 * Pairs are processed in chunks whose spectra stay under a cap (rl_chunk_bytes), in the context's workspace.  Synchronises the context's stream.
 * RL_ERR_INVALID (no kernel is launched): a NULL ctx / buffer / offsets / peaks_out, a dtype that is neither, n_pairs < 1, ny or
 * nx < 1, R < 1, R > min(ny, nx) / 2, ny + R or nx + R > 1152 (the lengths 2304 and 4608 have a column geometry of their own and
 * are not served), a negative offset. */
#define RL_XCORR_FIELDS 7
int rl_register_xcorr(rl_ctx* ctx, const void* ref_dev, int ref_dtype, const int64_t* ref_offsets, const void* mov_dev, int mov_dtype,
                      const int64_t* mov_offsets, int n_pairs, int ny, int nx, int R, double* peaks_out, float* surface_out);

/* rl_register_peaks: the host's NCC, first-maximum search and parabola (registration.ncc_surface, surface_peak) on the device, bit
 * for bit, for n_pairs rows of sums as rl_register_sums forms them.  tot_dev: device [n_pairs][(2 R + 1)^2 * 3 + 2] float64 = per
 * displacement S_b, S_bb, S_ab, then S_a, S_aa.  n_terms: the number of terms of every sum, (ny - 2 M)(nx - 2 M).  Per displacement,
 * in float64 with every operation rounded on its own: va = S_aa - S_a S_a / n, vb = S_bb - S_b S_b / n,
 * c = (S_ab - S_a S_b / n) / sqrt(va vb).  A pair is FLAT when va or any vb is not positive (nan included).  The peak is the first
 * maximum in row-major order; the parabola per axis is delta = (0.5 (m - p)) / ((m - 2 z) + p), 0 where the denominator is 0, and
 * 0 with at_limit set where the peak lies on the window's border; shift = (peak index - R) + delta.
 * peaks_out: host [n_pairs][RL_PEAK_FIELDS] = shift_y, shift_x, value at the peak, at_limit (0 / 1), flat (0 / 1); a flat pair gives
 * 0, 0, 0, 0, 1.  surface_out: NULL, or host [n_pairs][(2 R + 1)^2] = c (zeros for a flat pair).  One workgroup per pair, no
 * atomics: bit-identical from run to run.  Synchronises the context's stream.
 * RL_ERR_INVALID (no kernel is launched): a NULL ctx / tot_dev / peaks_out, n_pairs < 1, R outside 1 .. 32, n_terms not finite or
 * below 1.
 *
 * rl_register_estimate: registration._estimate without the coarse stage, in one call -- the sums of rl_register_sums (addressing,
 * R, M and their checks as there), the peaks of rl_register_peaks on the device, 5 doubles per pair down, then `refine` passes over
 * the pairs that are not flat: each moving image shifted by its current estimate (rl_shift_images, order 3, no floor) into
 * scratch_dev (float64, n_pairs images of ny x nx, not overlapping the images), the sums at R = 1 with the same M, the peaks, and
 * shift += the new offset; such a pass replaces the value, keeps at_limit of the first stage and leaves a pair it finds flat alone.
 * shifts_out: host [n_pairs][2]; fields_out: host [n_pairs][3] = ncc, at_limit, flat; surface_out: NULL, or host
 * [n_pairs][(2 R + 1)^2], the first stage's surfaces.  scratch_dev may be NULL when refine == 0.  Uses the context's workspace and
 * synchronises its stream.
 * RL_ERR_INVALID (no kernel is launched): as rl_register_sums, a NULL shifts_out / fields_out, refine < 0, refine > 0 without a
 * scratch buffer. */
#define RL_PEAK_FIELDS 5
int rl_register_peaks(rl_ctx* ctx, const double* tot_dev, int n_pairs, int R, double n_terms, double* peaks_out, double* surface_out);
int rl_register_estimate(rl_ctx* ctx, const void* ref_dev, int ref_dtype, const int64_t* ref_offsets, const void* mov_dev, int mov_dtype,
                         const int64_t* mov_offsets, int n_pairs, int ny, int nx, int R, int M, int refine, double* scratch_dev,
                         double* shifts_out, double* fields_out, double* surface_out);

/* ---- rotation, scale and shear between views: affine resampling and the sums of a Gauss-Newton step (INTEGRATION.md section 5l,
 * DESIGN.md section 4n) ----
 * rl_warp_images: src_dev [n][sy][sx] of src_dtype -> dst_dev [n][oy][ox] of dst_dtype (RL_F32 / RL_F64 each; no overlap; the output
 * shape is independent of the source's):
 *     dst[i] = max(scipy.ndimage.affine_transform(src[i], [[m00, m01], [m10, m11]], offset = (o0, o1), output_shape = (oy, ox),
 *                                                 order = order, mode = 'mirror'), floor)
 * with xf: host [n][6] = (m00, m01, m10, m11, o0, o1): dst[i][y][x] samples the spline of image i at
 *     Y = fma(m00, y, fma(m01, x, o0)),   X = fma(m10, y, fma(m11, x, o1)),
 * whole-sample mirror boundaries in the prefilter and in the evaluation.  Every entry finite, and the four corners of the output
 * grid must map to |Y|, |X| <= 1e9 (the map is affine, so every pixel then does; F = floor(.) converts exactly to a 32-bit index,
 * which folds to i mod 2 (n - 1) and then to 2 (n - 1) - i where that is >= n; an axis of length 1 maps to 0).  order: 1 or 3.
 * floor: any double but nan (-infinity: none).  Computed in float64 with one rounding to the destination type.
 * ORDER 3: the spline coefficients are the prefilter alone, along x and then along y: per axis the impulse response
 * h[k] = sqrt(3) z^|k|, z = sqrt(3) - 2, |k| <= 30, of rl_shift_images without its evaluation weights (61 taps formed on the host in
 * long double, a coefficient is h_0 v_0, then fma(h_m, v_m, .) for m = 1, 2, ... over the samples mirror(. - 30 + m); the dropped tail
 * is at most 8.8e-18 max|src| per axis), run by the shift's own passes.  The evaluation per axis, with F = floor(Y), t = Y - F,
 * u = 1 - t, s = the double nearest 1/6, every operation rounded on its own:
 *     w_0 = ((u u) u) s    w_1 = (((t t) (t - 2)) 3 + 4) s    w_2 = (((u u) (u - 2)) 3 + 4) s    w_3 = ((t t) t) s
 * at the offsets -1 .. 2 from F (wy from Y, wx from X); with c_ij the coefficient at (Fy - 1 + i, Fx - 1 + j) through the mirror rule:
 *     r_i = wx_0 c_i0, then r_i = fma(wx_j, c_ij, r_i) for j = 1, 2, 3;     v = wy_0 r_0, then v = fma(wy_i, r_i, v) for i = 1, 2, 3.
 * ORDER 1: the weights (1 - t, t) at the offsets 0, 1 on the samples themselves: r_i = (1 - tx) s_i0, then r_i = fma(tx, s_i1, r_i)
 * only where tx != 0; v = (1 - ty) r_0, then v = fma(ty, r_1, v) only where ty != 0.  A weight that is exactly 0 does not read its
 * sample: an integer translation is a bit-exact copy of the displaced pixels, as in rl_shift_images, and the matrix diag(2, 2) with
 * offset (0.5, 0.5) is the 2 x 2 mean ((a + b) + (c + d)) / 4.
 * stats_out: NULL, or host [n][RL_SHIFT_FIELDS] = the count of pixels raised to `floor`, the float64 sum of the stored image, in the
 * fixed order of csrc/affine_kernels.hpp (a thread of an output tile of 32 x 32 over its rows t / 32 + 8 k in increasing order,
 * binary tree over 256 threads, workgroups in increasing order; no atomics).  Writes exactly n * oy * ox values.
 * A tile's source footprint is staged in LDS when it takes at most 48 KB as float64, and read from global memory otherwise: the same
 * arithmetic, the same bits (rl_warp_path: 1 reads every tile directly, 0 -- the default -- decides per tile; for tests and
 * measurements).  Images are processed in chunks whose float64 intermediates (order 3: 16 bytes per source pixel) stay under a cap,
 * in the context's workspace (rl_warp_chunk_bytes: the cap for the later calls on this context, >= 1 byte, at least one image per
 * chunk; the results do not depend on it).  Synchronises the context's stream.
 * RL_ERR_INVALID (no kernel is launched): a NULL ctx / source / xf / destination, a dtype that is neither, n, sy, sx, oy or ox < 1,
 * an order that is neither, floor nan, an entry of xf that is not finite, a corner beyond 1e9, a destination that overlaps the source.
 *
 * rl_affine_sums: the normal equations of one Gauss-Newton step of an intensity-based registration, for every motion model at once.
 * Addressing as rl_register_sums: pair i is the reference A at ELEMENT offset ref_offsets[i] of ref_dev and the moving image W --
 * ALREADY WARPED by the current estimate -- at w_offsets[i] of w_dev, both [ny][nx]; shared references allowed.  M: margin, M >= 1,
 * with ny - 2 M >= 8 and nx - 2 M >= 8; ny * nx < 2^31.  With the interior I = [M, ny - M) x [M, nx - M), every value widened to
 * float64, yc = y - (ny - 1) / 2, xc = x - (nx - 1) / 2 (exact),
 *     gy = 0.5 (W[y+1][x] - W[y-1][x])    gx = 0.5 (W[y][x+1] - W[y][x-1])    w = W[y][x]    a = A[y][x]
 *     phi = (gy, gx, gy yc, gy xc, gx yc, gx xc, w, 1)                    (every product rounded on its own)
 * sums_out: host [n_pairs][RL_AFFINE_FIELDS]: [0, 36) the upper triangle of sum_I phi phi^T in row-major order ((0,0), (0,1), ...,
 * (0,7), (1,1), ...), each term through fma(phi_j, phi_k, .); [36, 44) sum_I phi_j a through fma(phi_j, a, .); [44] sum_I a^2 through
 * fma(a, a, .).  The linearisation a ~ g w + b + phi_{0..5} q, q = g (dt_y, dt_x, dL_00, dL_01, dL_10, dL_11), is linear in (q, g, b):
 * translation, rigid, similarity and affine steps are projections of this one 8 x 8 system on the host.
 * FIXED ORDER (csrc/affine_kernels.hpp), no atomics: the interior's n pixels in row-major order are cut into nb = min(4096,
 * ceil(n / 8192)) runs of ceil(n / nb); thread t of a run's 256 takes its pixels t, t + 256, ... in increasing order from 0.0; the
 * halving tree s[t] = s[t] + s[t + h], h = 128, ..., 1; (((0.0 + run_0) + run_1) + ...).  Bit-identical from run to run, a pair's
 * result does not depend on the other pairs of the call, and nothing outside an image is read.  Pairs are processed in chunks whose
 * partial sums stay under a cap (rl_chunk_bytes), in the context's workspace.  Synchronises the context's stream.
 * RL_ERR_INVALID (no kernel is launched): a NULL argument, a dtype that is neither, n_pairs < 1, M < 1, an interior smaller than
 * 8 x 8, 2^31 pixels or more, a negative offset. */
#define RL_AFFINE_FIELDS 45
int rl_warp_images(rl_ctx* ctx, const void* src_dev, int src_dtype, int n, int sy, int sx, const double* xf, int order, double floor,
                   void* dst_dev, int dst_dtype, int oy, int ox, double* stats_out);
int rl_warp_chunk_bytes(rl_ctx* ctx, size_t bytes);
int rl_warp_path(rl_ctx* ctx, int path);
int rl_affine_sums(rl_ctx* ctx, const void* ref_dev, int ref_dtype, const int64_t* ref_offsets, const void* w_dev, int w_dtype,
                   const int64_t* w_offsets, int n_pairs, int ny, int nx, int M, double* sums_out);

/* ---- bead images: the peak finder of the PSF measurement ----
 * rl_find_peaks: the candidates of n images of ny x nx, src_dtype (RL_F32 / RL_F64) at the ELEMENT offsets offsets[i] of src_dev
 * (host array [n]; any offset >= 0, no alignment assumed).  taps: host float64 w[0 .. 2 h], 0 <= h <= 16; r: the suppression
 * radius, 1 .. 16; b: the border, b >= h + r, with ny, nx >= 2 b + 1.  Every value widened to float64, no contraction, sums in the
 * order written:
 *     u(y, x) = (...((0.0 + w[0] x(y, x - h)) + w[1] x(y, x - h + 1)) + ...) + w[2h] x(y, x + h)
 *     s(y, x) = the same sum over u(y - h + k, x), k ascending
 * D = {b <= y < ny - b, b <= x < nx - b}; lo, hi: the min and max of the non-nan s over D (+inf and -inf when there is none);
 *     t = v > threshold ? v : threshold,   v = lo + rel (hi - lo)
 * A pixel p of D is a candidate when s(p) >= t, s(q) < s(p) for every q with |q - p|_inf <= r that comes before p in row-major
 * order and s(q) <= s(p) for every such q after it -- IEEE comparisons as written: a nan anywhere in the window disqualifies p, and a
 * plateau yields one candidate, its first pixel.
 * Outputs, host arrays: per image the candidates in ROW-MAJOR order, the first cap of them: yx_out [n][cap][2] = (y, x), s_out
 * [n][cap] = s(p), x_out [n][cap] = x(p) widened; count_out [n] the true count (it may exceed cap); levels_out [n][RL_PEAK_LEVELS]
 * = lo, hi, t.  Entries past min(count, cap) are not written.
 * Tiles of 16 x 32 pixels of D with a halo of h + r in LDS (at most 64 KB), a mask word per tile row, ranks from an integer prefix
 * over the mask in row-major order (csrc/bead_kernels.hpp); no atomics: bit-identical from run to run, and an image's result does
 * not depend on the other images of the call.  Images are processed in chunks whose tile partials, masks and candidate lists stay
 * under a cap of 256 MB (at least one image per chunk); the workspace is kept in the context and freed with it.  Synchronises the
 * context's stream.
 * RL_ERR_INVALID (no kernel is launched): a NULL argument, a dtype that is neither, n < 1, h outside 0 .. 16, r outside 1 .. 16,
 * b < h + r, an image smaller than 2 b + 1 on an axis, a negative offset, cap < 1. */
#define RL_PEAK_LEVELS 3
int rl_find_peaks(rl_ctx* ctx, const void* src_dev, int src_dtype, const int64_t* offsets, int n, int ny, int nx, const double* taps,
                  int h, int r, int b, double rel, double threshold, int cap, int32_t* yx_out, double* s_out, double* x_out,
                  int64_t* count_out, double* levels_out);
/* The cap above for the later calls on this context, in bytes (>= 1; a cap below one image's share gives chunks of one image).  The
 * results do not depend on it.  RL_ERR_INVALID: a NULL ctx, 0 bytes. */
int rl_find_peaks_chunk_bytes(rl_ctx* ctx, size_t bytes);

/* ---- camera calibration: temporal statistics of raw stacks, repair of known defect pixels (DESIGN.md
 * section 4m) ----
 * rl_calib: the per-pixel accumulators of one sensor window (y0, x0) + ny x nx of frames of src_ny x src_pitch elements of
 * raw_dtype (RL_RAW_*), on a context.  rl_calib_accumulate adds n_frames contiguous sensor frames at raw_dev (device memory, e.g.
 * filled with rl_device_upload_bytes); the launch is enqueued on the context's stream and nothing outside the window is read.
 *   Integer raw types (u8, u16, i16): S = sum x is int64, Q = sum x^2 is uint64, both exact.  An accumulator holds at most 65535
 *   frames in all: F Q and S^2 then stay below 2^64 and N = F Q - S^2 is formed exactly in uint64 (>= 0 by Cauchy-Schwarz).  The
 *   sums do not depend on how the frames are chunked over calls nor on the launch's work split: a call whose window gives few
 *   workgroups splits its frames over a second grid axis and combines the parts with 64-bit integer atomics.
 *       mean = (double)S / (double)F;   var = F > 1 ? (double)N / (double)(F (F - 1)) : 0        (unbiased)
 *   f32: S and Q are float64, S = S + (double)x, Q = Q + (double)x * (double)x in frame order, calls in sequence, no contraction and
 *   no frame split (the order is part of the definition).  mean = S / F;  var = F > 1 ? (Q - S mean) / (F - 1) : 0.  A non-finite
 *   input makes its pixel's sums, and with them its mean and variance, non-finite; the other pixels are not touched by it.
 * rl_calib_frames: F.  rl_calib_sums: waits for the stream and copies the accumulators as they are to host arrays [ny][nx] of 8-byte
 * values (int64 and uint64, or float64 for f32 raw); either may be NULL, not both.  rl_calib_finalize: float64 maps [ny][nx] in
 * device memory, either may be NULL, not both; enqueued.  rl_calib_reset: zero sums, F = 0.  rl_calib_destroy(NULL) is RL_OK.
 * RL_ERR_INVALID (no kernel is launched): a NULL argument, a raw_dtype that is none of RL_RAW_*, a size below 1, a window that
 * overhangs the frame, n_frames < 1, an accumulate that would take an integer accumulator past 65535 frames (nothing is enqueued, F
 * stays), a finalize before the first frame or with overlapping maps. */
typedef struct rl_calib rl_calib;
int rl_calib_create(rl_ctx* ctx, int raw_dtype, int src_ny, int src_pitch, int y0, int x0, int ny, int nx, rl_calib** out);
int rl_calib_accumulate(rl_calib* c, const void* raw_dev, int n_frames);
int rl_calib_frames(const rl_calib* c, long long* frames);
int rl_calib_sums(rl_calib* c, void* sum_host, void* sumsq_host);
int rl_calib_finalize(rl_calib* c, double* mean_dev, double* var_dev);
int rl_calib_reset(rl_calib* c);
int rl_calib_destroy(rl_calib* c);

/* rl_repair_pixels: the known defect pixels of n_images images [ny][nx] of dtype (RL_F32 / RL_F64) at img_dev, replaced IN PLACE by
 * the median of their good neighbours.  mask_host [ny][nx], nonzero = defect; radius 1 .. 3.  Per image and defect pixel (y, x):
 *   for r = 1 .. radius: the values of the pixels within Chebyshev distance r that are inside the image and not defects, in
 *   row-major order; stop at the first r that yields at least one value;
 *   sort the c values (ascending, nan last, equal values keep their order): the replacement is v[(c - 1) / 2] for odd c and
 *   ((double)v[c / 2 - 1] + (double)v[c / 2]) * 0.5, rounded once to dtype, for even c;
 *   no good pixel within radius: the pixel is left as it is and counted in unrepaired[image] (host array [n_images], may be NULL;
 *   the mask is the same for every image, so are the counts).
 * The kernel reads only pixels that are not defects and writes only pixels that are: in place is free of races by construction, and
 * the result does not depend on the order in which the defects are visited.  The host builds the list of repairable defects (pixel,
 * ring radius, a bit per window position that is a good neighbour), stages it in a workspace kept in the context and enqueues ONE
 * launch over (image, listed defect) on the context's stream; a mask without repairable defects launches nothing.
 * rl_stack_set_defects: the same rule inside rl_stack_run and rl_stack_run_registered, for the plan's window (mask_host [ny][nx] of
 * it, NULL: none -- the default, and then both runs enqueue exactly what they did before).  The repair of a chunk's images follows
 * the chunk's rl_ingest on the context's stream: on the plan's measurement buffer in rl_stack_run, on the staging buffer -- before
 * references and estimates -- in rl_stack_run_registered; in both before rl_deconv_measurement_written.  The ingest statistics stay
 * those of the ingest.  The list is built once, here, and kept on the device until the next call or rl_stack_destroy.
 * RL_ERR_INVALID (no kernel is launched): a NULL argument (but mask_host of rl_stack_set_defects), a dtype that is neither, a size
 * below 1, an image of more than 2^31 - 1 pixels, a radius outside 1 .. 3. */
int rl_repair_pixels(rl_ctx* ctx, void* img_dev, int dtype, int n_images, int ny, int nx, const unsigned char* mask_host, int radius,
                     long long* unrepaired);
int rl_stack_set_defects(rl_stack* st, const unsigned char* mask_host, int radius);

/* ---- line_sted_figure_3.py: the scan-position-by-scan-position imaging simulator (:76-273) ----
 * rl_rotate_image: `rotate` (:382-391) for one [ny][nx] plane -- scipy.ndimage.rotate(order 3,
 * mode 'nearest', reshape=False) about the centre; clip != 0 clips to [0, 1.1 * max(in)].  Host in / out. */
int rl_rotate_image(rl_ctx* ctx, const double* in, double* out, int ny, int nx, double degrees, int clip);

/* One orientation's scan (:172-239), all scan positions in one call, batched on the device.
 * rot_obj, centered_exc: [ny][nx] (the padded, rotated object :169; the blurred excitation :139).
 * positions: [n_pos][2] = (shift_y, shift_x) (:112-137).  display: ascending indices of the positions
 * whose detector images are wanted (the frames the reference renders, :258-263).
 * pos_scalars [n_pos][4] = { glow.max(), inst_detector_sig.max(), cum_detector_sig.max(),
 *   inst_detector_sig.sum() } per position (:252-256; the sum is descan_point's reconstruction value :200).
 * pos_values: descan_line [n_pos][nx] = inst_detector_sig.sum(axis=1) (:192); nondescan_multipoint
 *   [n_pos][ceil(n_y/exc_sep) * ceil(n_x/exc_sep)] = the region sums (:213-220), y major; else unused.
 * display_out [n_display][2][ny][nx] = inst_detector_sig, cum_detector_sig of the display positions.
 * cum_final [ny][nx]: rescan_line's accumulated detector image (:234), else unused.              */
typedef struct rl_fig3_params {
    int imaging_type;    /* 0 descan_point, 1 nondescan_multipoint, 2 descan_line, 3 rescan_line */
    int ny, nx;          /* padded shape */
    int n_y, n_x, pad;   /* object shape and padding (:106-107) */
    int step, exc_sep;   /* scan step (:102); spot separation (:131, multipoint) */
    double psf_sigma;    /* detection blur (:100) */
    double rescan_scale; /* 1 / (R^2 + 1) (:229), rescan_line */
} rl_fig3_params;
int rl_fig3_scan(rl_ctx* ctx, const rl_fig3_params* p, const double* rot_obj, const double* centered_exc,
                 const int* positions, int n_pos, const int* display, int n_display, double* pos_scalars,
                 double* pos_values, double* display_out, double* cum_final);

/* Per-kernel device time: launches each kernel of the RL iteration `reps`
 * times back to back between two hipEvents on the plan's stream and returns
 * the average milliseconds per launch in avg_ms[0..5] = { column pass (H),
 * row pass RATIO, column pass (H_t), row pass UPDATE, row pass FWD, Poisson };
 * avg_ms[6] = frames covered by one launch of the four RL kernels (the RL
 * loop works through the batch in equal slices sized for the Infinity Cache;
 * FWD and Poisson run over the whole batch).  avg_ms must hold 7 doubles.
 * Destroys the current estimate (the next iterate restarts from 1).          */
int rl_deconv_time_kernels(rl_deconv* h, int reps, double* avg_ms);

/* In-situ kernel durations of ONE whole cycle (simulate + k iterations, as rl_deconv_bench_cycles
 * runs it): a hipEvent pair around every launch, recorded on the stream the launch goes to, with
 * the batch slices overlapping on their streams as in production -- the figure a rocprofv3 kernel
 * trace of the same run reports.  avg_ms[8] / launches[8] (may be NULL): average duration and
 * number of launches of { column pass (H), row pass RATIO, column pass (H_t), row pass UPDATE, row
 * pass FWD, row pass INV, Poisson (both kernels), unused (0) };
 * *frames_per_launch: frames one launch of the RL kernels covers.                        */
int rl_deconv_time_cycle(rl_deconv* h, int k, int rng_kind, uint64_t seed, double* avg_ms, double* launches,
                         double* frames_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* RLSTED_H */
