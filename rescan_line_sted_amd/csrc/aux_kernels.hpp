// aux_kernels.hpp -- host-callable launchers of aux_kernels.hip, and the per-pixel arithmetic of the box normaliser as a
// host-compilable function (the CPU tests run it through tests/emu/sep_emu.cpp; the header includes without HIP for that)
#pragma once
#include "fft_core.hpp"

#include <cstddef>

#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
#include <hip/hip_runtime.h>
#include "kernel_table.hpp"
#endif

namespace rl {

// H_t(ones) without a transform (line_sted_tools.py:589-592): the 'same' convolution of an image of ones with a PSF is
// the sum of the PSF over the rectangle of taps that still meet the image,
//     conv(1, p)[i][j] = sum over a in [i + cy - ny + 1, i + cy], b in [j + cx - nx + 1, j + cx] (inside the PSF) of p[a][b],
// i.e. four reads of the PSF's float64 integral image I[a][b] = sum_{a' < a, b' < b} p[a'][b'] per view (sep_taps.hpp
// box_integral_images: integ [V][py+1][px+1]); each view's sum is clamped at 0 as the reference clamps each view's convolution
// (:587).  Exact to float64 rounding, where the transform path of an f32 plan carries ~2e-7 of white rounding noise -- an error
// every iteration multiplies into the estimate again.  Pixel (i, j) of the [ny][nx] normaliser:
template <typename T>
RL_HD T box_norm_pixel(const double* __restrict__ integ, int V, int py, int px, int ny, int nx, int i, int j) {
    const int cy = (py - 1) / 2, cx = (px - 1) / 2;
    const int a0 = i + cy - ny + 1 > 0 ? i + cy - ny + 1 : 0, a1 = (i + cy < py - 1 ? i + cy : py - 1) + 1;
    const int b0 = j + cx - nx + 1 > 0 ? j + cx - nx + 1 : 0, b1 = (j + cx < px - 1 ? j + cx : px - 1) + 1;
    double acc = 0.0;
    if (a1 > a0 && b1 > b0) {
        for (int v = 0; v < V; ++v) {
            const double* I = integ + (size_t)v * (py + 1) * (px + 1);
            const double s = (I[(size_t)a1 * (px + 1) + b1] - I[(size_t)a0 * (px + 1) + b1]) - (I[(size_t)a1 * (px + 1) + b0] - I[(size_t)a0 * (px + 1) + b0]);
            acc += s > 0.0 ? s : 0.0;
        }
    }
    return (T)acc;
}

#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t aux_fill(int dtype, void* p, size_t n, double value, hipStream_t s);
// psf_dev: [n_psf][py][px] float64 on the device.  wx/wy: float64 twiddle tables
// exp(-2 pi i m / L).  s1_dev: scratch [n_psf][py][kx] complex128.
// out: [n_psf][ly][pitch] complex of `dtype` (or [n_psf][kx][ly] when transposed), scaled by 1/(ly*lx).
hipError_t aux_psf_spectrum(int dtype, const double* psf_dev, const void* wx_dev, const void* wy_dev, void* s1_dev,
                            void* out, int n_psf, int py, int px, int ly, int lx, int kx, int pitch, int transposed,
                            hipStream_t s);
// list_ws: device scratch of at least aux_poisson_workspace_bytes(n_pix * n_img) bytes.
// image0: index of the first image in the Philox counter (the draws of an image do not depend on
// which slice of the batch a launch covers).
size_t aux_poisson_workspace_bytes(size_t total_pixels);
// frame_seeds / frame_ids (device arrays, one entry per frame of V views each) override seed / image0:
// image (frame f, view v) then draws with seed frame_seeds[f] and image index frame_ids[f]*V + v.
// rate_frame (device array, one entry per frame of the launch; nullptr: image i's rates are image i of `noiseless`): frame f's
// rates are images rate_frame[f]*V + v of `noiseless` -- frames that carry the same object are simulated once.  The Philox
// counters stay those of the frame itself, so every draw is the one it would be from a copy of the rates.
// grid_cap: at most so many workgroups (1 .. kPoissonGrid).  The tiles are walked with a grid stride and a value is a function of
// (seed, image, pixel) alone: a launch of any width writes the same bits -- a narrow one leaves the chip to the kernels beside it.
// groups: a launch with rate_frame and the Philox generator (aux_poisson_groups) draws through k_poisson_groups -- frame groups
// per pixel tile, the sampler's rate-only set-up once per pixel and run of frames with one rate image (poisson_kernels.hpp) --,
// the same bits; every other launch, and every launch with groups == false, through k_poisson.
constexpr unsigned kPoissonGrid = 4096;
inline bool aux_poisson_groups(bool groups, int rng_kind, bool rate_frame) { return groups && rate_frame && rng_kind == 1; }
hipError_t aux_poisson(int dtype, const void* noiseless, void* noisy, unsigned n_pix, unsigned n_img, unsigned image0,
                       unsigned long long seed, int rng_kind, void* list_ws, hipStream_t s,
                       const unsigned long long* frame_seeds = nullptr, const unsigned* frame_ids = nullptr, unsigned V = 1,
                       const unsigned* rate_frame = nullptr, unsigned grid_cap = kPoissonGrid, bool groups = true);
// float64 stack [frames][n] (device) -> plan dtype, each frame scaled to sum target[f]
// Every `sums` argument below is device memory of aux_sums_elems(frames) doubles: the frames' sums, then scratch for the partial
// sums of large frames (aux_kernels.hip frame_sums).
constexpr size_t kSumChunks = 64;
inline size_t aux_sums_elems(size_t frames) { return frames * (1 + kSumChunks); }
// (target: device array of `frames` doubles; target == nullptr: no scaling)
// want_sums: fill `sums` even without a target (the caller reads the frames' levels)
hipError_t aux_scale_convert(int dtype, const double* src, void* dst, size_t n, size_t frames, const double* target,
                             double* sums, hipStream_t s, bool want_sums = false);
// *flag = 1 if any of the n values is negative, else 0 (flag: device memory)
hipError_t aux_any_negative(int dtype, const void* src, size_t n, int* flag, hipStream_t s);
// sums[f] = sum of image f of a stack [frames][n] in the plan's dtype (float64 accumulation)
hipError_t aux_image_sums(int dtype, const void* src, size_t n, size_t frames, double* sums, hipStream_t s);
// as aux_scale_convert with frame f taken from staged object idx[f] (n_unique staged objects; sums: [n_unique] scratch)
hipError_t aux_scale_convert_indexed(int dtype, const double* src, const unsigned* idx, size_t n_unique, void* dst, size_t n, size_t frames,
                                     const double* target, double* sums, hipStream_t s);
hipError_t aux_to_f64(int dtype, const void* src, double* dst, size_t total, hipStream_t s);
// dst[i] = (dst type) src[i]: a plan buffer into a result buffer of another arithmetic type (same type: a device copy)
hipError_t aux_cast(int dtype_src, const void* src, int dtype_dst, void* dst, size_t total, hipStream_t s);
// dst image j = src image list[j / V] * V + j % V for `images` images of n values in the plan's dtype (list: device array; src
// and dst must not overlap): the representatives' objects into their compact buffer, the shared rates back out to every frame
hipError_t aux_gather_images(int dtype, const void* src, void* dst, const unsigned* list, size_t n, size_t images, unsigned V, hipStream_t s);
// re[i] = z[i].re for n complex values of `dtype`; stats (device, 2 doubles) <- max |im|, max(|re|, |im|)
hipError_t aux_split_real(int dtype, const void* z, size_t n, void* re, double* stats, hipStream_t s);
// out [ny][nx] (plan dtype) = sum_v max(conv_same(ones, psf_v), 0) from the PSFs' float64 integral images
// integral_dev [V][py+1][px+1] (I[a][b] = sum of psf[a' < a][b' < b]): H_t(ones) to float64 rounding, no transform
hipError_t aux_box_norm(int dtype, const double* integral_dev, void* out, int V, int py, int px, int ny, int nx, hipStream_t s);
#endif
}  // namespace rl
