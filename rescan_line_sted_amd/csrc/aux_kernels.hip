// aux_kernels.hip -- small gfx950 kernels around the FFT path: constant fill,
// PSF spectrum (direct DFT of the small PSF support, float64), Poisson noise.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "aux_kernels.hpp"
#include "dev_sync.hpp"
#include "philox_poisson.hpp"
#include "poisson_kernels.hpp"

namespace rl {

template <typename T>
__global__ void k_fill(T* p, size_t n, T value) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = value;
}

// Stage 1: S1[v][a][kx] = sum_b psf[v][a][b] * W_Lx[(kx * ((b - cx) mod Lx)) mod Lx]
__global__ void k_psf_dft_rows(const double* __restrict__ psf, const double2* __restrict__ wx, double2* __restrict__ s1,
                               int py, int px, int lx, int kx) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int a = blockIdx.y, v = blockIdx.z;
    if (k >= kx) return;
    const int cx = (px - 1) / 2;
    const double* row = psf + ((size_t)v * py + a) * px;
    double re = 0.0, im = 0.0;
    for (int b = 0; b < px; ++b) {
        const int off = ((b - cx) % lx + lx) % lx;
        const double2 w = wx[(int)(((long long)k * off) % lx)];
        re += row[b] * w.x;
        im += row[b] * w.y;
    }
    s1[((size_t)v * py + a) * kx + k] = make_double2(re, im);
}

// Stage 2: psf_hat[v][ky][kx] = scale * sum_a S1[v][a][kx] * W_Ly[(ky * ((a - cy) mod Ly)) mod Ly]
template <typename T>
__global__ void k_psf_dft_cols(const double2* __restrict__ s1, const double2* __restrict__ wy, cx<T>* __restrict__ out,
                               int py, int ly, int kx, int pitch, double scale, int transposed) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int ky = blockIdx.y, v = blockIdx.z;
    if (k >= pitch) return;
    const int cy = (py - 1) / 2;
    double re = 0.0, im = 0.0;
    if (k < kx) {
        for (int a = 0; a < py; ++a) {
            const int off = ((a - cy) % ly + ly) % ly;
            const double2 w = wy[(int)(((long long)ky * off) % ly)];
            const double2 s = s1[((size_t)v * py + a) * kx + k];
            re += s.x * w.x - s.y * w.y;
            im += s.x * w.y + s.y * w.x;
        }
    }
    if (transposed) {   // [view][kx][ly]: contiguous along ky for wave-private column transforms
        if (k < kx) out[((size_t)v * kx + k) * ly + ky] = mk<T>((T)(re * scale), (T)(im * scale));
    } else {
        out[((size_t)v * ly + ky) * pitch + k] = mk<T>((T)(re * scale), (T)(im * scale));
    }
}

// noisy = Poisson(noiseless) + 1e-9   (line_sted_tools.py:510).  ONE launch since round 4: a workgroup takes tiles of 2048
// pixels; every pixel gets the first PTRS attempt (philox_poisson_fast: ~87 % are squeeze-accepted and written at once), the
// others go -- index and rate -- to a list in LDS: lam >= 10 from the front, 0 < lam < 10 (multiplication method) from the back.
// The listed pixels are then finished by the same workgroup, densely packed: one PTRS attempt per round (attempt 0 repeats the
// first candidate and continues into the acceptance test the fast path skipped), the survivors repacked into the other list
// between rounds -- a wave never waits for its slowest lane's fifth attempt -- and the small rates through the multiplication
// loop.  Values are a function of (seed, image, pixel) only, so the order is irrelevant: bit for bit what rounds 1-3's two
// launches (all pixels; then a global work list of the rejected ones, which re-read their rates from global memory: 2.9x the
// bytes of read + write) produced, and what the numpy twin produces.
// TILE_IMG: n_pix is a multiple of the tile (512^2, 2048^2, 128^2 ...), so a tile lies inside one image: its index -- and with it
// the Philox key and the base of its rates, through rate_frame -- is resolved once per tile in scalar registers instead of with a
// 32-bit division and a dependent load per pixel.  Tiles that straddle images (200^2) keep the per-pixel path; the draws are the same.
// The grid is the host's to choose (aux_poisson's grid_cap): the tiles are walked in rounds of one per workgroup, so any width
// writes the same bits.  A workgroup's place in the round moves on by 0.618 of the grid from round to round: a plain grid stride
// that divides the image (128 workgroups over 512^2 frames of 128 tiles) would hand a workgroup the same rows of EVERY frame, and
// a tile's cost follows its rates -- dark rows cost nothing, rates below 10 loop -- so that on a batch of one object the slowest
// workgroup sets a narrow launch's duration (measured on the headline's object: 58.8 ms per cycle against 48.1 ms).  A launch as
// wide as its tiles has one round and is the launch it always was.
constexpr int kPoissonE = 8, kPoissonTile = 256 * kPoissonE;
template <typename T, bool TILE_IMG>
__global__ void __launch_bounds__(256) k_poisson(const T* __restrict__ noiseless, T* __restrict__ noisy, unsigned n_pix, unsigned total,
                                                 PoissonKeys keys, int rng_kind) {
    __shared__ unsigned lst_idx[2][kPoissonTile];
    __shared__ T lst_lam[2][kPoissonTile];
    __shared__ unsigned cnt[2], cnt_small;
    const unsigned tid = threadIdx.x;
    const unsigned n_tiles = (total + (unsigned)kPoissonTile - 1u) / (unsigned)kPoissonTile;
    const unsigned turn = (unsigned)((float)gridDim.x * 0.6180339887f) | 1u;
    for (unsigned first = 0, round = 0; first < n_tiles; first += gridDim.x, ++round) {
        const unsigned tile = first + (blockIdx.x + round * turn) % gridDim.x;
        if (tile >= n_tiles) continue;        // (uniform; the last round may be short)
        const unsigned tile0 = tile * (unsigned)kPoissonTile;
        if (tid == 0) cnt[0] = cnt_small = 0;
        __syncthreads();
        const unsigned img_t = TILE_IMG ? tile0 / n_pix : 0u;   // (workgroup uniform)
        const T* __restrict__ rates_t = TILE_IMG ? keys.image_rates(noiseless, img_t, n_pix) : nullptr;
#pragma unroll
        for (int e = 0; e < kPoissonE; ++e) {
            const unsigned i = tile0 + tid + 256u * (unsigned)e;
            if (i < total) {
                const T lam_t = TILE_IMG ? rates_t[i - img_t * n_pix] : keys.rate(noiseless, i, n_pix);
                const double lam = (double)lam_t;
                if (rng_kind != 1) {
                    noisy[i] = (T)(lam + 1e-9);
                } else {
                    const unsigned img = TILE_IMG ? img_t : i / n_pix, pix = i - img * n_pix;   // (32-bit division per pixel)
                    double k;
                    if (philox_poisson_fast(lam, keys.seed(img), keys.image(img), pix, &k)) {
                        noisy[i] = (T)(k + 1e-9);
                    } else if (lam >= 10.0) {
                        const unsigned q = atomicAdd(&cnt[0], 1u);
                        lst_idx[0][q] = i;
                        lst_lam[0][q] = lam_t;
                    } else {
                        const unsigned q = kPoissonTile - 1u - atomicAdd(&cnt_small, 1u);
                        lst_idx[0][q] = i;
                        lst_lam[0][q] = lam_t;
                    }
                }
            }
        }
        __syncthreads();
        if (rng_kind != 1) continue;          // (uniform)
        // lam >= 10: attempt `blk` of every pixel still listed
        unsigned n = cnt[0];
        const unsigned n_small = cnt_small;
        int cur = 0;
        for (unsigned blk = 0; n > 0; ++blk) {
            if (tid == 0) cnt[cur ^ 1] = 0;
            __syncthreads();
            const bool last = blk + 1 == kPoissonMaxBlocks;
            for (unsigned q = tid; q < n; q += 256u) {
                const unsigned i = lst_idx[cur][q];
                const T lam_t = lst_lam[cur][q];
                const unsigned img = TILE_IMG ? img_t : i / n_pix, pix = i - img * n_pix;
                const unsigned long long seed = keys.seed(img);
                double k;
                const bool done = philox_ptrs_attempt((double)lam_t, (unsigned)seed, (unsigned)(seed >> 32), keys.image(img), pix, blk, &k);
                if (done || last) {
                    noisy[i] = (T)((done || k >= 0.0 ? k : 0.0) + 1e-9);
                } else {
                    const unsigned q2 = atomicAdd(&cnt[cur ^ 1], 1u);   // (at most n <= front region: never reaches the small rates at the back of list 0)
                    lst_idx[cur ^ 1][q2] = i;
                    lst_lam[cur ^ 1][q2] = lam_t;
                }
            }
            __syncthreads();
            n = cnt[cur ^ 1];
            cur ^= 1;
        }
        // 0 < lam < 10: multiplication method, one pixel per lane
        for (unsigned q = tid; q < n_small; q += 256u) {
            const unsigned at = kPoissonTile - 1u - q, i = lst_idx[0][at];
            const unsigned img = TILE_IMG ? img_t : i / n_pix;
            noisy[i] = (T)(philox_poisson((double)lst_lam[0][at], keys.seed(img), keys.image(img), i - img * n_pix) + 1e-9);
        }
        __syncthreads();                      // the lists are free for the next tile
    }
}

// Frames that share rate images (keys.rate_frame), Philox: groups of kPoissonGroup frames per 256-pixel tile, the PTRS set-up once
// per pixel and run of equal rate images instead of once per frame (poisson_kernels.hpp).  29.0 KB of LDS against k_poisson's 32.8.
struct PoissonSync : DevSync {
    __device__ __forceinline__ unsigned lds_add(unsigned* p, unsigned v) const { return atomicAdd(p, v); }
};
template <typename T>
// amdgpu_waves_per_eu(5): 96 vector registers instead of 98, so that the fifth workgroup per CU that the LDS allows fits the register
// file too; 2 registers go to 12 B of scratch per lane for it (tests/test_poisson_groups_cpu.py holds the kernel to that).  Kernel
// median 6.5 % lower with it, and the headline's rounds all below the parent's only with it (profiles/poisson_groups).
__global__ void __launch_bounds__(kPoissonGroupPix) __attribute__((amdgpu_waves_per_eu(5))) k_poisson_groups(PoissonGroupParams<T> p) {
    __shared__ __attribute__((aligned(8))) unsigned char lds[kPoissonGroupLds];
    poisson_groups_body<T>(p, threadIdx.x, blockIdx.x, gridDim.x, lds, PoissonSync{});
}

// ---- host <-> plan staging: float64 host arrays are converted on the device -----------
// per-frame sums of a stack [frames][n], accumulated in float64 (wavefront shuffles).  grid (frames, chunks): workgroup (f, c) sums
// the c-th of `chunks` equal sections of frame f into out[f * chunks + c] -- chunks == 1: the frame's sum itself.  Few large frames
// (a 4096^2 float64 image is 134 MB: one workgroup read it at 19 GB/s, 7 ms) take kSumChunks sections and a second launch of the
// same kernel over the partial sums; the order of the additions is fixed either way, so a frame's sum does not depend on the batch.
template <typename T>
__global__ void __launch_bounds__(1024) k_frame_sums(const T* __restrict__ x, size_t n, double* __restrict__ out) {
    __shared__ double part[16];
    const size_t chunks = gridDim.y, len = (n + chunks - 1) / chunks, i0 = blockIdx.y * len, i1 = i0 + len < n ? i0 + len : n;
    const T* f = x + (size_t)blockIdx.x * n;
    double v = 0.0;
    for (size_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) v += (double)f[i];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x < 64) {
        v = threadIdx.x < (blockDim.x >> 6) ? part[threadIdx.x] : 0.0;
        for (int off = 8; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (threadIdx.x == 0) out[(size_t)blockIdx.x * chunks + blockIdx.y] = v;
    }
}
// sums[0 .. frames) <- the frames' sums; sums[frames .. frames * (1 + kSumChunks)) is scratch (aux_sums_elems)
template <typename T>
static void frame_sums(const T* x, size_t n, size_t frames, double* sums, hipStream_t s) {
    if (n >= ((size_t)1 << 20) && frames * kSumChunks <= 8192) {
        double* part = sums + frames;
        k_frame_sums<T><<<dim3((unsigned)frames, kSumChunks), 1024, 0, s>>>(x, n, part);
        k_frame_sums<double><<<dim3((unsigned)frames, 1), 64, 0, s>>>(part, (size_t)kSumChunks, sums);
    } else {
        k_frame_sums<T><<<dim3((unsigned)frames, 1), 1024, 0, s>>>(x, n, sums);
    }
}

// dst[f][i] = (T)(src[f][i] * (target[f] / sums[f]))   (target == nullptr: plain conversion)
template <typename T>
__global__ void k_scale_convert(const double* __restrict__ src, T* __restrict__ dst, size_t n, size_t frames,
                                const double* __restrict__ target, const double* __restrict__ sums) {
    const size_t total = n * frames;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / n;
        const double k = target ? target[f] / sums[f] : 1.0;
        dst[i] = (T)(src[i] * k);
    }
}

template <typename T>
__global__ void k_to_f64(const T* __restrict__ src, double* __restrict__ dst, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = (double)src[i];
}

static unsigned blocks_for(size_t n, unsigned block) {
    size_t b = (n + block - 1) / block;
    return (unsigned)(b > 2048 ? 2048 : (b ? b : 1));   // grid-stride beyond 2048 workgroups
}

hipError_t aux_fill(int dtype, void* p, size_t n, double value, hipStream_t s) {
    if (dtype == DT_F32) k_fill<float><<<blocks_for(n, 256), 256, 0, s>>>((float*)p, n, (float)value);
    else k_fill<double><<<blocks_for(n, 256), 256, 0, s>>>((double*)p, n, value);
    return hipGetLastError();
}

hipError_t aux_psf_spectrum(int dtype, const double* psf_dev, const void* wx_dev, const void* wy_dev, void* s1_dev,
                            void* out, int n_psf, int py, int px, int ly, int lx, int kx, int pitch, int transposed,
                            hipStream_t s) {
    k_psf_dft_rows<<<dim3((kx + 127) / 128, py, n_psf), 128, 0, s>>>(psf_dev, (const double2*)wx_dev, (double2*)s1_dev, py, px, lx, kx);
    const double scale = 1.0 / ((double)ly * (double)lx);
    if (dtype == DT_F32)
        k_psf_dft_cols<float><<<dim3((pitch + 127) / 128, ly, n_psf), 128, 0, s>>>((const double2*)s1_dev, (const double2*)wy_dev, (cx<float>*)out, py, ly, kx, pitch, scale, transposed);
    else
        k_psf_dft_cols<double><<<dim3((pitch + 127) / 128, ly, n_psf), 128, 0, s>>>((const double2*)s1_dev, (const double2*)wy_dev, (cx<double>*)out, py, ly, kx, pitch, scale, transposed);
    return hipGetLastError();
}

// Real parts of a complex array + max |im| and max |z| (stats[0], stats[1]; zeroed by the caller): a
// point-symmetric PSF has a real spectrum, which the column kernels can then use as a real multiplier.
// Non-negative doubles order like their bit patterns, so the maxima are integer atomics.
template <typename T>
__global__ void k_split_real(const cx<T>* __restrict__ z, size_t n, T* __restrict__ re, double* __restrict__ stats) {
    double im = 0.0, ab = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {   // grid stride
        const cx<T> v = z[i];
        re[i] = v.re;
        im = fmax(im, fabs((double)v.im));
        ab = fmax(ab, fmax(fabs((double)v.re), fabs((double)v.im)));
    }
    for (int off = 32; off > 0; off >>= 1) {
        im = fmax(im, __shfl_down(im, off, 64));
        ab = fmax(ab, __shfl_down(ab, off, 64));
    }
    if (threadIdx.x % 64 == 0) {
        atomicMax((unsigned long long*)stats, (unsigned long long)__double_as_longlong(im));
        atomicMax((unsigned long long*)stats + 1, (unsigned long long)__double_as_longlong(ab));
    }
}

hipError_t aux_split_real(int dtype, const void* z, size_t n, void* re, double* stats, hipStream_t s) {
    hipError_t e = hipMemsetAsync(stats, 0, 2 * sizeof(double), s);
    if (e != hipSuccess) return e;
    const unsigned g = blocks_for(n, 256);
    if (dtype == DT_F32) k_split_real<float><<<g, 256, 0, s>>>((const cx<float>*)z, n, (float*)re, stats);
    else k_split_real<double><<<g, 256, 0, s>>>((const cx<double>*)z, n, (double*)re, stats);
    return hipGetLastError();
}

// H_t(ones) without a transform: one thread per pixel of the normaliser, the arithmetic is box_norm_pixel (aux_kernels.hpp)
template <typename T>
__global__ void k_box_norm(const double* __restrict__ integ, T* __restrict__ out, int V, int py, int px, int ny, int nx) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= nx) return;
    out[(size_t)i * nx + j] = box_norm_pixel<T>(integ, V, py, px, ny, nx, i, j);
}

hipError_t aux_box_norm(int dtype, const double* integral_dev, void* out, int V, int py, int px, int ny, int nx, hipStream_t s) {
    const dim3 grid((unsigned)((nx + 255) / 256), (unsigned)ny);
    if (dtype == DT_F32) k_box_norm<float><<<grid, 256, 0, s>>>(integral_dev, (float*)out, V, py, px, ny, nx);
    else k_box_norm<double><<<grid, 256, 0, s>>>(integral_dev, (double*)out, V, py, px, ny, nx);
    return hipGetLastError();
}

hipError_t aux_poisson(int dtype, const void* noiseless, void* noisy, unsigned n_pix, unsigned n_img, unsigned image0,
                       unsigned long long seed, int rng_kind, void* list_ws, hipStream_t s,
                       const unsigned long long* frame_seeds, const unsigned* frame_ids, unsigned V, const unsigned* rate_frame,
                       unsigned grid_cap, bool groups) {
    (void)list_ws;   // (rounds 1-3: the global work list between the two launches)
    const PoissonKeys keys{seed, image0, V ? V : 1u, frame_seeds, frame_ids, rate_frame};
    const size_t total = (size_t)n_pix * n_img;
    if (total >= 0xffffffffull - (size_t)kPoissonTile * kPoissonGrid) return hipErrorInvalidValue;      // 32-bit pixel indices (and their tile stride)
    if (total == 0) return hipSuccess;
    const size_t tiles = (total + kPoissonTile - 1) / kPoissonTile;
    const size_t cap = grid_cap < 1 ? 1 : grid_cap > kPoissonGrid ? kPoissonGrid : grid_cap;
    const unsigned g = (unsigned)(tiles > cap ? cap : tiles);
    if (aux_poisson_groups(groups, rng_kind, rate_frame != nullptr)) {   // a sharing slice
        const unsigned items = poisson_group_items(n_pix, n_img / keys.V, keys.V);
        const unsigned gg = (unsigned)(items > cap ? cap : items);
        if (dtype == DT_F32) k_poisson_groups<float><<<gg, kPoissonGroupPix, 0, s>>>(PoissonGroupParams<float>{(const float*)noiseless, (float*)noisy, n_pix, n_img / keys.V, keys});
        else k_poisson_groups<double><<<gg, kPoissonGroupPix, 0, s>>>(PoissonGroupParams<double>{(const double*)noiseless, (double*)noisy, n_pix, n_img / keys.V, keys});
        return hipGetLastError();
    }
    const bool tile_img = n_pix % (unsigned)kPoissonTile == 0;
    auto launch = [&](auto zero, auto in_image) {
        using T = decltype(zero);
        k_poisson<T, decltype(in_image)::value><<<g, 256, 0, s>>>((const T*)noiseless, (T*)noisy, n_pix, (unsigned)total, keys, rng_kind);
    };
    if (dtype == DT_F32) tile_img ? launch(0.0f, std::true_type{}) : launch(0.0f, std::false_type{});
    else tile_img ? launch(0.0, std::true_type{}) : launch(0.0, std::false_type{});
    return hipGetLastError();
}

hipError_t aux_scale_convert(int dtype, const double* src, void* dst, size_t n, size_t frames, const double* target,
                             double* sums, hipStream_t s, bool want_sums) {
    if (target || want_sums) frame_sums<double>(src, n, frames, sums, s);
    const unsigned g = blocks_for(n * frames, 256);
    if (dtype == DT_F32) k_scale_convert<float><<<g, 256, 0, s>>>(src, (float*)dst, n, frames, target, sums);
    else k_scale_convert<double><<<g, 256, 0, s>>>(src, (double*)dst, n, frames, target, sums);
    return hipGetLastError();
}

template <typename T>
__global__ void k_any_negative(const T* __restrict__ x, size_t n, int* __restrict__ flag) {
    bool neg = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) neg = neg || x[i] < (T)0;
    if (__any(neg) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}
hipError_t aux_any_negative(int dtype, const void* src, size_t n, int* flag, hipStream_t s) {
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e != hipSuccess || n == 0) return e;
    const unsigned g = blocks_for(n, 256);
    if (dtype == DT_F32) k_any_negative<float><<<g, 256, 0, s>>>((const float*)src, n, flag);
    else k_any_negative<double><<<g, 256, 0, s>>>((const double*)src, n, flag);
    return hipGetLastError();
}

hipError_t aux_image_sums(int dtype, const void* src, size_t n, size_t frames, double* sums, hipStream_t s) {
    if (frames == 0) return hipSuccess;
    if (dtype == DT_F32) frame_sums<float>((const float*)src, n, frames, sums, s);
    else frame_sums<double>((const double*)src, n, frames, sums, s);
    return hipGetLastError();
}

// dst[f][i] = (T)(src[idx[f]][i] * (target[f] / sums[idx[f]]))   (target == nullptr: plain conversion): frames that share an
// object (a sweep's seeds) are staged and uploaded once
template <typename T>
__global__ void k_scale_convert_indexed(const double* __restrict__ src, const unsigned* __restrict__ idx, T* __restrict__ dst, size_t n,
                                        size_t frames, const double* __restrict__ target, const double* __restrict__ sums) {
    const size_t total = n * frames;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / n, u = idx[f];
        const double k = target ? target[f] / sums[u] : 1.0;
        dst[i] = (T)(src[u * n + (i - f * n)] * k);
    }
}
hipError_t aux_scale_convert_indexed(int dtype, const double* src, const unsigned* idx, size_t n_unique, void* dst, size_t n, size_t frames,
                                     const double* target, double* sums, hipStream_t s) {
    if (target) frame_sums<double>(src, n, n_unique, sums, s);
    const unsigned g = blocks_for(n * frames, 256);
    if (dtype == DT_F32) k_scale_convert_indexed<float><<<g, 256, 0, s>>>(src, idx, (float*)dst, n, frames, target, sums);
    else k_scale_convert_indexed<double><<<g, 256, 0, s>>>(src, idx, (double*)dst, n, frames, target, sums);
    return hipGetLastError();
}

hipError_t aux_to_f64(int dtype, const void* src, double* dst, size_t total, hipStream_t s) {
    const unsigned g = blocks_for(total, 256);
    if (dtype == DT_F32) k_to_f64<float><<<g, 256, 0, s>>>((const float*)src, dst, total);
    else k_to_f64<double><<<g, 256, 0, s>>>((const double*)src, dst, total);
    return hipGetLastError();
}

template <typename S, typename D>
__global__ void k_cast(const S* __restrict__ src, D* __restrict__ dst, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) dst[i] = (D)src[i];
}
hipError_t aux_cast(int dtype_src, const void* src, int dtype_dst, void* dst, size_t total, hipStream_t s) {
    if (total == 0) return hipSuccess;
    if (dtype_src == dtype_dst) return hipMemcpyAsync(dst, src, total * (dtype_src == DT_F32 ? 4 : 8), hipMemcpyDeviceToDevice, s);
    const unsigned g = blocks_for(total, 256);
    if (dtype_src == DT_F32) k_cast<float, double><<<g, 256, 0, s>>>((const float*)src, (double*)dst, total);
    else k_cast<double, float><<<g, 256, 0, s>>>((const double*)src, (float*)dst, total);
    return hipGetLastError();
}

// dst image j = src image list[j / V] * V + j % V   (images of n values; src and dst do not overlap)
template <typename T>
__global__ void k_gather_images(const T* __restrict__ src, T* __restrict__ dst, const unsigned* __restrict__ list, size_t n, size_t images,
                                unsigned V) {
    const size_t total = n * images;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t j = i / n;
        dst[i] = src[((size_t)list[j / V] * V + j % V) * n + (i - j * n)];
    }
}
hipError_t aux_gather_images(int dtype, const void* src, void* dst, const unsigned* list, size_t n, size_t images, unsigned V, hipStream_t s) {
    if (images == 0 || n == 0) return hipSuccess;
    const unsigned g = blocks_for(n * images, 256);
    if (dtype == DT_F32) k_gather_images<float><<<g, 256, 0, s>>>((const float*)src, (float*)dst, list, n, images, V ? V : 1u);
    else k_gather_images<double><<<g, 256, 0, s>>>((const double*)src, (double*)dst, list, n, images, V ? V : 1u);
    return hipGetLastError();
}

size_t aux_poisson_workspace_bytes(size_t total_pixels) {
    (void)total_pixels;
    return 256;      // (the sampler keeps its work lists in LDS since round 4; the callers' buffers stay for the interface)
}

}  // namespace rl
