// sep_kernels.hpp -- the direct stencils of sep_kernels.hip (separable stencils for rank-1 PSFs, the direct 2-D stencil for small
// PSFs that are not rank 1): the workgroup bodies as host-compilable templates, so that the CPU tests run the very same code
// (tests/emu/sep_emu.cpp, one OS thread per GPU thread, under AddressSanitizer in tools/asan_emu.sh), the LDS byte counts and the
// size rules that launcher, plan and emulator share, and the launchers.
//
// Semantics (the FFT path's): out[i][j] = sum_ab x[i + cy - a][j + cx - b] p[a][b], cy = (py-1)/2, cx = (px-1)/2, zero outside the
// image, each view's result clamped at 0 before anything else is done with it.
//
// A body takes the kernel's arguments, the thread index t, the three block indices, the workgroup's dynamic LDS and a Sync whose
// wg() is the workgroup barrier.  The *_body overloads take the arguments as a parameter struct and forward to the *_impl form,
// whose pointer PARAMETERS carry __restrict__ (a restrict-qualified struct member tells the compiler nothing).
#pragma once
#include "fft_core.hpp"

#include <cstddef>

#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
#include <hip/hip_runtime.h>
#include "kernel_table.hpp"
#endif

namespace rl {
enum { SEP_STORE_ = 0, SEP_RATIO_ = 1, SEP_SUM_ = 2, SEP_UPDATE_ = 3 };   // epilogues of the column pass
enum SepMode { SEP_STORE = 0, SEP_RATIO = 1, SEP_SUM = 2, SEP_UPDATE = 3 };

constexpr int kRowSeg = 256;   // outputs per workgroup in the row pass (= its threads)
constexpr int kColW = 64, kColH = 32;
constexpr int kSepThreads = 256;            // threads of a column-pass / one-kernel workgroup
constexpr size_t kSep2dMaxLds = 160 * 1024;
constexpr size_t kSepMaxLds = 160 * 1024;   // LDS of a gfx950 compute unit

// ---- LDS byte counts (what the launchers pass as dynamic LDS) and the size rules built on them.  esize: sizeof(T); th: the tile
// height of the one-kernel form (32 or 64).
RL_HD size_t sep_rows_lds(size_t esize, int px) { return (size_t)(kRowSeg + px - 1) * esize; }
RL_HD size_t sep_cols_lds(size_t esize, int py) { return (size_t)(kColH + py - 1) * kColW * esize; }
RL_HD size_t sep2d_lds(size_t esize, int th, int py, int px, int V, bool direct) {
    const int nca = (py + 7) / 8, ncb = (px + 7) / 8;
    if (direct) return ((size_t)(th + 8 * nca) * ((kColW + 8 * ncb) | 1) + (size_t)V * px * 8 * nca) * esize;
    return ((size_t)(th + 8 * nca) * (((kColW + 8 * ncb) | 1) + kColW + 1) + (size_t)V * 8 * (nca + ncb)) * esize;
}
RL_HD bool sep2d_fits_tile(size_t esize, int th, int py, int px, int V) { return sep2d_lds(esize, th, py, px, V, false) <= kSep2dMaxLds; }
RL_HD bool direct2d_fits_tile(size_t esize, int th, int py, int px, int V) { return sep2d_lds(esize, th, py, px, V, true) <= kSep2dMaxLds; }
// the two-pass form: the column pass stages (32 + py - 1) rows of 64 columns, the row pass 256 + px - 1 values
RL_HD bool sep_two_pass_fits_esize(size_t esize, int py, int px) {
    return sep_cols_lds(esize, py) <= kSepMaxLds && sep_rows_lds(esize, px) <= 65536;
}

// ---- row pass: one workgroup = 256 outputs of one row, the row segment + halo staged in LDS.
// out[img][y][x] = sum_b in[src(img)][y][x + cx - b] * v[view(img)][b];  grid (ceil(nx / 256), ny, images)
template <typename T>
struct SepRowsParams {
    const T* in;       // [images / in_div][ny][nx]
    T* out;            // [images][ny][nx]
    const T* taps_v;   // [V][px]
    int ny, nx, px, V, in_div;
};

template <typename T, class Sync>
RL_HD void sep_rows_impl(const T* __restrict__ in, T* __restrict__ out, const T* __restrict__ taps_v, int ny, int nx, int px, int V,
                         int in_div, int t, int bx, int by, int bz, unsigned char* smem, Sync& sync) {
    T* seg = reinterpret_cast<T*>(smem);                    // [kRowSeg + px - 1]
    const int img = bz, y = by, x0 = bx * kRowSeg;
    const int cx = (px - 1) / 2, view = img % V;
    const T* __restrict__ row = in + ((size_t)(img / in_div) * ny + y) * nx;
    // input index of seg[i]: x0 + i + cx - (px - 1)
    for (int i = t; i < kRowSeg + px - 1; i += kRowSeg) {
        const int xi = x0 + i + cx - (px - 1);
        seg[i] = (xi >= 0 && xi < nx) ? row[xi] : (T)0;
    }
    sync.wg();
    const int x = x0 + t;
    if (x >= nx) return;
    const T* __restrict__ v = taps_v + (size_t)view * px;
    T acc = 0;
    for (int b = 0; b < px; ++b) acc += seg[t + (px - 1) - b] * v[b];   // x + cx - b  <->  seg[t + px - 1 - b]
    out[((size_t)img * ny + y) * nx + x] = acc;
}
template <typename T, class Sync>
RL_HD void sep_rows_body(const SepRowsParams<T>& p, int t, int bx, int by, int bz, unsigned char* smem, Sync& sync) {
    sep_rows_impl<T>(p.in, p.out, p.taps_v, p.ny, p.nx, p.px, p.V, p.in_div, t, bx, by, bz, smem, sync);
}

// ---- column pass: one workgroup = 64 columns x 32 rows of outputs, the (32 + py - 1) x 64 tile of row-pass results staged in
// LDS; the Richardson-Lucy pointwise steps are its epilogues (ref:520-531).  Images of `tmp` are [frame*V + view].
//   SEP_STORE : dst[frame*V+view] = max(conv, 0)                                   (H / noiseless)
//   SEP_RATIO : dst[frame*V+view] = aux[frame*V+view] / max(conv, 0)               (measurement / H(est); 1 where conv <= 0)
//   SEP_SUM   : dst[frame] = sum_v max(conv_v, 0) (/ norm if norm)                 (H_t, normaliser)
//   SEP_UPDATE: dst[frame] *= sum_v max(conv_v, 0) / norm                          (est *= H_t(ratio) / H_t(1))
// grid (ceil(nx / 64), ceil(ny / 32), frames for SUM / UPDATE, else images)
template <typename T>
struct SepColsParams {
    const T* tmp;      // row-pass results
    const T* taps_u;   // [V][py]
    const T* aux;      // RATIO: the measurement
    const T* norm;     // [ny][nx] (SUM: may be null)
    T* dst;
    int ny, nx, py, V;
};

template <typename T, int MODE, class Sync>
RL_HD void sep_cols_impl(const T* __restrict__ tmp, const T* __restrict__ taps_u, const T* __restrict__ aux, const T* __restrict__ norm,
                         T* __restrict__ dst, int ny, int nx, int py, int V, int t, int bx, int by, int bz, unsigned char* smem, Sync& sync) {
    T* tile = reinterpret_cast<T*>(smem);                   // [kColH + py - 1][kColW]
    const int x0 = bx * kColW, y0 = by * kColH;
    const int c = t % kColW, g = t / kColW;                 // column in the tile, row group (4 groups of 8 rows)
    const int cy = (py - 1) / 2;
    const bool multi = MODE == SEP_SUM || MODE == SEP_UPDATE;
    const int frame = bz;                                   // multi: frame; else image frame*V + view
    const int nview = multi ? V : 1;
    T acc[kColH / 4];
#pragma unroll
    for (int k = 0; k < kColH / 4; ++k) acc[k] = 0;
    for (int vw = 0; vw < nview; ++vw) {
        const int img = multi ? frame * V + vw : frame;
        const int view = multi ? vw : frame % V;
        const T* __restrict__ src = tmp + (size_t)img * ny * nx;
        if (vw > 0) sync.wg();
        // tile row i holds input row y0 + i + cy - (py - 1)
        for (int i = g; i < kColH + py - 1; i += 4) {
            const int yi = y0 + i + cy - (py - 1), x = x0 + c;
            tile[i * kColW + c] = (yi >= 0 && yi < ny && x < nx) ? src[(size_t)yi * nx + x] : (T)0;
        }
        sync.wg();
        const T* __restrict__ u = taps_u + (size_t)view * py;
#pragma unroll
        for (int k = 0; k < kColH / 4; ++k) {
            const int r = g * (kColH / 4) + k;              // output row y0 + r
            T s = 0;
            for (int a = 0; a < py; ++a) s += tile[(r + (py - 1) - a) * kColW + c] * u[a];
            acc[k] += s > (T)0 ? s : (T)0;                  // each view clamped before the sum (ref:587)
        }
    }
    const int x = x0 + c;
    if (x >= nx) return;
#pragma unroll
    for (int k = 0; k < kColH / 4; ++k) {
        const int y = y0 + g * (kColH / 4) + k;
        if (y >= ny) continue;
        const size_t o = ((size_t)frame * ny + y) * nx + x;
        const size_t pix = (size_t)y * nx + x;
        if (MODE == SEP_STORE) dst[o] = acc[k];
        else if (MODE == SEP_RATIO) dst[o] = acc[k] > (T)0 ? aux[o] / acc[k] : (T)1;   // (a prediction that is not positive: neutral pixel, conv_kernels.hpp rl_ratio)
        else if (MODE == SEP_SUM) dst[o] = norm ? acc[k] / norm[pix] : acc[k];
        else dst[o] = dst[o] * (acc[k] / norm[pix]);
    }
}
template <typename T, int MODE, class Sync>
RL_HD void sep_cols_body(const SepColsParams<T>& p, int t, int bx, int by, int bz, unsigned char* smem, Sync& sync) {
    sep_cols_impl<T, MODE>(p.tmp, p.taps_u, p.aux, p.norm, p.dst, p.ny, p.nx, p.py, p.V, t, bx, by, bz, smem, sync);
}

// ---- both passes in one kernel: the input tile + halo staged in LDS once, row stencil LDS -> LDS, column
// stencil LDS -> registers, epilogue.  Taps arrive flipped and zero padded to a multiple of 8 (correlation
// form: out[y][x] = sum_k in[..+k] f[k]), so every thread slides a 16-register window along its 8 outputs and
// an LDS value is read once per 8 multiply-adds.
//   STORE / RATIO : in = [frames] (the tile is shared by the views), dst = [frames*V]
//   SUM / UPDATE  : in = [frames*V], dst = [frames]
// sep_window8 reads base[0 .. (8 * (chunks + 1) - 1) * stride] and taps[0 .. 8 * chunks - 1].
template <typename T>
RL_HD void sep_window8(const T* __restrict__ base, int stride, const T* __restrict__ taps, int chunks, T (&acc)[8]) {
    T win[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) { win[j] = base[j * stride]; acc[j] = 0; }
    for (int c = 0; c < chunks; ++c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) win[8 + j] = base[(8 * (c + 1) + j) * stride];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const T f = taps[c * 8 + k];                    // uniform address: an LDS broadcast
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += win[k + j] * f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) win[j] = win[8 + j];
    }
}

template <typename T>
struct Sep2dParams {
    const T* in;
    const T* uf;     // [V][8 nca] flipped column taps (DIRECT: [V][px][8 nca])
    const T* vf;     // [V][8 ncb] flipped row taps (DIRECT: unused)
    const T* aux;    // RATIO: the measurement
    const T* norm;   // [ny][nx] (SUM: may be null)
    T* dst;
    int ny, nx, py, px, V;
};

// DIRECT (round 4): the PSF is NOT rank 1 -- no row pass; every output sums px column windows of the input tile, taps
// uf = [V][px][8 nca]: F[l][k] = p[py-1-k][px-1-l] (flipped both ways, zero padded along k), vf unused.  py * px multiply-adds per
// pixel, all of one sign for a non-negative PSF: the RELATIVE accuracy the FFT path cannot give a dark region.
// grid (ceil(nx / 64), ceil(ny / TH), frames), 256 threads, sep2d_lds(sizeof(T), TH, py, px, V, DIRECT) bytes of LDS
template <typename T, int MODE, int TH, bool DIRECT, class Sync>
RL_HD void sep2d_impl(const T* __restrict__ in, const T* __restrict__ uf, const T* __restrict__ vf, const T* __restrict__ aux,
                      const T* __restrict__ norm, T* __restrict__ dst, int ny, int nx, int py, int px, int V, int t, int bx, int by, int bz,
                      unsigned char* smem, Sync& sync) {
    constexpr bool multi = MODE == SEP_SUM || MODE == SEP_UPDATE;
    constexpr int NI = TH / 8 * kColW / 256;               // column-pass items (8 rows of one column) per thread
    static_assert(NI >= 1, "tile height");
    const int nca = (py + 7) / 8, ncb = (px + 7) / 8;
    const int R = TH + 8 * nca, IP = (kColW + 8 * ncb) | 1, TP = kColW + 1;   // rows staged, odd pitches
    T* tin = reinterpret_cast<T*>(smem);                    // [R][IP]  input tile, element (i, j) <-> (y0 - oy + i, x0 - ox + j)
    T* tmp = tin + (size_t)R * IP;                          // [R][TP]  row-pass results (not DIRECT)
    T* ftaps = DIRECT ? tmp : tmp + (size_t)R * TP;         // [V][8 nca] then [V][8 ncb] (DIRECT: [V][px][8 nca]): LDS broadcasts instead of scalar-load latency
    if constexpr (DIRECT) {
        for (int i = t; i < V * px * 8 * nca; i += 256) ftaps[i] = uf[i];
    } else {
        for (int i = t; i < V * 8 * nca; i += 256) ftaps[i] = uf[i];
        for (int i = t; i < V * 8 * ncb; i += 256) ftaps[V * 8 * nca + i] = vf[i];
    }
    const int oy = py - 1 - (py - 1) / 2, ox = px - 1 - (px - 1) / 2;
    const int x0 = bx * kColW, y0 = by * TH, frame = bz;
    T sum[NI][8];
#pragma unroll
    for (int n = 0; n < NI; ++n)
#pragma unroll
        for (int j = 0; j < 8; ++j) sum[n][j] = 0;
    for (int view = 0; view < V; ++view) {
        if (view > 0) sync.wg();                            // the previous view's column pass has read tmp
        if (view == 0 || multi) {
            const T* __restrict__ src = in + (size_t)(multi ? frame * V + view : frame) * ny * nx;
            for (int i = t / kColW; i < R; i += 256 / kColW) {
                const int y = y0 - oy + i;
                const bool row_ok = y >= 0 && y < ny;
                for (int j = t % kColW; j < IP; j += kColW) {
                    const int x = x0 - ox + j;
                    tin[i * IP + j] = (row_ok && x >= 0 && x < nx) ? src[(size_t)y * nx + x] : (T)0;
                }
            }
            sync.wg();
        }
        if constexpr (!DIRECT) {
            const T* fv = ftaps + V * 8 * nca + view * 8 * ncb;
            for (int w = t; w < R * (kColW / 8); w += 256) {    // lanes along rows: odd pitches keep LDS conflict free
                const int i = w % R, sgm = w / R;
                T acc[8];
                sep_window8(tin + i * IP + sgm * 8, 1, fv, ncb, acc);
#pragma unroll
                for (int j = 0; j < 8; ++j) tmp[i * TP + sgm * 8 + j] = acc[j];
            }
            sync.wg();
        } else if (view == 0) {
            sync.wg();                                          // the taps are in LDS
        }
        const T* fu = ftaps + view * (DIRECT ? px : 1) * 8 * nca;
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            const int it = t + 256 * n, c = it % kColW, g = it / kColW;
            T acc[8];
            if constexpr (DIRECT) {
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = 0;
                for (int l = 0; l < px; ++l) {                  // column x0 + c + l - ox of the tile, all its taps
                    T part[8];
                    sep_window8(tin + (g * 8) * IP + c + l, IP, fu + l * 8 * nca, nca, part);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] += part[j];
                }
            } else {
                sep_window8(tmp + (g * 8) * TP + c, TP, fu, nca, acc);
            }
            const int x = x0 + c;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const T a = acc[j] > (T)0 ? acc[j] : (T)0;  // each view clamped (ref:575,587)
                if (multi) {
                    sum[n][j] += a;
                } else {
                    const int y = y0 + g * 8 + j;
                    if (x < nx && y < ny) {
                        const size_t o = (((size_t)frame * V + view) * ny + y) * nx + x;
                        dst[o] = MODE == SEP_STORE ? a : (a > (T)0 ? aux[o] / a : (T)1);   // (neutral where the prediction is not positive: rl_ratio)
                    }
                }
            }
        }
    }
    if (multi) {
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            const int it = t + 256 * n, c = it % kColW, g = it / kColW, x = x0 + c;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int y = y0 + g * 8 + j;
                if (x >= nx || y >= ny) continue;
                const size_t pix = (size_t)y * nx + x, o = (size_t)frame * ny * nx + pix;
                if (MODE == SEP_SUM) dst[o] = norm ? sum[n][j] / norm[pix] : sum[n][j];
                else dst[o] = dst[o] * (sum[n][j] / norm[pix]);
            }
        }
    }
}
template <typename T, int MODE, int TH, bool DIRECT, class Sync>
RL_HD void sep2d_body(const Sep2dParams<T>& p, int t, int bx, int by, int bz, unsigned char* smem, Sync& sync) {
    sep2d_impl<T, MODE, TH, DIRECT>(p.in, p.uf, p.vf, p.aux, p.norm, p.dst, p.ny, p.nx, p.py, p.px, p.V, t, bx, by, bz, smem, sync);
}

// ---- launchers (sep_kernels.hip)
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
// out[img] = row stencil of in[img / in_div] with taps_v[img % V] (px taps); images = number of output images
hipError_t sep_rows(int dtype, const void* in, void* out, const void* taps_v, int images, int ny, int nx, int px, int V,
                    int in_div, hipStream_t s);
// column stencil of tmp with taps_u (py taps) + epilogue `mode`; frames_or_images: frames for SUM / UPDATE, else images
hipError_t sep_cols(int dtype, int mode, const void* tmp, const void* taps_u, const void* aux, const void* norm, void* dst,
                    int frames_or_images, int ny, int nx, int py, int V, hipStream_t s);
// Both passes in one kernel (input tile + halo in LDS).  taps_uf / taps_vf: [V][8*ceil(py/8)] / [V][8*ceil(px/8)],
// FLIPPED (f[k] = taps[n-1-k]) and zero padded (sep_taps.hpp).  STORE / RATIO: in [frames], dst [frames*V]; SUM / UPDATE: in
// [frames*V], dst [frames].  th: the tile height, the plan's (plan_options.hpp sep_th: 32, or 64 on a float plan; anything else
// is an error).  sep2d_fits: the tile fits the 160 KB of LDS at height th.
bool sep2d_fits(int dtype, int th, int py, int px, int V);
// the direct 2-D stencil for PSFs that are not rank 1 (sep2d with taps_vf == nullptr, taps_uf = [V][px][8*ceil(py/8)]:
// F[l][k] = p[py-1-k][px-1-l], zero padded along k): the input tile and the taps fit LDS
bool direct2d_fits(int dtype, int th, int py, int px, int V);
// the two-pass form (sep_rows + sep_cols) fits LDS: py up to 609 taps in f32, 289 in f64 (the plan falls back to the FFT path beyond)
bool sep_two_pass_fits(int dtype, int py, int px);
hipError_t sep2d(int dtype, int th, int mode, const void* in, const void* taps_uf, const void* taps_vf, const void* aux, const void* norm,
                 void* dst, int frames, int ny, int nx, int py, int px, int V, hipStream_t s);
#endif
}  // namespace rl
