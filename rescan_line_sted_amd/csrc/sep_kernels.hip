// sep_kernels.hip -- direct separable stencils for rank-1 PSFs (BASELINE north
// star: "direct separable stencils with LDS-staged tiles or FFT... chosen per kernel size").
//
// A rank-1 PSF p[a][b] = u[a] v[b] (the 0 / 90 degree line PSFs are: they are rot90s of the blurred line,
// line_sted_figure_2.py:266-269) turns the zero padded 'same' convolution of H / H_t (line_sted_tools.py:
// 567-594) into a row stencil with v followed by a column stencil with u: (py + px) multiply-adds per pixel
// instead of four FFT passes.  That wins for SMALL kernels only -- at the figure-2 size (107 taps a side) the
// FFT path is 3x faster -- so the plan picks this path when every view is rank 1 and py + px <= a threshold
// (rlsted.cpp).  Same semantics as the FFT path: out[i][j] = sum_ab x[i + cy - a][j + cx - b] p[a][b],
// cy = (py-1)/2, cx = (px-1)/2, zero outside the image, each view's result clamped at 0 (ref:575,587).
//
// Row pass: one workgroup = 256 outputs of one row, the row segment + halo staged in LDS.
// Column pass: one workgroup = 64 columns x 32 rows of outputs, the (32 + py - 1) x 64 tile of row-pass
// results staged in LDS; the Richardson-Lucy pointwise steps are its epilogues (ref:520-531).
#include <hip/hip_runtime.h>

#include <mutex>
#include <set>

#include "sep_kernels.hpp"

namespace rl {
namespace {

struct SepSync {
    __device__ __forceinline__ void wg() const { __syncthreads(); }
};

// the bodies are in sep_kernels.hpp (sep_rows_body, sep_cols_body, sep2d_body): the host emulator of the CPU tests runs them too
template <typename T>
__global__ void __launch_bounds__(kRowSeg) k_sep_rows(const T* __restrict__ in, T* __restrict__ out, const T* __restrict__ taps_v,
                                                      int ny, int nx, int px, int V, int in_div) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    SepSync sync;
    sep_rows_body<T>(SepRowsParams<T>{in, out, taps_v, ny, nx, px, V, in_div}, threadIdx.x, blockIdx.x, blockIdx.y, blockIdx.z, smem, sync);
}

template <typename T, int MODE>
__global__ void __launch_bounds__(256) k_sep_cols(const T* __restrict__ tmp, const T* __restrict__ taps_u, const T* __restrict__ aux,
                                                  const T* __restrict__ norm, T* __restrict__ dst, int ny, int nx, int py, int V) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    SepSync sync;
    sep_cols_body<T, MODE>(SepColsParams<T>{tmp, taps_u, aux, norm, dst, ny, nx, py, V}, threadIdx.x, blockIdx.x, blockIdx.y, blockIdx.z, smem, sync);
}

template <typename T, int MODE, int TH, bool DIRECT = false>
__global__ void __launch_bounds__(256) k_sep2d(const T* __restrict__ in, const T* __restrict__ uf, const T* __restrict__ vf,
                                               const T* __restrict__ aux, const T* __restrict__ norm, T* __restrict__ dst, int ny, int nx,
                                               int py, int px, int V) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    SepSync sync;
    sep2d_body<T, MODE, TH, DIRECT>(Sep2dParams<T>{in, uf, vf, aux, norm, dst, ny, nx, py, px, V}, threadIdx.x, blockIdx.x, blockIdx.y, blockIdx.z,
                                    smem, sync);
}

template <typename T, int MODE, int TH, bool DIRECT = false>
hipError_t sep2d_launch(const void* in, const void* uf, const void* vf, const void* aux, const void* norm, void* dst, int frames,
                        int ny, int nx, int py, int px, int V, hipStream_t s) {
    static unsigned long long allowed_devices = 0;   // the attribute is per device: one bit per device id
    const size_t lds = sep2d_lds(sizeof(T), TH, py, px, V, DIRECT);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !(allowed_devices >> dev & 1ull)) {
        e = hipFuncSetAttribute((const void*)k_sep2d<T, MODE, TH, DIRECT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSep2dMaxLds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) allowed_devices |= 1ull << dev;
    }
    const dim3 grid((unsigned)((nx + kColW - 1) / kColW), (unsigned)((ny + TH - 1) / TH), (unsigned)frames);
    k_sep2d<T, MODE, TH, DIRECT><<<grid, 256, lds, s>>>((const T*)in, (const T*)uf, (const T*)vf, (const T*)aux, (const T*)norm, (T*)dst, ny, nx, py, px, V);
    return hipGetLastError();
}
template <typename T, int TH, bool DIRECT = false>
hipError_t sep2d_t(int mode, const void* in, const void* uf, const void* vf, const void* aux, const void* norm, void* dst, int frames,
                   int ny, int nx, int py, int px, int V, hipStream_t s) {
    switch (mode) {
        case SEP_STORE: return sep2d_launch<T, SEP_STORE, TH, DIRECT>(in, uf, vf, aux, norm, dst, frames, ny, nx, py, px, V, s);
        case SEP_RATIO: return sep2d_launch<T, SEP_RATIO, TH, DIRECT>(in, uf, vf, aux, norm, dst, frames, ny, nx, py, px, V, s);
        case SEP_SUM: return sep2d_launch<T, SEP_SUM, TH, DIRECT>(in, uf, vf, aux, norm, dst, frames, ny, nx, py, px, V, s);
        case SEP_UPDATE: return sep2d_launch<T, SEP_UPDATE, TH, DIRECT>(in, uf, vf, aux, norm, dst, frames, ny, nx, py, px, V, s);
        default: return hipErrorInvalidValue;
    }
}

template <typename T>
hipError_t rows_t(const void* in, void* out, const void* v, int images, int ny, int nx, int px, int V, int in_div, hipStream_t s) {
    const dim3 grid((unsigned)((nx + kRowSeg - 1) / kRowSeg), (unsigned)ny, (unsigned)images);
    k_sep_rows<T><<<grid, kRowSeg, sep_rows_lds(sizeof(T), px), s>>>((const T*)in, (T*)out, (const T*)v, ny, nx, px, V, in_div);
    return hipGetLastError();
}
template <typename T>
hipError_t cols_t(int mode, const void* tmp, const void* u, const void* aux, const void* norm, void* dst, int frames_or_images,
                  int ny, int nx, int py, int V, hipStream_t s) {
    const dim3 grid((unsigned)((nx + kColW - 1) / kColW), (unsigned)((ny + kColH - 1) / kColH), (unsigned)frames_or_images);
    const size_t lds = sep_cols_lds(sizeof(T), py);
    if (lds > kSepMaxLds) return hipErrorInvalidValue;   // (the plan does not choose the stencils for such a PSF: sep_cols_fits)
    if (lds > 65536) {   // above the default dynamic-LDS limit: raise it, once per kernel AND DEVICE (the attribute belongs to the
                         // device's code object: a process-wide flag would leave a second GPU without it; a failure is not cached)
        static std::mutex mu;
        static std::set<int> raised;
        int dev = -1;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(mu);
        if (!raised.count(dev)) {
            e = hipFuncSetAttribute((const void*)k_sep_cols<T, SEP_STORE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSepMaxLds);
            if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_sep_cols<T, SEP_RATIO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSepMaxLds);
            if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_sep_cols<T, SEP_SUM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSepMaxLds);
            if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_sep_cols<T, SEP_UPDATE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSepMaxLds);
            if (e != hipSuccess) return e;
            raised.insert(dev);
        }
    }
    switch (mode) {
        case SEP_STORE: k_sep_cols<T, SEP_STORE><<<grid, 256, lds, s>>>((const T*)tmp, (const T*)u, (const T*)aux, (const T*)norm, (T*)dst, ny, nx, py, V); break;
        case SEP_RATIO: k_sep_cols<T, SEP_RATIO><<<grid, 256, lds, s>>>((const T*)tmp, (const T*)u, (const T*)aux, (const T*)norm, (T*)dst, ny, nx, py, V); break;
        case SEP_SUM: k_sep_cols<T, SEP_SUM><<<grid, 256, lds, s>>>((const T*)tmp, (const T*)u, (const T*)aux, (const T*)norm, (T*)dst, ny, nx, py, V); break;
        case SEP_UPDATE: k_sep_cols<T, SEP_UPDATE><<<grid, 256, lds, s>>>((const T*)tmp, (const T*)u, (const T*)aux, (const T*)norm, (T*)dst, ny, nx, py, V); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t sep_rows(int dtype, const void* in, void* out, const void* taps_v, int images, int ny, int nx, int px, int V,
                    int in_div, hipStream_t s) {
    if (images < 1) return hipSuccess;
    if (images > 65535) return hipErrorInvalidValue;   // grid.z
    return dtype == DT_F32 ? rows_t<float>(in, out, taps_v, images, ny, nx, px, V, in_div, s)
                           : rows_t<double>(in, out, taps_v, images, ny, nx, px, V, in_div, s);
}
hipError_t sep_cols(int dtype, int mode, const void* tmp, const void* taps_u, const void* aux, const void* norm, void* dst,
                    int frames_or_images, int ny, int nx, int py, int V, hipStream_t s) {
    if (frames_or_images < 1) return hipSuccess;
    if (frames_or_images > 65535) return hipErrorInvalidValue;
    return dtype == DT_F32 ? cols_t<float>(mode, tmp, taps_u, aux, norm, dst, frames_or_images, ny, nx, py, V, s)
                           : cols_t<double>(mode, tmp, taps_u, aux, norm, dst, frames_or_images, ny, nx, py, V, s);
}


// th: the tile height of the one-kernel form, the plan's (plan_options.hpp sep_th): 32 or 64 for float, 32 for double
static size_t sep_esize(int dtype) { return dtype == DT_F32 ? 4 : 8; }
bool sep2d_fits(int dtype, int th, int py, int px, int V) { return sep2d_fits_tile(sep_esize(dtype), th, py, px, V); }
bool direct2d_fits(int dtype, int th, int py, int px, int V) { return direct2d_fits_tile(sep_esize(dtype), th, py, px, V); }
bool sep_two_pass_fits(int dtype, int py, int px) { return sep_two_pass_fits_esize(sep_esize(dtype), py, px); }
hipError_t sep2d(int dtype, int th, int mode, const void* in, const void* taps_uf, const void* taps_vf, const void* aux, const void* norm,
                 void* dst, int frames, int ny, int nx, int py, int px, int V, hipStream_t s) {
    if (frames < 1) return hipSuccess;
    if (th != 32 && !(th == 64 && dtype == DT_F32)) return hipErrorInvalidValue;
    if (taps_vf == nullptr) {   // the direct 2-D stencil: taps_uf = [V][px][8 * ceil(py / 8)]
        if (frames > 65535 || !direct2d_fits(dtype, th, py, px, V)) return hipErrorInvalidValue;
        if (dtype != DT_F32) return sep2d_t<double, 32, true>(mode, in, taps_uf, nullptr, aux, norm, dst, frames, ny, nx, py, px, V, s);
        return th == 64 ? sep2d_t<float, 64, true>(mode, in, taps_uf, nullptr, aux, norm, dst, frames, ny, nx, py, px, V, s)
                        : sep2d_t<float, 32, true>(mode, in, taps_uf, nullptr, aux, norm, dst, frames, ny, nx, py, px, V, s);
    }
    if (frames > 65535 || !sep2d_fits(dtype, th, py, px, V)) return hipErrorInvalidValue;
    if (dtype != DT_F32) return sep2d_t<double, 32>(mode, in, taps_uf, taps_vf, aux, norm, dst, frames, ny, nx, py, px, V, s);
    return th == 64 ? sep2d_t<float, 64>(mode, in, taps_uf, taps_vf, aux, norm, dst, frames, ny, nx, py, px, V, s)
                    : sep2d_t<float, 32>(mode, in, taps_uf, taps_vf, aux, norm, dst, frames, ny, nx, py, px, V, s);
}

}  // namespace rl
