// calib_kernels.hip -- the gfx950 kernels of rl_calib_accumulate, rl_calib_finalize and rl_repair_pixels (bodies, the work split and
// the frame split: calib_kernels.hpp).  No LDS, no scratch.
//   k_calib_accumulate<TR>   a thread per 8 adjacent window pixels, grid (window workgroups, parts of the frame split); 64-bit
//                            integer atomics only where parts > 1
//   k_calib_finalize<INT>    a thread per pixel: mean and variance, float64
//   k_repair<T>              a thread per (image, listed defect), in place
#include <hip/hip_runtime.h>
#include "calib_kernels.hpp"
#include "ingest_kernels.hpp"
#include "kernel_table.hpp"

namespace rl {

template <typename TR>
__global__ __launch_bounds__(kCalibThreads) void k_calib_accumulate(CalibParams<TR> p) {
    calib_accumulate_thread<TR>(p, (int)blockIdx.x, (int)threadIdx.x, (int)blockIdx.y);
}

template <bool INTEGER>
__global__ __launch_bounds__(kCalibThreads) void k_calib_finalize(const void* sum, const void* sumsq, long long frames, size_t n_pix,
                                                                  double* mean, double* var) {
    const size_t i = (size_t)blockIdx.x * kCalibThreads + threadIdx.x;
    if (i >= n_pix) return;
    if (INTEGER) {
        calib_finalize_int((const long long*)sum, (const unsigned long long*)sumsq, frames, i, mean, var);
    } else {
        calib_finalize_f32((const double*)sum, (const double*)sumsq, frames, i, mean, var);
    }
}

template <typename T>
__global__ __launch_bounds__(kCalibThreads) void k_repair(T* img, size_t n_pix, int nx, const RepairEntry* list, unsigned n_list, size_t total) {
    const size_t id = (size_t)blockIdx.x * kCalibThreads + threadIdx.x;
    if (id >= total) return;
    const size_t image = id / n_list;
    repair_thread<T>(img + image * n_pix, nx, list[id % n_list]);
}

namespace {
constexpr size_t kMaxGridX = 0x7fffffffull;

template <typename TR>
hipError_t accumulate_t(const void* raw, void* sum, void* sumsq, int src_ny, int src_pitch, int y0, int x0, int ny, int nx, int n_frames,
                        hipStream_t s) {
    const int groups = calib_groups(calib_vectors(ny, nx));
    const int parts = calib_parts(groups, n_frames, CalibAcc<TR>::integer);
    const CalibParams<TR> p = calib_params<TR>(raw, sum, sumsq, src_ny, src_pitch, y0, x0, ny, nx, n_frames, parts);
    hipLaunchKernelGGL((k_calib_accumulate<TR>), dim3((unsigned)groups, (unsigned)parts), dim3(kCalibThreads), 0, s, p);
    return hipGetLastError();
}
}  // namespace

hipError_t calib_accumulate(int raw_dtype, const void* raw, void* sum, void* sumsq, int src_ny, int src_pitch, int y0, int x0, int ny,
                            int nx, int n_frames, hipStream_t s) {
    if (n_frames <= 0) return hipSuccess;
    if (calib_vectors(ny, nx) > kMaxGridX * kCalibThreads) return hipErrorInvalidValue;
    switch (raw_dtype) {
        case RAW_U8: return accumulate_t<uint8_t>(raw, sum, sumsq, src_ny, src_pitch, y0, x0, ny, nx, n_frames, s);
        case RAW_U16: return accumulate_t<uint16_t>(raw, sum, sumsq, src_ny, src_pitch, y0, x0, ny, nx, n_frames, s);
        case RAW_I16: return accumulate_t<int16_t>(raw, sum, sumsq, src_ny, src_pitch, y0, x0, ny, nx, n_frames, s);
        case RAW_F32: return accumulate_t<float>(raw, sum, sumsq, src_ny, src_pitch, y0, x0, ny, nx, n_frames, s);
    }
    return hipErrorInvalidValue;
}

hipError_t calib_finalize(int raw_dtype, const void* sum, const void* sumsq, long long frames, size_t n_pix, double* mean, double* var,
                          hipStream_t s) {
    const size_t blocks = (n_pix + kCalibThreads - 1) / kCalibThreads;
    if (blocks == 0 || blocks > kMaxGridX) return hipErrorInvalidValue;
    if (raw_dtype == RAW_F32) {
        hipLaunchKernelGGL(k_calib_finalize<false>, dim3((unsigned)blocks), dim3(kCalibThreads), 0, s, sum, sumsq, frames, n_pix, mean, var);
    } else {
        hipLaunchKernelGGL(k_calib_finalize<true>, dim3((unsigned)blocks), dim3(kCalibThreads), 0, s, sum, sumsq, frames, n_pix, mean, var);
    }
    return hipGetLastError();
}

hipError_t repair(int dtype, void* img, int n_images, size_t n_pix, int nx, const RepairEntry* list, int n_list, hipStream_t s) {
    if (n_images <= 0 || n_list <= 0) return hipSuccess;
    const size_t total = (size_t)n_images * (size_t)n_list, blocks = (total + kCalibThreads - 1) / kCalibThreads;
    if (blocks > kMaxGridX) return hipErrorInvalidValue;
    if (dtype == DT_F32) {
        hipLaunchKernelGGL(k_repair<float>, dim3((unsigned)blocks), dim3(kCalibThreads), 0, s, (float*)img, n_pix, nx, list, (unsigned)n_list, total);
    } else {
        hipLaunchKernelGGL(k_repair<double>, dim3((unsigned)blocks), dim3(kCalibThreads), 0, s, (double*)img, n_pix, nx, list, (unsigned)n_list, total);
    }
    return hipGetLastError();
}

}  // namespace rl
