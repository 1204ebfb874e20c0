// ingest_kernels.hip -- the gfx950 kernels of rl_ingest and rl_export (bodies, the work split and the order of every sum:
// ingest_kernels.hpp).  Streaming kernels, one workgroup of four waves per run of an image's vectors, a one-dimensional grid of
// images * nb workgroups sized by the pixels; LDS for the statistics' tree alone, no atomics.
//   k_ingest<TR, TD>    raw sensor frames -> the frames of a plan's measurement buffer (dark, gain, window, view order; fillers: ones)
//   k_export<TE, TO>    estimates, scaled -> f32 / f64 / u16
//   k_ingest_totals     the workgroups' partials -> one row of statistics per image
#include <hip/hip_runtime.h>
#include "ingest_kernels.hpp"
#include "kernel_table.hpp"

namespace rl {

// the workgroup's tree over its threads' FIELDS sums -> part[(img * nb + b)][FIELDS]
template <int FIELDS>
__device__ __forceinline__ void ingest_tree(double (*sm)[kIngestThreads], const double* sums, double* part, int t) {
    for (int f = 0; f < FIELDS; ++f) sm[f][t] = sums[f];
    __syncthreads();
    for (int h = kIngestThreads / 2; h > 0; h >>= 1) {
        for (int f = 0; f < FIELDS; ++f) accel_tree_step(sm[f], t, h);
        __syncthreads();
    }
    if (t < FIELDS) part[t] = sm[t][0];
}

template <typename TR, typename TD>
__global__ __launch_bounds__(kIngestThreads) void k_ingest(IngestParams<TR, TD> p) {
    __shared__ double sm[kIngestFields][kIngestThreads];
    const int t = threadIdx.x;
    const size_t img = blockIdx.x / (unsigned)p.nb;
    const int b = (int)(blockIdx.x % (unsigned)p.nb);
    double sums[kIngestFields];
    ingest_thread<TR, TD>(p, img, b, t, sums);
    if (!p.part) return;   // (uniform) no statistics asked for
    ingest_tree<kIngestFields>(sm, sums, p.part + (size_t)blockIdx.x * kIngestFields, t);
}

template <typename TE, typename TO>
__global__ __launch_bounds__(kIngestThreads) void k_export(ExportParams<TE, TO> p) {
    __shared__ double sm[kExportFields][kIngestThreads];
    const int t = threadIdx.x;
    const size_t img = blockIdx.x / (unsigned)p.nb;
    const int b = (int)(blockIdx.x % (unsigned)p.nb);
    double sums[kExportFields];
    export_thread<TE, TO>(p, img, b, t, sums);
    if (!p.part) return;
    ingest_tree<kExportFields>(sm, sums, p.part + (size_t)blockIdx.x * kExportFields, t);
}

// one thread per (image, field)
__global__ __launch_bounds__(kIngestThreads) void k_ingest_totals(const double* part, double* stats, int nb, int fields, size_t values) {
    const size_t id = (size_t)blockIdx.x * kIngestThreads + threadIdx.x;
    if (id >= values) return;
    const size_t img = id / (unsigned)fields;
    stats[id] = ingest_total(part + img * (size_t)nb * fields, nb, fields, (int)(id % (unsigned)fields));
}

namespace {
constexpr size_t kMaxGrid = 0x7fffffffull;   // workgroups of a one-dimensional grid

hipError_t totals(const double* part, double* stats, int nb, int fields, size_t images, hipStream_t s) {
    const size_t values = images * fields, blocks = (values + kIngestThreads - 1) / kIngestThreads;
    if (blocks > kMaxGrid) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ingest_totals, dim3((unsigned)blocks), dim3(kIngestThreads), 0, s, part, stats, nb, fields, values);
    return hipGetLastError();
}

template <typename TR, typename TD>
hipError_t ingest_t(const IngestArgs& a, hipStream_t s) {
    const int nb = ingest_blocks(ingest_vectors(a.ny, a.nx));
    IngestArgs b = a;
    if (!a.stats) b.part = nullptr;
    const IngestParams<TR, TD> p = ingest_params<TR, TD>(b, nb);
    const size_t images = (size_t)a.n_slots * a.V, blocks = images * nb;
    if (blocks > kMaxGrid) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_ingest<TR, TD>), dim3((unsigned)blocks), dim3(kIngestThreads), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !p.part) return e;
    return totals(p.part, a.stats, nb, kIngestFields, images, s);
}

template <typename TR>
hipError_t ingest_r(int dst_dtype, const IngestArgs& a, hipStream_t s) {
    return dst_dtype == DT_F32 ? ingest_t<TR, float>(a, s) : ingest_t<TR, double>(a, s);
}

template <typename TE, typename TO>
hipError_t export_t(const ExportArgs& a, hipStream_t s) {
    const int nb = ingest_blocks(export_vectors(a.n_pix));
    ExportArgs b = a;
    if (!a.stats) b.part = nullptr;
    const ExportParams<TE, TO> p = export_params<TE, TO>(b, nb);
    const size_t blocks = (size_t)a.n * nb;
    if (blocks > kMaxGrid) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_export<TE, TO>), dim3((unsigned)blocks), dim3(kIngestThreads), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !p.part) return e;
    return totals(p.part, a.stats, nb, kExportFields, (size_t)a.n, s);
}

template <typename TE>
hipError_t export_e(int out_dtype, const ExportArgs& a, hipStream_t s) {
    switch (out_dtype) {
        case OUT_F32: return export_t<TE, float>(a, s);
        case OUT_F64: return export_t<TE, double>(a, s);
        case OUT_U16: return export_t<TE, uint16_t>(a, s);
    }
    return hipErrorInvalidValue;
}
}  // namespace

hipError_t ingest(int raw_dtype, int dst_dtype, const IngestArgs& a, hipStream_t s) {
    if (a.n_slots <= 0) return hipSuccess;
    if (a.stats && !a.part) return hipErrorInvalidValue;
    switch (raw_dtype) {
        case RAW_U8: return ingest_r<uint8_t>(dst_dtype, a, s);
        case RAW_U16: return ingest_r<uint16_t>(dst_dtype, a, s);
        case RAW_I16: return ingest_r<int16_t>(dst_dtype, a, s);
        case RAW_F32: return ingest_r<float>(dst_dtype, a, s);
    }
    return hipErrorInvalidValue;
}

hipError_t export_estimates(int est_dtype, int out_dtype, const ExportArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.n_pix == 0) return hipSuccess;
    if (a.stats && !a.part) return hipErrorInvalidValue;
    return est_dtype == DT_F32 ? export_e<float>(out_dtype, a, s) : export_e<double>(out_dtype, a, s);
}

}  // namespace rl
