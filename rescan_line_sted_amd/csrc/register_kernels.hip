// register_kernels.hip -- the gfx950 kernels of rl_register_sums and rl_shift_images (bodies, the work split, the LDS layout and the
// order of every sum: register_kernels.hpp).
//   k_register_sums<TA, TB>          a workgroup per (pair, band, pass): the band's column blocks through LDS, a displacement per lane
//   k_register_totals                the strips' partials -> one row of sums per pair, in increasing order
//   k_shift_pass<TS, TD, AXIS, FINAL> one 64-tap (or 1- / 2-tap) mirror FIR along an axis, a 32 x 64 tile per workgroup through LDS
//   k_shift_totals                   the workgroups' statistics -> raised, sum per image
// No atomics anywhere.
#include <hip/hip_runtime.h>
#include "register_kernels.hpp"
#include "kernel_table.hpp"

namespace rl {

template <typename TA, typename TB>
__global__ __launch_bounds__(kRegThreads) void k_register_sums(RegSumParams<TA, TB> p) {
    extern __shared__ double reg_lds[];
    const RegGeom& g = p.g;
    const int t = threadIdx.x;
    const int pass = (int)(blockIdx.x % (unsigned)g.passes);
    const int band = (int)((blockIdx.x / (unsigned)g.passes) % (unsigned)g.bands);
    const int pair = (int)(blockIdx.x / ((unsigned)g.passes * (unsigned)g.bands));
    double acc[kRegFields] = {0.0, 0.0, 0.0}, row[2] = {0.0, 0.0};
    for (int tile = 0; tile < g.ntx; ++tile) {
        reg_stage<TA, TB>(p, pair, band, tile, t, reg_lds);
        __syncthreads();
        reg_walk(g, band, tile, pass, t, reg_lds, acc, row);
        __syncthreads();
    }
    reg_store(g, p.part, pair, band, pass, t, acc, row);
}

// one thread per (pair, value)
__global__ __launch_bounds__(kRegThreads) void k_register_totals(const double* part, double* tot, RegGeom g, size_t values) {
    const size_t id = (size_t)blockIdx.x * kRegThreads + threadIdx.x;
    if (id >= values) return;
    const int per = g.nd * kRegFields + 2;
    const size_t pair = id / (unsigned)per;
    tot[id] = reg_total(g, part + pair * reg_part_doubles(g), (int)(id % (unsigned)per));
}

template <typename TS, typename TD, int AXIS, bool FINAL>
__global__ __launch_bounds__(kRegThreads) void k_shift_pass(ShiftParams<TS, TD> p) {
    __shared__ double lds[kShiftLds];
    __shared__ double sm[kShiftFields][kRegThreads];
    const int t = threadIdx.x;
    const unsigned nb = (unsigned)p.nby * (unsigned)p.nbx;
    const size_t i = blockIdx.x / nb;
    const int b = (int)(blockIdx.x % nb), by = b / p.nbx, bx = b % p.nbx;
    shift_stage<TS, TD, AXIS>(p, i, by, bx, t, lds);
    __syncthreads();
    double sums[kShiftFields];
    shift_compute<TS, TD, AXIS, FINAL>(p, i, by, bx, t, lds, sums);
    if (!FINAL || !p.part) return;   // (uniform)
    for (int f = 0; f < kShiftFields; ++f) sm[f][t] = sums[f];
    __syncthreads();
    for (int h = kRegThreads / 2; h > 0; h >>= 1) {
        for (int f = 0; f < kShiftFields; ++f) accel_tree_step(sm[f], t, h);
        __syncthreads();
    }
    if (t < kShiftFields) p.part[(size_t)blockIdx.x * kShiftFields + t] = sm[t][0];
}

// one thread per (image, field)
__global__ __launch_bounds__(kRegThreads) void k_shift_totals(const double* part, double* stats, int nb, size_t values) {
    const size_t id = (size_t)blockIdx.x * kRegThreads + threadIdx.x;
    if (id >= values) return;
    const size_t img = id / kShiftFields;
    stats[id] = ingest_total(part + img * (size_t)nb * kShiftFields, nb, kShiftFields, (int)(id % kShiftFields));
}

namespace {
constexpr size_t kMaxGrid = 0x7fffffffull;

template <typename TA, typename TB>
hipError_t sums_t(const RegSumArgs& a, hipStream_t s) {
    const RegGeom& g = a.g;
    const size_t blocks = (size_t)a.pairs * g.bands * g.passes;
    const size_t lds = reg_lds_doubles(g) * sizeof(double);
    if (blocks > kMaxGrid || lds > 65536) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_register_sums<TA, TB>), dim3((unsigned)blocks), dim3(kRegThreads), lds, s, reg_sum_params<TA, TB>(a));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t values = (size_t)a.pairs * (g.nd * kRegFields + 2), tb = (values + kRegThreads - 1) / kRegThreads;
    if (tb > kMaxGrid) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_register_totals, dim3((unsigned)tb), dim3(kRegThreads), 0, s, (const double*)a.part, a.tot, g, values);
    return hipGetLastError();
}

template <typename TS, typename TD, int AXIS, bool FINAL>
hipError_t pass_t(const ShiftArgs& a, hipStream_t s) {
    const ShiftParams<TS, TD> p = shift_params<TS, TD>(a);
    const size_t blocks = (size_t)a.n * p.nby * p.nbx;
    if (blocks > kMaxGrid) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_shift_pass<TS, TD, AXIS, FINAL>), dim3((unsigned)blocks), dim3(kRegThreads), 0, s, p);
    return hipGetLastError();
}
}  // namespace

hipError_t register_sums(int a_dtype, int b_dtype, const RegSumArgs& a, hipStream_t s) {
    if (a.pairs <= 0) return hipSuccess;
    if (a_dtype == DT_F32) return b_dtype == DT_F32 ? sums_t<float, float>(a, s) : sums_t<float, double>(a, s);
    return b_dtype == DT_F32 ? sums_t<double, float>(a, s) : sums_t<double, double>(a, s);
}

hipError_t shift_images(int src_dtype, int dst_dtype, const ShiftArgs& a, double* tmp, double* stats, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (stats && !a.part) return hipErrorInvalidValue;
    ShiftArgs x = a;            // along x into the workspace
    x.dst = tmp;
    x.part = nullptr;
    hipError_t e = src_dtype == DT_F32 ? pass_t<float, double, 1, false>(x, s) : pass_t<double, double, 1, false>(x, s);
    if (e != hipSuccess) return e;
    ShiftArgs y = a;            // along y into the destination
    y.src = tmp;
    if (!stats) y.part = nullptr;
    e = dst_dtype == DT_F32 ? pass_t<double, float, 0, true>(y, s) : pass_t<double, double, 0, true>(y, s);
    if (e != hipSuccess || !stats) return e;
    const int nb = shift_blocks_y(a.ny) * shift_blocks_x(a.nx);
    const size_t values = (size_t)a.n * kShiftFields, tb = (values + kRegThreads - 1) / kRegThreads;
    hipLaunchKernelGGL(k_shift_totals, dim3((unsigned)tb), dim3(kRegThreads), 0, s, (const double*)a.part, stats, nb, values);
    return hipGetLastError();
}

}  // namespace rl
