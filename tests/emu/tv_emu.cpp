// Host emulator of the RL-TV kernels (rescan_line_sted_amd/csrc/tv_kernels.hpp): the very same thread bodies, run thread by thread and
// workgroup by workgroup.  WEIGHT: all threads stage the tile, then (the barrier) all threads form their weights; APPLY: the threads of
// a launch touch disjoint elements and meet only in the workgroup tree, which runs here step by step as the device runs it between
// barriers.  The LDS tile is poisoned before each workgroup, so that a pixel the staging forgot would show.  TEST INFRASTRUCTURE ONLY --
// built by tests/test_tv_cpu.py with g++ (-ffp-contract=off) and never loaded by the product.
#include <limits>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/tv_kernels.hpp"

using namespace rl;

namespace {

template <typename T>
TvParams<T> params(T* est, T* w, double* part, double lambda, double eps_rel, int ny, int nx, int flags) {
    TvParams<T> p{};
    p.est = est; p.w = w; p.part = part; p.lambda = lambda; p.eps_rel = eps_rel; p.ny = ny; p.nx = nx; p.flags = flags;
    p.nb = accel_blocks((size_t)ny * nx, sizeof(T));
    p.tiles_x = tv_tiles_x(nx, sizeof(T));
    return p;
}

template <typename T>
void weight(T* est, T* w, double* part, double lambda, double eps_rel, int ny, int nx, int frames) {
    const TvParams<T> p = params<T>(est, w, part, lambda, eps_rel, ny, nx, 0);
    // (16-byte aligned, as the __shared__ array of the kernel is)
    std::vector<AccelVec<T>> store((tv_lds_elems<T>() * sizeof(T) + 15) / 16);
    T* tile = reinterpret_cast<T*>(store.data());
    const int tiles = p.tiles_x * tv_tiles_y(ny);
    for (int f = 0; f < frames; ++f)
        for (int b = 0; b < tiles; ++b) {
            for (int i = 0; i < tv_lds_elems<T>(); ++i) tile[i] = std::numeric_limits<T>::quiet_NaN();
            for (int t = 0; t < kAccelThreads; ++t) tv_stage_thread<T>(p, f, b, t, tile);
            const double s = tv_mean(part + (size_t)f * p.nb, p.nb, (size_t)ny * nx);
            for (int t = 0; t < kAccelThreads; ++t) tv_weight_thread<T>(p, f, b, t, tile, tv_eps2<T>(eps_rel, s));
        }
}

template <typename T>
void apply(T* est, T* w, double* part, int ny, int nx, int frames, int flags) {
    const TvParams<T> p = params<T>(est, w, part, 0.0, 1.0, ny, nx, flags);
    std::vector<double> ss(kAccelThreads);
    for (int f = 0; f < frames; ++f)
        for (int b = 0; b < p.nb; ++b) {
            for (int t = 0; t < kAccelThreads; ++t) ss[t] = tv_apply_thread<T>(p, f, b, t);
            for (int h = kAccelThreads / 2; h > 0; h >>= 1)
                for (int t = 0; t < kAccelThreads; ++t) accel_tree_step(ss.data(), t, h);
            part[(size_t)f * p.nb + b] = ss[0];
        }
}

}  // namespace

extern "C" {
int emu_tv_blocks(size_t n, size_t esize) { return accel_blocks(n, esize); }
int emu_tv_threads() { return kAccelThreads; }
int emu_tv_tile_rows() { return kTvRows; }
int emu_tv_tile_cols(size_t esize) { return kTvVecs * (int)(16 / esize); }
void emu_tv_weight_f64(double* est, double* w, double* part, double lambda, double eps_rel, int ny, int nx, int frames) {
    weight<double>(est, w, part, lambda, eps_rel, ny, nx, frames);
}
void emu_tv_weight_f32(float* est, float* w, double* part, double lambda, double eps_rel, int ny, int nx, int frames) {
    weight<float>(est, w, part, lambda, eps_rel, ny, nx, frames);
}
void emu_tv_apply_f64(double* est, double* w, double* part, int ny, int nx, int frames, int flags) {
    apply<double>(est, w, part, ny, nx, frames, flags);
}
void emu_tv_apply_f32(float* est, float* w, double* part, int ny, int nx, int frames, int flags) {
    apply<float>(est, w, part, ny, nx, frames, flags);
}
}
