// ctx.hpp -- internals shared by the C-ABI translation units (not installed)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rlsted.h"
#include "kernel_table.hpp"

namespace rl {
std::string& last_error();                 // thread local
int fail(int code, const std::string& msg);
bool debug_sync();                         // RLSTED_DEBUG_SYNC set: sync + check after every launch
rl_ctx* plan_ctx(rl_deconv* h);            // the context of a plan (rlsted.cpp)
}  // namespace rl

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return rl::fail(RL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));             \
    } while (0)
#define RL_TRY(expr)                \
    do {                            \
        int r_ = (expr);            \
        if (r_ != RL_OK) return r_; \
    } while (0)

using rl::fail;

namespace rl {
// host float64 values -> a device array of h.size() elements of `dtype` (twiddle tables, stencil taps)
inline int upload_as(int dtype, const std::vector<double>& h, void* dev) {
    if (dtype == RL_F64) {
        HIP_TRY(hipMemcpy(dev, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    } else {
        const std::vector<float> f(h.begin(), h.end());
        HIP_TRY(hipMemcpy(dev, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return RL_OK;
}
}  // namespace rl

struct rl_ctx {
    // grow-only device scratch for the PSF pipeline (float64 elements)
    double* psf_work = nullptr;
    size_t psf_work_elems = 0;
    int psf_workspace(size_t elems, double** out) {
        if (elems > psf_work_elems) {
            if (psf_work) (void)hipFree(psf_work);
            psf_work = nullptr;
            psf_work_elems = 0;
            HIP_TRY(hipMalloc((void**)&psf_work, elems * sizeof(double)));
            psf_work_elems = elems;
        }
        *out = psf_work;
        return RL_OK;
    }

    // rl_ring_stats, rl_ring_sector_stats (ring_api.cpp): the device ring tables, one per (ny, nx, n_rings), the sector tables,
    // one per (ny, nx, n_rings, n_sectors), and a grow-only workspace; freed with the context (rl_ctx_destroy deletes it with its
    // device current)
    struct RingTable {
        int* row_ptr = nullptr;   // [n_rings + 1]; a sector table's cell_ptr [n_rings * n_sectors + 1]
        int* bins = nullptr;      // [row_ptr[n_rings]]
    };
    struct RingCache {
        std::map<std::pair<std::pair<int, int>, int>, RingTable> tables;
        std::map<std::pair<std::pair<int, int>, std::pair<int, int>>, RingTable> sector_tables;
        void* work = nullptr;
        size_t work_bytes = 0;
        static void release(RingTable& t) {
            if (t.row_ptr) (void)hipFree(t.row_ptr);
            if (t.bins) (void)hipFree(t.bins);
        }
        ~RingCache() {
            for (auto& kv : tables) release(kv.second);
            for (auto& kv : sector_tables) release(kv.second);
            if (work) (void)hipFree(work);
        }
    } ring;

    // rl_ensemble_stats (ensemble_api.cpp): a grow-only workspace for the offset tables, the partials and the totals; freed with
    // the context
    struct EnsembleWork {
        void* work = nullptr;
        size_t work_bytes = 0;
        ~EnsembleWork() {
            if (work) (void)hipFree(work);
        }
    } ensemble;
    // rl_tile_gather, rl_tile_blend (tile_api.cpp): a grow-only workspace for the slot list / the layout tables of a call; freed
    // with the context
    EnsembleWork tile;
    // rl_ingest, rl_export (stack_api.cpp): a grow-only workspace for the per-workgroup partials of a call's statistics; freed with
    // the context
    EnsembleWork ingest;
    // rl_register_sums, rl_shift_images (register_api.cpp): a grow-only workspace for a call's offsets, taps, partials, totals
    // and the shift's float64 intermediate; freed with the context
    EnsembleWork reg;
    // rl_warp_images (register_api.cpp, in the workspace above): warp_cap, the bytes the float64 intermediates of one chunk's images
    // may take (rl_warp_chunk_bytes); warp_direct, 1 when no tile is to be staged in LDS (rl_warp_path)
    size_t warp_cap = (size_t)512 << 20;
    int warp_direct = 0;
    // rl_find_peaks (bead_api.cpp): a grow-only workspace for a call's taps, offsets, tile partials, levels, masks and candidate
    // lists; freed with the context.  beads_cap: the bytes the images in flight of one chunk may take (rl_find_peaks_chunk_bytes)
    EnsembleWork beads;
    size_t beads_cap = (size_t)256 << 20;
    // rl_repair_pixels (calib_api.cpp): a grow-only workspace for a call's defect list; freed with the context
    EnsembleWork calib;

    int device = 0;
    hipStream_t stream = nullptr;
    std::map<std::pair<int, int>, void*> tw;   // (L, dtype) -> device table
    std::map<int, bool> prepared;

    // plain table exp(-2 pi i m / L), float64 (PSF spectrum DFT)
    int plain_twiddles(int L, void** out) {
        auto key = std::make_pair(-L, (int)RL_F64);
        auto it = tw.find(key);
        if (it != tw.end()) {
            *out = it->second;
            return RL_OK;
        }
        std::vector<double> h(2 * (size_t)L);
        for (int m = 0; m < L; ++m) {
            const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)m / (long double)L;
            h[2 * m] = (double)cosl(a);
            h[2 * m + 1] = (double)sinl(a);
        }
        void* dev = nullptr;
        HIP_TRY(hipMalloc(&dev, sizeof(double) * 2 * L));
        HIP_TRY(hipMemcpy(dev, h.data(), sizeof(double) * 2 * L, hipMemcpyHostToDevice));
        tw[key] = dev;
        *out = dev;
        return RL_OK;
    }

    // per-pass twiddle table of one transform length (layout: fft_core.hpp PassTw)
    // column == true: the table of the column kernels' geometry (fft_configs.hpp ColCfgFor)
    int twiddles(const rl::KernelTable* t, int dtype, void** out, bool column = false) {
        auto key = std::make_pair(t->L + (column ? (1 << 24) : 0), dtype);
        auto it = tw.find(key);
        if (it != tw.end()) {
            *out = it->second;
            return RL_OK;
        }
        const int count = column ? t->tw_count_col[dtype] : t->tw_count;
        const size_t n = 2 * (size_t)(count > 0 ? count : 1);
        std::vector<double> h(n, 0.0);
        if (count > 0) (column ? t->fill_tw_col[dtype] : t->fill_tw)(h.data());
        void* dev = nullptr;
        HIP_TRY(hipMalloc(&dev, (dtype == RL_F64 ? sizeof(double) : sizeof(float)) * n));
        if (int r = rl::upload_as(dtype, h, dev)) {
            (void)hipFree(dev);
            return r;
        }
        tw[key] = dev;
        *out = dev;
        return RL_OK;
    }

    int prepare(const rl::KernelTable* t) {
        if (prepared[t->L]) return RL_OK;
        HIP_TRY(t->prepare());
        prepared[t->L] = true;
        return RL_OK;
    }
};

