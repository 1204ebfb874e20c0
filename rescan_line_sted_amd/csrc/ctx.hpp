// ctx.hpp -- internals shared by the C-ABI translation units (not installed)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rlsted.h"
#include "kernel_table.hpp"
#include "work_layout.hpp"

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
// ---- what every C-ABI call checks and sizes the same way ----
inline bool dtype_ok(int d) { return d == RL_F32 || d == RL_F64; }
inline size_t dtype_size(int d) { return d == RL_F32 ? sizeof(float) : sizeof(double); }
inline bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return (const char*)a < (const char*)b + b_bytes && (const char*)b < (const char*)a + a_bytes;
}
// the items of one chunk: as many of the n as stay under the cap, at least one (a larger single item runs alone)
inline size_t chunk_under(size_t cap_bytes, size_t per_item_bytes, size_t n) {
    return std::min(n, std::max<size_t>(1, cap_bytes / per_item_bytes));
}
// the image offsets of n pairs (the register and affine calls)
inline int check_pair_offsets(const int64_t* a, const int64_t* b, int n) {
    for (int i = 0; i < n; ++i)
        if (a[i] < 0 || b[i] < 0) return fail(RL_ERR_INVALID, "pair " + std::to_string(i) + ": negative offset");
    return RL_OK;
}
// the pixels a margin of M leaves inside an image (the register and affine calls)
inline int check_interior(int ny, int nx, int M) {
    if (ny < 1 || nx < 1 || (long long)ny - 2LL * M < 8 || (long long)nx - 2LL * M < 8)
        return fail(RL_ERR_INVALID, "the interior must be at least 8 x 8 pixels: ny - 2 M >= 8 and nx - 2 M >= 8");
    return RL_OK;
}

struct DevBuf {   // scoped device allocation
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int get(size_t bytes) {
        HIP_TRY(hipMalloc(&p, bytes ? bytes : 8));
        return RL_OK;
    }
};

// Grow-only device scratch of one family of calls, freed with the context.  A call declares its regions in a WorkLayout
// (work_layout.hpp), reserves the layout's bytes() here and takes every pointer from the regions' at(base).
struct Workspace {
    void* ptr = nullptr;
    size_t bytes = 0;
    int reserve(hipStream_t stream, size_t need, char** out) {
        if (need > bytes) {
            HIP_TRY(hipStreamSynchronize(stream));   // (a call still queued may use the present block)
            if (ptr) (void)hipFree(ptr);
            ptr = nullptr;
            bytes = 0;
            HIP_TRY(hipMalloc(&ptr, need));
            bytes = need;
        }
        *out = (char*)ptr;
        return RL_OK;
    }
    ~Workspace() { if (ptr) (void)hipFree(ptr); }
};
}  // namespace rl

struct rl_ctx {
    // the PSF pipeline, the figure scans and the f32 transfers of rl_device_upload / rl_device_download: float64 elements, carved
    // by the callers in double offsets
    rl::Workspace psf;
    int psf_workspace(size_t elems, double** out) {
        char* p = nullptr;
        RL_TRY(psf.reserve(stream, elems * sizeof(double), &p));
        *out = (double*)p;
        return RL_OK;
    }

    // rl_ring_stats, rl_ring_sector_stats (ring_api.cpp): the device ring tables, one per (ny, nx, n_rings), the sector tables,
    // one per (ny, nx, n_rings, n_sectors), and the workspace of a call: its offsets and scales, the results and the spectra of
    // the pairs in flight; freed with the context (rl_ctx_destroy deletes it with its device current)
    struct RingTable {
        int* row_ptr = nullptr;   // [n_rings + 1]; a sector table's cell_ptr [n_rings * n_sectors + 1]
        int* bins = nullptr;      // [row_ptr[n_rings]]
    };
    struct RingCache {
        std::map<std::pair<std::pair<int, int>, int>, RingTable> tables;
        std::map<std::pair<std::pair<int, int>, std::pair<int, int>>, RingTable> sector_tables;
        rl::Workspace work;
        static void release(RingTable& t) {
            if (t.row_ptr) (void)hipFree(t.row_ptr);
            if (t.bins) (void)hipFree(t.bins);
        }
        ~RingCache() {
            for (auto& kv : tables) release(kv.second);
            for (auto& kv : sector_tables) release(kv.second);
        }
    } ring;

    // rl_ensemble_stats (ensemble_api.cpp): the offset tables, the partials and the totals
    rl::Workspace ensemble;
    // rl_tile_gather, rl_tile_blend (tile_api.cpp): the slot list / the layout tables of a call
    rl::Workspace tile;
    // rl_ingest, rl_export (stack_api.cpp): the per-workgroup partials of a call's statistics
    rl::Workspace ingest;
    // rl_register_sums, rl_shift_images and the other calls of register_api.cpp: a call's offsets, taps, partials, totals and the
    // shift's float64 intermediate
    rl::Workspace reg;
    // rl_warp_images (register_api.cpp, in the workspace above): warp_cap, the bytes the float64 intermediates of one chunk's images
    // may take (rl_warp_chunk_bytes); warp_direct, 1 when no tile is to be staged in LDS (rl_warp_path)
    size_t warp_cap = (size_t)512 << 20;
    int warp_direct = 0;
    // rl_find_peaks (bead_api.cpp): a call's taps, offsets, tile partials, levels, masks and candidate lists.  beads_cap: the bytes
    // the images in flight of one chunk may take (rl_find_peaks_chunk_bytes)
    rl::Workspace beads;
    size_t beads_cap = (size_t)256 << 20;
    // rl_repair_pixels (calib_api.cpp): a call's defect list
    rl::Workspace calib;
    // the other chunked calls' caps (rl_chunk_bytes).  reg_sum_cap: the partials of the pairs in flight of rl_register_sums,
    // rl_register_estimate and rl_affine_sums; shift_cap: the float64 intermediates of the images in flight of rl_shift_images and
    // the refine passes; xcorr_cap: the spectra and kept rows of rl_register_xcorr's pairs in flight; ring_cap: T and F of the
    // pairs in flight of the ring statistics, and their sector results; fig3_cap: one image stack of rl_fig3_scan's positions in
    // flight.  A larger single item runs alone.
    size_t reg_sum_cap = (size_t)256 << 20;
    size_t shift_cap = (size_t)512 << 20;
    size_t xcorr_cap = (size_t)32 << 20;
    size_t ring_cap = (size_t)256 << 20;
    size_t fig3_cap = ((size_t)64 << 20) * sizeof(double);
    // the cap of RL_CHUNK_* `which`, or nullptr
    size_t* chunk_cap(int which) {
        switch (which) {
            case RL_CHUNK_REGISTER_SUMS: return &reg_sum_cap;
            case RL_CHUNK_SHIFT: return &shift_cap;
            case RL_CHUNK_XCORR: return &xcorr_cap;
            case RL_CHUNK_RING: return &ring_cap;
            case RL_CHUNK_FIG3: return &fig3_cap;
            case RL_CHUNK_WARP: return &warp_cap;
            case RL_CHUNK_BEADS: return &beads_cap;
        }
        return nullptr;
    }
    // the trips of the chunk loop under each cap in the most recent call that has one (rl_chunks_run); host bookkeeping only
    int chunks_run[RL_CHUNK_COUNT] = {};

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
        HIP_TRY(hipMalloc(&dev, rl::dtype_size(dtype) * n));
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

