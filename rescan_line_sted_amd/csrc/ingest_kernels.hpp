// ingest_kernels.hpp -- acquired camera stacks in their native type (rl_ingest, rl_export, include/rlsted.h; DESIGN.md section
// 4j): the thread bodies of ingest_kernels.hip, written as host-compilable templates so that the CPU tests run the very same code
// (tests/emu/ingest_emu.cpp), and the launchers.
//
// INGEST  raw (TR: u8, u16, i16, f32), src_images sensor frames of src_ny x src_pitch elements -> dst [n_slots][V][ny][nx] (TD: f32,
//   f64), a plan's measurement buffer.  The source image of slot b, view v is b * frame_stride + v * view_stride; the window's
//   origin in it is (y0, x0).  Slots >= n_valid are fillers, written with ones.  Per pixel, in float64, no contraction:
//       x = (double)raw;  d = dark ? (double)dark[y][x] : offset;  v = (x - d) * gain            (two roundings)
//       saturated += saturation > 0 && x >= saturation
//       v not finite: invalid += 1, v = 0;   otherwise v < 0: clipped += 1, v = 0
//       out = (TD)(v + epsilon)
// EXPORT  est [n][ny * nx] (TE: f32, f64) -> out (TO: f32, f64, u16):  y = (double)e * scale;  f32 / f64: (TO)y, one rounding;
//   u16: rint(y) (half to even), nan and y <= 0 give 0, y > 65535 gives 65535 and is counted.
//
// Work split (decided by the image size alone, as in accel_kernels.hpp): an image is nvec vectors of W = 8 pixels -- INGEST: every
// destination row is ceil(nx / W) vectors, the last one partial; EXPORT: the ny * nx pixels as one run, the last vector partial --
// handed out in nb = ingest_blocks(nvec) equal runs of vpb = ceil(nvec / nb) vectors, one run per workgroup of kIngestThreads
// threads; thread t of workgroup b takes vectors b * vpb + t, + kIngestThreads, ...  A vector's W source values are one unaligned
// run (tile_load_run: 16 bytes of u16 / i16) where the vector is whole, element loads where it is partial: nothing outside the
// window is read.  Stores are 16-byte ones where every vector is whole and the destination is 16-byte aligned, element stores
// otherwise; nothing is written past the destination's values.
// Statistics, float64: INGEST [image][4] = sum of the stored values (as float64), clipped, saturated, invalid; EXPORT [image][2]
// = sum of (double)e, clamped.  The fixed order of accel_kernels.hpp:
//   thread    (((0 + p_0) + p_1) + ...) over its vectors in increasing order, the W pixels of a vector in order
//   workgroup tree over the kIngestThreads slots: s[t] = s[t] + s[t + h] for t < h, h = kIngestThreads / 2, ..., 1
//   image     (((0 + part_0) + part_1) + ...) over the workgroups in increasing order (k_ingest_totals)
// No atomics: bit-identical from run to run; the counts are sums of 0 / 1 in float64, exact below 2^53.
#pragma once
#include "tile_kernels.hpp"

#include <cstddef>
#include <cstdint>

namespace rl {

constexpr int kIngestThreads = 256;      // four waves
constexpr int kIngestW = 8;              // pixels per vector
constexpr int kIngestVecsPerThread = 4;  // vectors per thread the work split aims at
constexpr int kIngestFields = 4;         // RL_INGEST_FIELDS
constexpr int kExportFields = 2;         // RL_EXPORT_FIELDS
enum IngestRaw { RAW_U8 = 0, RAW_U16 = 1, RAW_I16 = 2, RAW_F32 = 3 };   // RL_RAW_*
enum ExportOut { OUT_F32 = 0, OUT_F64 = 1, OUT_U16 = 2 };               // RL_OUT_*

// workgroups per image of nvec vectors
RL_HD int ingest_blocks(size_t nvec) {
    const size_t per = (size_t)kIngestThreads * kIngestVecsPerThread, nb = (nvec + per - 1) / per;
    return nb < 1 ? 1 : (nb > 0x10000 ? 0x10000 : (int)nb);
}
RL_HD size_t ingest_vectors(int ny, int nx) { return (size_t)ny * (size_t)((nx + kIngestW - 1) / kIngestW); }
RL_HD size_t export_vectors(size_t n_pix) { return (n_pix + kIngestW - 1) / kIngestW; }

// what a launch is told, whatever its types (the launchers', the C ABI's and the emulation's)
struct IngestArgs {
    const void* raw;        // src_images x src_ny x src_pitch
    void* dst;              // [n_slots][V][ny][nx]
    const float* dark;      // [ny][nx] in window coordinates, or nullptr: `offset`
    double* part;           // [n_slots * V][nb][4] workspace, or nullptr: no statistics
    double* stats;          // [n_slots * V][4], or nullptr
    long long frame_stride, view_stride;   // in source images
    int src_ny, src_pitch, y0, x0, n_slots, n_valid, V, ny, nx;
    double offset, gain, epsilon, saturation;
};
struct ExportArgs {
    const void* est;        // [n][n_pix]
    void* out;              // [n][n_pix]
    double* part;           // [n][nb][2] workspace, or nullptr
    double* stats;          // [n][2], or nullptr
    int n;
    size_t n_pix;
    double scale;
};

template <typename TR, typename TD>
struct IngestParams {
    const TR* raw;
    TD* dst;
    const float* dark;
    double* part;
    long long frame_stride, view_stride;
    size_t src_elems;       // src_ny * src_pitch
    int src_pitch, y0, x0, n_valid, V, ny, nx;
    int cpr;                // vectors per destination row
    int nb;                 // workgroups per image
    bool vec;               // 16-byte stores
    double offset, gain, epsilon, saturation;
};
template <typename TE, typename TO>
struct ExportParams {
    const TE* est;
    TO* out;
    double* part;
    size_t n_pix;
    int nb;
    bool vec;
    double scale;
};

template <typename TR, typename TD>
inline IngestParams<TR, TD> ingest_params(const IngestArgs& a, int nb) {
    IngestParams<TR, TD> p;
    p.raw = (const TR*)a.raw;
    p.dst = (TD*)a.dst;
    p.dark = a.dark;
    p.part = a.part;
    p.frame_stride = a.frame_stride; p.view_stride = a.view_stride;
    p.src_elems = (size_t)a.src_ny * (size_t)a.src_pitch;
    p.src_pitch = a.src_pitch; p.y0 = a.y0; p.x0 = a.x0; p.n_valid = a.n_valid; p.V = a.V; p.ny = a.ny; p.nx = a.nx;
    p.cpr = (a.nx + kIngestW - 1) / kIngestW;
    p.nb = nb;
    p.vec = a.nx % kIngestW == 0 && accel_aligned(a.dst);
    p.offset = a.offset; p.gain = a.gain; p.epsilon = a.epsilon; p.saturation = a.saturation;
    return p;
}
template <typename TE, typename TO>
inline ExportParams<TE, TO> export_params(const ExportArgs& a, int nb) {
    ExportParams<TE, TO> p;
    p.est = (const TE*)a.est;
    p.out = (TO*)a.out;
    p.part = a.part;
    p.n_pix = a.n_pix;
    p.nb = nb;
    p.vec = a.n_pix % kIngestW == 0 && accel_aligned(a.out);
    p.scale = a.scale;
    return p;
}

// kIngestW values of a row of n: accel_store's 16-byte vectors (or its element stores), one after the other
template <typename T>
RL_HD void ingest_store(T* row, size_t e0, size_t n, bool vec, const T* v) {
    constexpr int WT = 16 / sizeof(T);
    for (int k = 0; k < kIngestW; k += WT) accel_store(row, e0 + k, n, vec, v + k);
}

RL_HD bool ingest_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }   // (nan fails both)

// INGEST, thread t of workgroup b of destination image `img` (= slot * V + view): writes its vectors, returns its four sums
template <typename TR, typename TD>
RL_HD void ingest_thread(const IngestParams<TR, TD>& p, size_t img, int b, int t, double* sums) {
#pragma clang fp contract(off)
    constexpr int W = kIngestW;
    const size_t nvec = (size_t)p.ny * p.cpr, vpb = (nvec + p.nb - 1) / p.nb;
    const size_t slot = img / (size_t)p.V;
    const int view = (int)(img % (size_t)p.V);
    const bool filler = slot >= (size_t)p.n_valid;
    const long long src_img = filler ? 0 : (long long)slot * p.frame_stride + (long long)view * p.view_stride;
    const TR* src = p.raw + (size_t)src_img * p.src_elems + (size_t)p.y0 * p.src_pitch + (size_t)p.x0;
    TD* dst = p.dst + img * (size_t)p.ny * p.nx;
    double s_sum = 0.0, s_clip = 0.0, s_sat = 0.0, s_inv = 0.0;
    const size_t j1 = ((size_t)b + 1) * vpb < nvec ? ((size_t)b + 1) * vpb : nvec;
    for (size_t j = (size_t)b * vpb + t; j < j1; j += kIngestThreads) {
        size_t y;
        int c;
        tile_divmod(j, p.cpr, y, c);
        const int x0 = c * W;
        const bool whole = x0 + W <= p.nx;
        TD out[W];
        if (filler) {
            for (int e = 0; e < W; ++e) out[e] = TD(1);
        } else {
            const TR* s = src + y * (size_t)p.src_pitch + (size_t)x0;
            TR in[W];
            float dk[W];
            if (whole) {
                tile_load_run<TR, W>(s, in);
            } else {
                for (int e = 0; e < W; ++e) in[e] = x0 + e < p.nx ? s[e] : TR(0);
            }
            if (p.dark) {
                const float* ds = p.dark + y * (size_t)p.nx + (size_t)x0;
                if (whole) {
                    tile_load_run<float, W>(ds, dk);
                } else {
                    for (int e = 0; e < W; ++e) dk[e] = x0 + e < p.nx ? ds[e] : 0.0f;
                }
            }
            for (int e = 0; e < W; ++e) {
                const double x = (double)in[e];
                const double d = p.dark ? (double)dk[e] : p.offset;
                const double diff = x - d;
                double v = diff * p.gain;
                const bool live = x0 + e < p.nx;
                if (live && p.saturation > 0.0 && x >= p.saturation) s_sat = s_sat + 1.0;
                if (!ingest_finite(v)) {
                    if (live) s_inv = s_inv + 1.0;
                    v = 0.0;
                } else if (v < 0.0) {
                    if (live) s_clip = s_clip + 1.0;
                    v = 0.0;
                }
                const double w = v + p.epsilon;
                out[e] = (TD)w;
            }
        }
        for (int e = 0; e < W; ++e)
            if (x0 + e < p.nx) s_sum = s_sum + (double)out[e];
        ingest_store(dst + y * (size_t)p.nx, (size_t)x0, (size_t)p.nx, p.vec, out);
    }
    sums[0] = s_sum; sums[1] = s_clip; sums[2] = s_sat; sums[3] = s_inv;
}

// one value of the EXPORT
template <typename TO>
RL_HD TO export_value(double y, double& clamped) {
    return (TO)y;
}
template <>
RL_HD uint16_t export_value<uint16_t>(double y, double& clamped) {
    if (!(y > 0.0)) return 0;                 // nan, negative, zero
    if (y > 65535.0) {
        clamped = clamped + 1.0;
        return 65535;
    }
    return (uint16_t)__builtin_rint(y);       // round to nearest, ties to even
}

// EXPORT, thread t of workgroup b of image `img`: writes its vectors, returns its two sums
template <typename TE, typename TO>
RL_HD void export_thread(const ExportParams<TE, TO>& p, size_t img, int b, int t, double* sums) {
#pragma clang fp contract(off)
    constexpr int W = kIngestW;
    const size_t n = p.n_pix, nvec = (n + W - 1) / W, vpb = (nvec + p.nb - 1) / p.nb;
    const TE* src = p.est + img * n;
    TO* dst = p.out + img * n;
    double s_sum = 0.0, s_clamp = 0.0;
    const size_t j1 = ((size_t)b + 1) * vpb < nvec ? ((size_t)b + 1) * vpb : nvec;
    for (size_t j = (size_t)b * vpb + t; j < j1; j += kIngestThreads) {
        const size_t e0 = j * W;
        TE in[W];
        TO out[W];
        if (e0 + W <= n) {
            tile_load_run<TE, W>(src + e0, in);
        } else {
            for (int e = 0; e < W; ++e) in[e] = e0 + e < n ? src[e0 + e] : TE(0);
        }
        for (int e = 0; e < W; ++e) {
            const double v = (double)in[e];
            const double y = v * p.scale;
            double c = 0.0;
            out[e] = export_value<TO>(y, c);
            if (e0 + e < n) {
                s_sum = s_sum + v;
                s_clamp = s_clamp + c;
            }
        }
        ingest_store(dst, e0, n, p.vec, out);
    }
    sums[0] = s_sum; sums[1] = s_clamp;
}

// an image's field from its workgroups' partials [nb][fields], summed in increasing order
RL_HD double ingest_total(const double* part, int nb, int fields, int field) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s = s + part[(size_t)b * fields + field];
    return s;
}

// ---- launchers (ingest_kernels.hip), on stream s.  raw_dtype: RL_RAW_*; dst / est dtype: RL_F32 / RL_F64; out_dtype: RL_OUT_*.
// All pointers are device pointers; part must hold images * ingest_blocks(vectors) * fields float64 values when stats is given.
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t ingest(int raw_dtype, int dst_dtype, const IngestArgs& a, hipStream_t s);
hipError_t export_estimates(int est_dtype, int out_dtype, const ExportArgs& a, hipStream_t s);
#endif

}  // namespace rl
