// Host emulator of the ingest / export kernels (rescan_line_sted_amd/csrc/ingest_kernels.hpp, ingest_kernels.hip): the very same
// thread bodies, run thread by thread over the launch grid (images x nb workgroups of kIngestThreads threads), the workgroup tree
// and the totals in the kernels' order, with the launchers' own parameters.  TEST INFRASTRUCTURE ONLY -- built by
// tests/test_stack_cpu.py with g++ (-ffp-contract=off), as a shared library and, with -DINGEST_EMU_MAIN, as a stand-alone program
// for the sanitizers; never loaded by the product.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/ingest_kernels.hpp"

using namespace rl;

namespace {

// the tree of ingest_tree() and k_ingest_totals, for one workgroup's FIELDS x kIngestThreads sums
template <int FIELDS>
void tree(std::vector<double>* sm, double* part) {
    for (int h = kIngestThreads / 2; h > 0; h >>= 1)
        for (int f = 0; f < FIELDS; ++f)
            for (int t = 0; t < kIngestThreads; ++t) accel_tree_step(sm[f].data(), t, h);   // (t < h reads slots >= h only)
    for (int f = 0; f < FIELDS; ++f) part[f] = sm[f][0];
}

template <typename TR, typename TD>
int ingest_run(const IngestArgs& a, int nb_override) {
    const int nb = nb_override > 0 ? nb_override : ingest_blocks(ingest_vectors(a.ny, a.nx));
    const size_t images = (size_t)a.n_slots * a.V;
    std::vector<double> part(images * nb * kIngestFields);
    IngestArgs b = a;
    b.part = a.stats ? part.data() : nullptr;
    const IngestParams<TR, TD> p = ingest_params<TR, TD>(b, nb);
    std::vector<double> sm[kIngestFields];
    for (auto& s : sm) s.resize(kIngestThreads);
    for (size_t block = 0; block < images * nb; ++block) {
        for (int t = 0; t < kIngestThreads; ++t) {
            double sums[kIngestFields];
            ingest_thread<TR, TD>(p, block / nb, (int)(block % nb), t, sums);
            for (int f = 0; f < kIngestFields; ++f) sm[f][t] = sums[f];
        }
        if (p.part) tree<kIngestFields>(sm, p.part + block * kIngestFields);
    }
    if (a.stats)
        for (size_t id = 0; id < images * kIngestFields; ++id)
            a.stats[id] = ingest_total(part.data() + (id / kIngestFields) * nb * kIngestFields, nb, kIngestFields, (int)(id % kIngestFields));
    return p.vec ? 1 : 0;
}

template <typename TE, typename TO>
int export_run(const ExportArgs& a, int nb_override) {
    const int nb = nb_override > 0 ? nb_override : ingest_blocks(export_vectors(a.n_pix));
    std::vector<double> part((size_t)a.n * nb * kExportFields);
    ExportArgs b = a;
    b.part = a.stats ? part.data() : nullptr;
    const ExportParams<TE, TO> p = export_params<TE, TO>(b, nb);
    std::vector<double> sm[kExportFields];
    for (auto& s : sm) s.resize(kIngestThreads);
    for (size_t block = 0; block < (size_t)a.n * nb; ++block) {
        for (int t = 0; t < kIngestThreads; ++t) {
            double sums[kExportFields];
            export_thread<TE, TO>(p, block / nb, (int)(block % nb), t, sums);
            for (int f = 0; f < kExportFields; ++f) sm[f][t] = sums[f];
        }
        if (p.part) tree<kExportFields>(sm, p.part + block * kExportFields);
    }
    if (a.stats)
        for (size_t id = 0; id < (size_t)a.n * kExportFields; ++id)
            a.stats[id] = ingest_total(part.data() + (id / kExportFields) * nb * kExportFields, nb, kExportFields, (int)(id % kExportFields));
    return p.vec ? 1 : 0;
}

template <typename TR>
int ingest_r(int dst_dtype, const IngestArgs& a, int nb) {
    return dst_dtype == 0 ? ingest_run<TR, float>(a, nb) : ingest_run<TR, double>(a, nb);
}
template <typename TE>
int export_e(int out_dtype, const ExportArgs& a, int nb) {
    return out_dtype == OUT_F32 ? export_run<TE, float>(a, nb) : (out_dtype == OUT_F64 ? export_run<TE, double>(a, nb) : export_run<TE, uint16_t>(a, nb));
}

}  // namespace

extern "C" {
int emu_ingest_blocks(int ny, int nx) { return ingest_blocks(ingest_vectors(ny, nx)); }
int emu_export_blocks(int ny, int nx) { return ingest_blocks(export_vectors((size_t)ny * nx)); }
// raw_dtype: 0 u8, 1 u16, 2 i16, 3 f32; dst_dtype: 0 f32, 1 f64.  dst: exactly n_slots * V * ny * nx values; stats: NULL or
// [n_slots * V][4].  nb: workgroups per image, 0: the launcher's.  Returns 1 if the launch takes the 16-byte store path, else 0.
int emu_ingest(const void* raw, int raw_dtype, int src_ny, int src_pitch, int y0, int x0, long long frame_stride, long long view_stride,
               int n_slots, int n_valid, int V, int ny, int nx, const float* dark, double offset, double gain, double epsilon,
               double saturation, void* dst, int dst_dtype, double* stats, int nb) {
    IngestArgs a;
    a.raw = raw; a.dst = dst; a.dark = dark; a.part = nullptr; a.stats = stats;
    a.frame_stride = frame_stride; a.view_stride = view_stride;
    a.src_ny = src_ny; a.src_pitch = src_pitch; a.y0 = y0; a.x0 = x0; a.n_slots = n_slots; a.n_valid = n_valid; a.V = V; a.ny = ny; a.nx = nx;
    a.offset = offset; a.gain = gain; a.epsilon = epsilon; a.saturation = saturation;
    switch (raw_dtype) {
        case RAW_U8: return ingest_r<uint8_t>(dst_dtype, a, nb);
        case RAW_U16: return ingest_r<uint16_t>(dst_dtype, a, nb);
        case RAW_I16: return ingest_r<int16_t>(dst_dtype, a, nb);
        case RAW_F32: return ingest_r<float>(dst_dtype, a, nb);
    }
    return -1;
}
// est_dtype: 0 f32, 1 f64; out_dtype: 0 f32, 1 f64, 2 u16.  stats: NULL or [n][2].
int emu_export(const void* est, int est_dtype, int n, int ny, int nx, double scale, void* out, int out_dtype, double* stats, int nb) {
    ExportArgs a;
    a.est = est; a.out = out; a.part = nullptr; a.stats = stats; a.n = n; a.n_pix = (size_t)ny * nx; a.scale = scale;
    if (out_dtype < 0 || out_dtype > 2) return -1;
    return est_dtype == 0 ? export_e<float>(out_dtype, a, nb) : export_e<double>(out_dtype, a, nb);
}
}

#ifdef INGEST_EMU_MAIN
// The stand-alone program of the sanitizer run: the raw, dark, destination and output buffers are heap blocks of EXACTLY their
// byte counts -- the sensor frame ends with the window (src_ny = y0 + ny, x0 + nx = src_pitch in the last row that is read), so the
// unaligned last run of the last row of the last image ends at the last byte of `raw`; a read or a write past any of them is the
// sanitizer's to find.  Results are held to plain loops written here.  Prints "ok <ingests> <exports>" and returns 0.
namespace {
unsigned g_state = 2463534242u;
unsigned next_u() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 17;
    g_state ^= g_state << 5;
    return g_state;
}

template <typename T>
struct Exact {   // n values at exactly n * sizeof(T) bytes
    T* p;
    size_t n;
    explicit Exact(size_t count) : p((T*)std::malloc(count * sizeof(T))), n(count) {}
    ~Exact() { std::free(p); }
    Exact(const Exact&) = delete;
};

template <typename TR> TR raw_value(unsigned u);
template <> uint8_t raw_value<uint8_t>(unsigned u) { return (uint8_t)(u >> 9); }
template <> uint16_t raw_value<uint16_t>(unsigned u) { return (u & 31u) == 0 ? 65535 : (uint16_t)(u >> 11); }
template <> int16_t raw_value<int16_t>(unsigned u) { return (int16_t)(u >> 7); }
template <> float raw_value<float>(unsigned u) {
    if ((u & 63u) == 0) return std::numeric_limits<float>::quiet_NaN();
    if ((u & 63u) == 1) return std::numeric_limits<float>::infinity();
    if ((u & 63u) == 2) return -std::numeric_limits<float>::infinity();
    return (float)(u >> 12) * 0.37f - 40.0f;
}

template <typename TR, typename TD>
int ingest_case(int ny, int nx, int pad, int y0, int x0, bool view_frame, int V, bool dark_map, long* done) {
    const int n_slots = 3, n_valid = 2, src_ny = y0 + ny, src_pitch = x0 + nx + pad, src_images = n_valid * V;
    const long long fs = view_frame ? 1 : V, vs = view_frame ? n_valid : 1;
    const double offset = 100.25, gain = 0.4587, eps = 1e-9, sat = sizeof(TR) == 1 ? 250.0 : 65535.0;
    // (the last row that is read ends src_pitch - x0 - nx = pad elements before the frame's end: pad 0 is the case to catch)
    Exact<TR> raw((size_t)src_images * src_ny * src_pitch);
    for (size_t i = 0; i < raw.n; ++i) raw.p[i] = raw_value<TR>(next_u());
    Exact<float> dark((size_t)ny * nx);
    for (size_t i = 0; i < dark.n; ++i) dark.p[i] = 90.0f + (float)(next_u() >> 24) * 0.125f;
    Exact<TD> dst((size_t)n_slots * V * ny * nx);
    Exact<double> stats((size_t)n_slots * V * kIngestFields);
    const int rdt = sizeof(TR) == 1 ? RAW_U8 : (sizeof(TR) == 4 ? RAW_F32 : (TR(-1) < TR(0) ? RAW_I16 : RAW_U16));
    for (int nb : {0, 2}) {
        for (size_t i = 0; i < dst.n; ++i) dst.p[i] = TD(-7);
        if (emu_ingest(raw.p, rdt, src_ny, src_pitch, y0, x0, fs, vs, n_slots, n_valid, V, ny, nx, dark_map ? dark.p : nullptr, offset, gain, eps,
                       sat, dst.p, sizeof(TD) == 4 ? 0 : 1, stats.p, nb) < 0)
            return 1;
        for (int b = 0; b < n_slots; ++b)
            for (int v = 0; v < V; ++v) {
                double counts[3] = {0, 0, 0};
                for (int y = 0; y < ny; ++y)
                    for (int x = 0; x < nx; ++x) {
                        TD want = TD(1);
                        if (b < n_valid) {
                            const double r = (double)raw.p[((size_t)(b * fs + v * vs) * src_ny + y0 + y) * src_pitch + x0 + x];
                            const double d = dark_map ? (double)dark.p[(size_t)y * nx + x] : offset;
                            double val = (r - d) * gain;
                            if (r >= sat) counts[1] += 1;
                            if (!std::isfinite(val)) {
                                counts[2] += 1;
                                val = 0;
                            } else if (val < 0) {
                                counts[0] += 1;
                                val = 0;
                            }
                            want = (TD)(val + eps);
                        }
                        const TD got = dst.p[(((size_t)b * V + v) * ny + y) * nx + x];
                        if (got != want) {
                            std::printf("ingest %d x %d slot %d view %d (%d, %d): %.17g, want %.17g\n", ny, nx, b, v, y, x, (double)got, (double)want);
                            return 1;
                        }
                    }
                const double* s = stats.p + ((size_t)b * V + v) * kIngestFields;
                if (s[1] != counts[0] || s[2] != counts[1] || s[3] != counts[2]) {
                    std::printf("ingest %d x %d slot %d view %d: counts %g %g %g, want %g %g %g\n", ny, nx, b, v, s[1], s[2], s[3], counts[0], counts[1], counts[2]);
                    return 1;
                }
            }
        ++*done;
    }
    return 0;
}

template <typename TE, typename TO>
int export_case(int ny, int nx, long* done) {
    const int n = 2;
    const double scale = 3.0;
    Exact<TE> est((size_t)n * ny * nx);
    for (size_t i = 0; i < est.n; ++i) est.p[i] = (TE)((double)(next_u() >> 12) * 0.03 - 500.0);
    est.p[0] = (TE)0.5; est.p[1] = (TE)1.5; est.p[2] = (TE)2.5; est.p[3] = (TE)std::numeric_limits<double>::quiet_NaN();
    Exact<TO> out(est.n);
    Exact<double> stats((size_t)n * kExportFields);
    if (emu_export(est.p, sizeof(TE) == 4 ? 0 : 1, n, ny, nx, scale, out.p, sizeof(TO) == 2 ? OUT_U16 : (sizeof(TO) == 4 ? OUT_F32 : OUT_F64), stats.p, 0) < 0)
        return 1;
    for (int i = 0; i < n; ++i) {
        double clamped = 0;
        for (size_t k = 0; k < (size_t)ny * nx; ++k) {
            const double y = (double)est.p[(size_t)i * ny * nx + k] * scale;
            TO want;
            if (sizeof(TO) == 2) {
                if (y > 65535.0) clamped += 1;
                want = !(y > 0.0) ? TO(0) : (y > 65535.0 ? TO(65535) : (TO)std::nearbyint(y));
            } else {
                want = (TO)y;
            }
            const TO got = out.p[(size_t)i * ny * nx + k];
            if (std::memcmp(&got, &want, sizeof(TO)) != 0 && !(got != got && want != want)) {
                std::printf("export %d x %d image %d pixel %zu: %.17g, want %.17g\n", ny, nx, i, k, (double)got, (double)want);
                return 1;
            }
        }
        if (stats.p[i * kExportFields + 1] != clamped) return 1;
    }
    ++*done;
    return 0;
}

template <typename TR>
int ingest_cases(long* done) {
    const int shapes[][2] = {{5, 13}, {7, 16}, {3, 33}};
    const int origins[][2] = {{0, 0}, {2, 1}, {1, 5}};
    for (const auto& sh : shapes)
        for (int pad : {0, 3})
            for (const auto& o : origins)
                for (int V : {1, 3}) {
                    const bool vf = (V + pad + o[0]) % 2 == 1, dm = (sh[0] + o[1] + V) % 2 == 0;
                    if (ingest_case<TR, float>(sh[0], sh[1], pad, o[0], o[1], vf, V, dm, done) ||
                        ingest_case<TR, double>(sh[0], sh[1], pad, o[0], o[1], !vf, V, !dm, done))
                        return 1;
                }
    return 0;
}
}  // namespace

int main() {
    long ingests = 0, exports = 0;
    if (ingest_cases<uint8_t>(&ingests) || ingest_cases<uint16_t>(&ingests) || ingest_cases<int16_t>(&ingests) || ingest_cases<float>(&ingests)) return 1;
    const int shapes[][2] = {{5, 13}, {7, 16}, {3, 33}};
    for (const auto& sh : shapes)
        if (export_case<float, float>(sh[0], sh[1], &exports) || export_case<float, double>(sh[0], sh[1], &exports) ||
            export_case<float, uint16_t>(sh[0], sh[1], &exports) || export_case<double, float>(sh[0], sh[1], &exports) ||
            export_case<double, double>(sh[0], sh[1], &exports) || export_case<double, uint16_t>(sh[0], sh[1], &exports))
            return 1;
    std::printf("ok %ld %ld\n", ingests, exports);
    return 0;
}
#endif
