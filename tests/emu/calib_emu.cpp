// Host emulator of the calibration kernels (rescan_line_sted_amd/csrc/calib_kernels.hpp, calib_kernels.hip): the very same thread
// bodies, run thread by thread at the launchers' geometry -- ACCUMULATE over (window workgroups) x (parts of the frame split) x 256
// threads, FINALIZE per pixel, REPAIR per (image, listed defect) with the host's own list.  TEST INFRASTRUCTURE ONLY -- built by
// tests/test_calibration_cpu.py with g++ (-ffp-contract=off), as a shared library and, with -DCALIB_EMU_MAIN, as a stand-alone
// program for the sanitizers; never loaded by the product.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/calib_kernels.hpp"
#include "../../rescan_line_sted_amd/csrc/ingest_kernels.hpp"

using namespace rl;

namespace {
template <typename TR>
int accumulate_run(const void* raw, void* sum, void* sumsq, int src_ny, int src_pitch, int y0, int x0, int ny, int nx, int n_frames, int parts_override) {
    const int groups = calib_groups(calib_vectors(ny, nx));
    const int parts = parts_override > 0 && CalibAcc<TR>::integer ? parts_override : calib_parts(groups, n_frames, CalibAcc<TR>::integer);
    const CalibParams<TR> p = calib_params<TR>(raw, sum, sumsq, src_ny, src_pitch, y0, x0, ny, nx, n_frames, parts);
    for (int part = parts - 1; part >= 0; --part)        // (any order of the parts: here the last first)
        for (int b = 0; b < groups; ++b)
            for (int t = 0; t < kCalibThreads; ++t) calib_accumulate_thread<TR>(p, b, t, part);
    return parts;
}
}  // namespace

extern "C" {
int emu_calib_parts(int ny, int nx, int n_frames, int integer) { return calib_parts(calib_groups(calib_vectors(ny, nx)), n_frames, integer != 0); }

// raw_dtype: 0 u8, 1 u16, 2 i16, 3 f32; sum / sumsq: [ny][nx] of 8 bytes, the accumulators that hold `frames` frames.  parts: the
// frame split to force, 0: the launcher's.  Returns the parts used, -1 where rl_calib_accumulate refuses (nothing is touched).
int emu_calib_accumulate(const void* raw, int raw_dtype, int src_ny, int src_pitch, int y0, int x0, int ny, int nx, int n_frames, void* sum,
                         void* sumsq, long long frames, int parts) {
    if (raw_dtype < 0 || raw_dtype > 3 || !calib_frames_ok(raw_dtype != RAW_F32, frames, n_frames)) return -1;
    switch (raw_dtype) {
        case RAW_U8: return accumulate_run<uint8_t>(raw, sum, sumsq, src_ny, src_pitch, y0, x0, ny, nx, n_frames, parts);
        case RAW_U16: return accumulate_run<uint16_t>(raw, sum, sumsq, src_ny, src_pitch, y0, x0, ny, nx, n_frames, parts);
        case RAW_I16: return accumulate_run<int16_t>(raw, sum, sumsq, src_ny, src_pitch, y0, x0, ny, nx, n_frames, parts);
    }
    return accumulate_run<float>(raw, sum, sumsq, src_ny, src_pitch, y0, x0, ny, nx, n_frames, parts);
}

void emu_calib_finalize(int raw_dtype, const void* sum, const void* sumsq, long long frames, long long n_pix, double* mean, double* var) {
    for (size_t i = 0; i < (size_t)n_pix; ++i) {
        if (raw_dtype == RAW_F32) {
            calib_finalize_f32((const double*)sum, (const double*)sumsq, frames, i, mean, var);
        } else {
            calib_finalize_int((const long long*)sum, (const unsigned long long*)sumsq, frames, i, mean, var);
        }
    }
}

// dtype: 0 f32, 1 f64.  Returns the threads per image (listed defects), -1 on a bad argument; *unrepaired: the count per image.
int emu_repair(void* img, int dtype, int n_images, int ny, int nx, const unsigned char* mask, int radius, long long* unrepaired) {
    if (radius < 1 || radius > kRepairMaxRadius || (dtype != 0 && dtype != 1)) return -1;
    std::vector<RepairEntry> list;
    repair_list(mask, ny, nx, radius, list, nullptr, unrepaired);
    const size_t n_pix = (size_t)ny * nx;
    for (size_t id = 0; id < (size_t)n_images * list.size(); ++id) {
        const size_t image = id / list.size();
        if (dtype == 0) {
            repair_thread<float>((float*)img + image * n_pix, nx, list[id % list.size()]);
        } else {
            repair_thread<double>((double*)img + image * n_pix, nx, list[id % list.size()]);
        }
    }
    return (int)list.size();
}
}

#ifdef CALIB_EMU_MAIN
// The stand-alone program of the sanitizer run: raw frames, accumulators, maps, images and mask are heap blocks of EXACTLY their byte
// counts, and the window ends with the sensor frame (the unaligned last run of the last row of the last frame ends at the last
// byte of `raw`); a read or a write past any of them is the sanitizer's to find.  Results are held to plain loops written here.
// Prints "ok <accumulates> <repairs>" and returns 0.
namespace {
unsigned g_state = 2463534242u;
unsigned next_u() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 17;
    g_state ^= g_state << 5;
    return g_state;
}

template <typename T>
struct Exact {
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
template <> float raw_value<float>(unsigned u) { return (float)(u >> 12) * 0.37f - 40.0f; }

template <typename TR>
int accumulate_case(int rdt, int ny, int nx, int pad, int y0, int x0, int F, int parts, long* done) {
    const int src_ny = y0 + ny, src_pitch = x0 + nx + pad;
    Exact<TR> raw((size_t)F * src_ny * src_pitch);
    for (size_t i = 0; i < raw.n; ++i) raw.p[i] = raw_value<TR>(next_u());
    Exact<long long> sum((size_t)ny * nx), sumsq((size_t)ny * nx);
    Exact<double> mean((size_t)ny * nx), var((size_t)ny * nx);
    std::memset(sum.p, 0, sum.n * 8);
    std::memset(sumsq.p, 0, sumsq.n * 8);
    const int first = F / 2;
    if (first > 0 && emu_calib_accumulate(raw.p, rdt, src_ny, src_pitch, y0, x0, ny, nx, first, sum.p, sumsq.p, 0, parts) < 0) return 1;
    if (emu_calib_accumulate(raw.p + (size_t)first * src_ny * src_pitch, rdt, src_ny, src_pitch, y0, x0, ny, nx, F - first, sum.p, sumsq.p, first, parts) < 0)
        return 1;
    emu_calib_finalize(rdt, sum.p, sumsq.p, F, (long long)ny * nx, mean.p, var.p);
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const size_t i = (size_t)y * nx + x;
            if (rdt == RAW_F32) {
                double s = 0, q = 0;
                for (int f = 0; f < F; ++f) {
                    const double v = (double)raw.p[((size_t)f * src_ny + y0 + y) * src_pitch + x0 + x];
                    s = s + v;
                    q = q + v * v;
                }
                double got_s, got_q;
                std::memcpy(&got_s, sum.p + i, 8);
                std::memcpy(&got_q, sumsq.p + i, 8);
                if (got_s != s || got_q != q) return 1;
            } else {
                long long s = 0;
                unsigned long long q = 0;
                for (int f = 0; f < F; ++f) {
                    const long long v = (long long)raw.p[((size_t)f * src_ny + y0 + y) * src_pitch + x0 + x];
                    s += v;
                    q += (unsigned long long)(v * v);
                }
                if (sum.p[i] != s || (unsigned long long)sumsq.p[i] != q) {
                    std::printf("accumulate dtype %d %d x %d (%d, %d): %lld %llu, want %lld %llu\n", rdt, ny, nx, y, x, sum.p[i],
                                (unsigned long long)sumsq.p[i], s, q);
                    return 1;
                }
                if (mean.p[i] != (double)s / (double)F) return 1;
            }
            if (!(var.p[i] >= 0.0) && rdt != RAW_F32) return 1;
        }
    ++*done;
    return 0;
}

template <typename T>
int repair_case(int ny, int nx, int radius, int every, long* done) {
    const int n = 3;
    Exact<T> img((size_t)n * ny * nx), before((size_t)n * ny * nx);
    Exact<unsigned char> mask((size_t)ny * nx);
    for (size_t i = 0; i < img.n; ++i) before.p[i] = img.p[i] = (T)((double)(next_u() >> 12) * 0.01);
    long long defects = 0;
    for (size_t i = 0; i < mask.n; ++i) defects += mask.p[i] = (next_u() % (unsigned)every) == 0 ? 1 : 0;
    mask.p[0] = mask.p[mask.n - 1] = 1;                     // the first and the last pixel of every image
    long long left = -1;
    const int listed = emu_repair(img.p, sizeof(T) == 4 ? 0 : 1, n, ny, nx, mask.p, radius, &left);
    if (listed < 0 || left < 0) return 1;
    for (int i = 0; i < n; ++i)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const size_t k = ((size_t)i * ny + y) * nx + x;
                if (!mask.p[(size_t)y * nx + x]) {
                    if (std::memcmp(img.p + k, before.p + k, sizeof(T)) != 0) return 1;      // a good pixel was written
                    continue;
                }
                // the replacement lies between the smallest and the largest good value of the widest window
                double lo = 1e300, hi = -1e300;
                for (int dy = -radius; dy <= radius; ++dy)
                    for (int dx = -radius; dx <= radius; ++dx) {
                        const int yy = y + dy, xx = x + dx;
                        if (yy < 0 || yy >= ny || xx < 0 || xx >= nx || mask.p[(size_t)yy * nx + xx]) continue;
                        const double v = (double)before.p[((size_t)i * ny + yy) * nx + xx];
                        lo = v < lo ? v : lo;
                        hi = v > hi ? v : hi;
                    }
                if (lo <= hi && !((double)img.p[k] >= lo && (double)img.p[k] <= hi)) return 1;
                if (lo > hi && std::memcmp(img.p + k, before.p + k, sizeof(T)) != 0) return 1;  // unrepairable: untouched
            }
    ++*done;
    return 0;
}
}  // namespace

int main() {
    long accumulates = 0, repairs = 0;
    const int shapes[][2] = {{5, 13}, {7, 16}, {3, 33}, {1, 8}};
    const int origins[][2] = {{0, 0}, {2, 1}, {1, 5}};
    for (const auto& sh : shapes)
        for (int pad : {0, 3})
            for (const auto& o : origins)
                for (int parts : {0, 3}) {
                    const int F = 7 + sh[0];
                    if (accumulate_case<uint8_t>(RAW_U8, sh[0], sh[1], pad, o[0], o[1], F, parts, &accumulates) ||
                        accumulate_case<uint16_t>(RAW_U16, sh[0], sh[1], pad, o[0], o[1], F, parts, &accumulates) ||
                        accumulate_case<int16_t>(RAW_I16, sh[0], sh[1], pad, o[0], o[1], F, parts, &accumulates) ||
                        accumulate_case<float>(RAW_F32, sh[0], sh[1], pad, o[0], o[1], F, parts, &accumulates))
                        return 1;
                }
    for (const auto& sh : shapes)
        for (int radius : {1, 2, 3})
            for (int every : {2, 7, 1}) {              // (every = 1: all defects, nothing to repair)
                if (repair_case<float>(sh[0], sh[1], radius, every, &repairs) || repair_case<double>(sh[0], sh[1], radius, every, &repairs)) return 1;
            }
    std::printf("ok %ld %ld\n", accumulates, repairs);
    return 0;
}
#endif
