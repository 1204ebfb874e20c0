// Host emulator of the stencil kernels (rescan_line_sted_amd/csrc/sep_kernels.hpp), their host side (sep_taps.hpp) and the box
// normaliser (aux_kernels.hpp box_norm_pixel): the very same workgroup bodies, one OS thread per GPU thread, a pthread barrier for
// wg().  TEST INFRASTRUCTURE ONLY -- built by tests/test_sep_cpu.py with g++ (-ffp-contract=off), sanitized by tools/asan_emu.sh,
// never loaded by the product.
//
// What this grid runner does that tests/emu/emu.cpp's does not:
//   * the workgroup's LDS is one malloc of EXACTLY the byte count the launcher passes as dynamic LDS -- no slack, so that
//     AddressSanitizer's red zone begins at the first byte the launcher did not pay for -- and is filled with 0xff (a nan in
//     both types) before every workgroup: an element read before it was written shows in the output;
//   * the grid has a z dimension;
//   * the threads live for the whole launch and walk the workgroups together (no 256 thread starts per workgroup).
#include <pthread.h>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/aux_kernels.hpp"
#include "../../rescan_line_sted_amd/csrc/sep_kernels.hpp"
#include "../../rescan_line_sted_amd/csrc/sep_taps.hpp"

using namespace rl;

namespace {

struct EmuSync {
    pthread_barrier_t* bar;
    void wg() const { pthread_barrier_wait(bar); }
};

// body(tid, bx, by, bz, lds, sync) for every thread of every workgroup of grid (gx, gy, gz)
template <class Body>
void run_grid(int gx, int gy, int gz, int nthreads, size_t lds_bytes, Body body) {
    unsigned char* lds = (unsigned char*)std::malloc(lds_bytes ? lds_bytes : 1);
    pthread_barrier_t bar;        // wg()
    pthread_barrier_t between;    // workgroup boundaries (a thread that left its body early waits here, not in wg())
    pthread_barrier_init(&bar, nullptr, nthreads);
    pthread_barrier_init(&between, nullptr, nthreads);
    const long total = (long)gx * gy * gz;
    std::vector<std::thread> th;
    th.reserve(nthreads);
    for (int tid = 0; tid < nthreads; ++tid)
        th.emplace_back([&, tid]() {
            EmuSync s{&bar};
            for (long w = 0; w < total; ++w) {
                if (tid == 0) std::memset(lds, 0xff, lds_bytes);
                pthread_barrier_wait(&between);
                body(tid, (int)(w % gx), (int)(w / gx % gy), (int)(w / ((long)gx * gy)), lds, s);
                pthread_barrier_wait(&between);
            }
        });
    for (auto& t : th) t.join();
    pthread_barrier_destroy(&bar);
    pthread_barrier_destroy(&between);
    std::free(lds);
}

// the launchers of sep_kernels.hip, with their grids, LDS sizes and refusals
template <typename T>
int rows(const void* in, void* out, const void* v, int images, int ny, int nx, int px, int V, int in_div) {
    if (images < 1) return 0;
    const SepRowsParams<T> p{(const T*)in, (T*)out, (const T*)v, ny, nx, px, V, in_div};
    run_grid((nx + kRowSeg - 1) / kRowSeg, ny, images, kRowSeg, sep_rows_lds(sizeof(T), px),
             [&](int t, int bx, int by, int bz, unsigned char* lds, EmuSync& s) { sep_rows_body<T>(p, t, bx, by, bz, lds, s); });
    return 0;
}

template <typename T, int MODE>
int cols_m(const SepColsParams<T>& p, int count) {
    const size_t lds = sep_cols_lds(sizeof(T), p.py);
    if (lds > kSepMaxLds) return -1;
    run_grid((p.nx + kColW - 1) / kColW, (p.ny + kColH - 1) / kColH, count, kSepThreads, lds,
             [&](int t, int bx, int by, int bz, unsigned char* l, EmuSync& s) { sep_cols_body<T, MODE>(p, t, bx, by, bz, l, s); });
    return 0;
}
template <typename T>
int cols(int mode, const void* tmp, const void* u, const void* aux, const void* norm, void* dst, int count, int ny, int nx, int py, int V) {
    if (count < 1) return 0;
    const SepColsParams<T> p{(const T*)tmp, (const T*)u, (const T*)aux, (const T*)norm, (T*)dst, ny, nx, py, V};
    switch (mode) {
        case SEP_STORE: return cols_m<T, SEP_STORE>(p, count);
        case SEP_RATIO: return cols_m<T, SEP_RATIO>(p, count);
        case SEP_SUM: return cols_m<T, SEP_SUM>(p, count);
        case SEP_UPDATE: return cols_m<T, SEP_UPDATE>(p, count);
        default: return -1;
    }
}

template <typename T, int MODE, int TH, bool DIRECT>
int one_m(const Sep2dParams<T>& p, int frames) {
    const size_t lds = sep2d_lds(sizeof(T), TH, p.py, p.px, p.V, DIRECT);
    if (lds > kSep2dMaxLds) return -1;
    run_grid((p.nx + kColW - 1) / kColW, (p.ny + TH - 1) / TH, frames, kSepThreads, lds,
             [&](int t, int bx, int by, int bz, unsigned char* l, EmuSync& s) { sep2d_body<T, MODE, TH, DIRECT>(p, t, bx, by, bz, l, s); });
    return 0;
}
template <typename T, int TH, bool DIRECT>
int one_t(int mode, const Sep2dParams<T>& p, int frames) {
    switch (mode) {
        case SEP_STORE: return one_m<T, SEP_STORE, TH, DIRECT>(p, frames);
        case SEP_RATIO: return one_m<T, SEP_RATIO, TH, DIRECT>(p, frames);
        case SEP_SUM: return one_m<T, SEP_SUM, TH, DIRECT>(p, frames);
        case SEP_UPDATE: return one_m<T, SEP_UPDATE, TH, DIRECT>(p, frames);
        default: return -1;
    }
}
template <typename T>
int one(int mode, int th, int direct, const void* in, const void* uf, const void* vf, const void* aux, const void* norm, void* dst, int frames,
        int ny, int nx, int py, int px, int V) {
    if (frames < 1) return 0;
    const Sep2dParams<T> p{(const T*)in, (const T*)uf, direct ? nullptr : (const T*)vf, (const T*)aux, (const T*)norm, (T*)dst, ny, nx, py, px, V};
    if (th == 32) return direct ? one_t<T, 32, true>(mode, p, frames) : one_t<T, 32, false>(mode, p, frames);
    if (th == 64) return direct ? one_t<T, 64, true>(mode, p, frames) : one_t<T, 64, false>(mode, p, frames);
    return -1;
}

}  // namespace

// dtype: 0 float, 1 double (kernel_table.hpp DType).  A launch the launcher would refuse returns -1 and runs nothing.
extern "C" {
int emu_sep_rows(int dtype, const void* in, void* out, const void* v, int images, int ny, int nx, int px, int V, int in_div) {
    return dtype == 0 ? rows<float>(in, out, v, images, ny, nx, px, V, in_div) : rows<double>(in, out, v, images, ny, nx, px, V, in_div);
}
int emu_sep_cols(int dtype, int mode, const void* tmp, const void* u, const void* aux, const void* norm, void* dst, int count, int ny, int nx,
                 int py, int V) {
    return dtype == 0 ? cols<float>(mode, tmp, u, aux, norm, dst, count, ny, nx, py, V) : cols<double>(mode, tmp, u, aux, norm, dst, count, ny, nx, py, V);
}
// th: 32 or 64 (the device runs 64 in float only; the index logic is the same template); direct: taps uf = [V][px][8 nca], vf unused
int emu_sep2d(int dtype, int mode, int th, int direct, const void* in, const void* uf, const void* vf, const void* aux, const void* norm, void* dst,
              int frames, int ny, int nx, int py, int px, int V) {
    return dtype == 0 ? one<float>(mode, th, direct, in, uf, vf, aux, norm, dst, frames, ny, nx, py, px, V)
                      : one<double>(mode, th, direct, in, uf, vf, aux, norm, dst, frames, ny, nx, py, px, V);
}
size_t emu_sep_rows_lds(size_t esize, int px) { return sep_rows_lds(esize, px); }
size_t emu_sep_cols_lds(size_t esize, int py) { return sep_cols_lds(esize, py); }
size_t emu_sep2d_lds(size_t esize, int th, int py, int px, int V, int direct) { return sep2d_lds(esize, th, py, px, V, direct != 0); }
size_t emu_sep_max_lds() { return kSep2dMaxLds; }
int emu_sep2d_fits(size_t esize, int th, int py, int px, int V) { return sep2d_fits_tile(esize, th, py, px, V) ? 1 : 0; }
int emu_direct2d_fits(size_t esize, int th, int py, int px, int V) { return direct2d_fits_tile(esize, th, py, px, V) ? 1 : 0; }
int emu_two_pass_fits(size_t esize, int py, int px) { return sep_two_pass_fits_esize(esize, py, px) ? 1 : 0; }

// u [V][py], v [V][px] (written whether or not the PSFs are rank 1); returns 1 if every view is rank 1
int emu_rank1(const double* psfs, int V, int py, int px, double* u, double* v) {
    std::vector<double> uu, vv;
    const bool r = sep_rank1_factors(psfs, V, py, px, uu, vv);
    std::memcpy(u, uu.data(), uu.size() * sizeof(double));
    std::memcpy(v, vv.data(), vv.size() * sizeof(double));
    return r ? 1 : 0;
}
// uf [V][8 ceil(py / 8)], vf [V][8 ceil(px / 8)]
void emu_flipped_taps(const double* u, const double* v, int V, int py, int px, double* uf, double* vf) {
    std::vector<double> a, b;
    sep_flipped_taps(std::vector<double>(u, u + (size_t)V * py), std::vector<double>(v, v + (size_t)V * px), V, py, px, a, b);
    std::memcpy(uf, a.data(), a.size() * sizeof(double));
    std::memcpy(vf, b.data(), b.size() * sizeof(double));
}
// f [V][px][8 ceil(py / 8)]
void emu_direct_taps(const double* psfs, int V, int py, int px, double* f) {
    std::vector<double> a;
    sep_direct_taps(psfs, V, py, px, a);
    std::memcpy(f, a.data(), a.size() * sizeof(double));
}
// integ [V][py+1][px+1]
void emu_box_integral(const double* psfs, int V, int py, int px, double* integ) {
    std::vector<double> a;
    box_integral_images(psfs, V, py, px, a);
    std::memcpy(integ, a.data(), a.size() * sizeof(double));
}
// the grid of aux_box_norm: (ceil(nx / 256), ny) workgroups of 256 threads, one pixel each; `integ` is copied into a buffer of
// exactly its size first (the sanitizer watches its end)
void emu_box_norm(int dtype, const double* integ, void* out, int V, int py, int px, int ny, int nx) {
    const size_t n = (size_t)V * (py + 1) * (px + 1);
    double* I = (double*)std::malloc(n * sizeof(double));
    std::memcpy(I, integ, n * sizeof(double));
    for (int i = 0; i < ny; ++i)
        for (int bx = 0; bx < (nx + 255) / 256; ++bx)
            for (int t = 0; t < 256; ++t) {
                const int j = bx * 256 + t;
                if (j >= nx) continue;
                if (dtype == 0) ((float*)out)[(size_t)i * nx + j] = box_norm_pixel<float>(I, V, py, px, ny, nx, i, j);
                else ((double*)out)[(size_t)i * nx + j] = box_norm_pixel<double>(I, V, py, px, ny, nx, i, j);
            }
    std::free(I);
}
}
