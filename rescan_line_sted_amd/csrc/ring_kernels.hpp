// ring_kernels.hpp -- per-ring sums over the 2-D spectra of two device-resident images (rl_ring_stats, include/rlsted.h): the host
// builder of the ring table, the workgroup bodies of ring_kernels.hip, written as host-compilable templates so that the CPU tests
// run the very same code (tests/emu/ring_emu.cpp), and the launchers.
//
// For a pair of real images a, b [ny][nx] of types TA, TB and a scale s, every value widened to float64 first:
//   PACK     Z = a + i (s b)                       formed while the first product loads its tiles (one rounding: s * b)
//   ROWS     T[y][k]  = sum_x Z[y][x] Wx[(x k) mod nx]          Wx[m] = exp(-2 pi i m / nx), the context's plain_twiddles(nx)
//   COLS     F[ky][k] = sum_y Wy[(ky y) mod ny] T[y][k]         Wy likewise for ny;  F = fft2(Z), unnormalised
//   REDUCE   per bin k of a ring, with Zm = F[-k]:  A = (F[k] + conj Zm) / 2 = fft2(a),  B = (F[k] - conj Zm) / (2 i) = fft2(s b);
//            fields 1..4 += |A|^2, |B|^2, Re(A conj B), |A - B|^2; field 0 = the ring's number of bins
//
// ROWS and COLS are complex float64 matrix products C[M][N] = sum_k A[m][k] B[k][n] on v_fma_f64 register tiles: a workgroup of
// kRingThreads = 256 threads owns a kRingTile x kRingTile = 64 x 64 tile of C, thread t = 16 ty + tx the 4 x 4 outputs
// (ty + 16 i, tx + 16 j); K is walked in steps of kRingKT = 16 through LDS (RingLds, 33 024 bytes).  Tiles may overhang the image:
// rows, columns and k past the end load as 0 and are not stored.  The twiddle operand is never a matrix in memory: the thread that
// fills LDS element (g, k) of it -- g its fixed row (COLS) or column (ROWS) of the image, k advancing by kRingKT per step -- keeps
// the table index (g k) mod n incrementally (RingTw), no sin / cos and no division in the loop.
// Order of an output's sum: k = 0, 1, ..., K - 1, per k
//     re = fma(a.re, b.re, re); re = fma(-a.im, b.im, re); im = fma(a.re, b.im, im); im = fma(a.im, b.re, im)
// -- explicit fma on the device and on the host alike, so the emulator's bits are the device's.  Chain length: 2 K roundings.
//
// REDUCE: one workgroup of kRingThreads threads per (pair, ring).  The ring table (ring_build_table: CSR, the bins of a ring in
// increasing order of ky * nx + kx) comes from the host, in exact integer arithmetic -- the device never computes a radius.  Sums
// are float64, in this order:
//   thread    s_t = (((0 + term_0) + term_1) + ...) over bins row_ptr[r] + t, + kRingThreads, ... of the ring, in table order
//   workgroup tree over the kRingThreads slots: s[t] = s[t] + s[t + h] for t < h, h = kRingThreads / 2, ..., 1
// No float atomics, no partials across workgroups; contraction off outside the explicit fma.  A pair's result depends on its own
// two images, the shape and the table only: never on the pairs beside it in the call.
//
// REDUCE BY SECTOR (rl_ring_sector_stats): the rings cut into n_sectors = S orientation sectors, cell c = ring * S + sector
// (sector_of_bin, ring_build_sector_table: CSR over the cells, a cell's bins in increasing ky * nx + kx; the orientation is decided
// on the host, ties in integers -- the device never computes an angle).  One workgroup of kRingThreads threads, four wave64s, per
// (pair, ring); a WAVE owns a cell: wave w takes sectors w, w + 4, ... of the ring.  Per cell, in float64:
//   lane      s_l = (((0 + term_0) + term_1) + ...) over bins cell_ptr[c] + l, + kRingWave, ... of the cell, in table order; the
//             terms are those of REDUCE (ring_sum_bins, the one body of both)
//   wave tree over the kRingWave lanes: v[l] = v[l] + v[l + h] for l < h, h = kRingWave / 2, ..., 1 (lane l reads lane l + h in
//             registers; the lanes at and above h compute values nobody reads)
//   lane 0    stores field 0 = cell_ptr[c + 1] - cell_ptr[c] and the four sums; an empty cell is five zeros.
// No workgroup barrier, no LDS, no float atomics, no partials across waves.
#pragma once
#include "fft_core.hpp"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rl {

constexpr int kRingThreads = 256;   // threads per workgroup (four waves), all three kernels
constexpr int kRingTile = 64;       // rows and columns of C per workgroup
constexpr int kRingKT = 16;         // k per LDS step
constexpr int kRingMicro = 4;       // a thread's outputs: kRingMicro x kRingMicro, strided by 16
constexpr int kRingPitchA = kRingTile + 1;   // ROWS fills A k-fastest: the odd pitch spreads a wave's 16 k over the banks
constexpr int kRingFields = 5;
constexpr int kRingWave = 64;       // lanes of a wave: the sector reduce gives a wave a cell
constexpr int kRingMaxSectors = 64;
constexpr int kRingMaxN = 4096;     // longest image side (products g * k stay below 2^31)

struct alignas(16) RingC {
    double re, im;
};

struct RingLds {
    RingC a[kRingKT][kRingPitchA];   // A[m][k] as a[k][m]
    RingC b[kRingKT][kRingTile];     // B[k][n]
};

// table indices (g k) mod n of the four twiddle elements thread t fills per step: k = k0 + (t >> 6) + 4 i, g fixed
struct RingTw {
    int idx[4];   // -1: g is past the image (the element is 0)
    int step;     // (kRingKT g) mod n
};

template <typename TA, typename TB>
struct RingRowsParams {
    const TA* a;               // base of the a images
    const TB* b;
    const int64_t* a_off;      // [pairs] element offsets (device)
    const int64_t* b_off;
    const double* scale;       // [pairs]
    const RingC* w;            // Wx [nx]
    RingC* out;                // T [pairs][ny][nx]
    int ny, nx;
};

struct RingColsParams {
    const RingC* in;           // T [pairs][ny][nx]
    const RingC* w;            // Wy [ny]
    RingC* out;                // F [pairs][ny][nx]
    int ny, nx;
};

struct RingReduceParams {
    const RingC* f;            // F [pairs][ny][nx]
    const int* row_ptr;        // [n_rings + 1]
    const int* bins;           // [row_ptr[n_rings]]  ky * nx + kx
    double* out;               // [pairs][n_rings][kRingFields]
    int ny, nx, n_rings;
};

struct RingSectorParams {
    const RingC* f;            // F [pairs][ny][nx]
    const int* cell_ptr;       // [n_rings * n_sectors + 1]
    const int* bins;           // [cell_ptr[n_rings * n_sectors]]  ky * nx + kx
    double* out;               // [pairs][n_rings][n_sectors][kRingFields]
    int ny, nx, n_rings, n_sectors;
};

RL_HD RingTw ring_tw_init(int g, int n, int t) {
    RingTw tw;
    const int64_t k = t >> 6;
    tw.step = g < n ? (int)(((int64_t)kRingKT * g) % n) : 0;
    tw.idx[0] = g < n ? (int)((g * k) % n) : -1;
    tw.idx[1] = g < n ? (int)((g * (k + 4)) % n) : -1;
    tw.idx[2] = g < n ? (int)((g * (k + 8)) % n) : -1;
    tw.idx[3] = g < n ? (int)((g * (k + 12)) % n) : -1;
    return tw;
}

// one twiddle element: W[idx] (0 where g or k is past the image) -> *dst, then idx moves on by a step
RL_HD void ring_tw_one(const RingC* w, int& idx, int step, int n, int k, RingC* dst) {
    double re = 0.0, im = 0.0;
    if (idx >= 0) {
        if (k < n) {
            re = w[idx].re;
            im = w[idx].im;
        }
        idx += step;
        if (idx >= n) idx -= n;
    }
    dst->re = re;
    dst->im = im;
}

// the thread's four twiddle elements of the step at k0 -> dst[k][g - g0] (dst pitch in elements)
RL_HD void ring_tw_fill(const RingC* w, RingTw& tw, int n, int k0, RingC* dst, int pitch, int t) {
    const int kk = t >> 6, c = t & 63;
    ring_tw_one(w, tw.idx[0], tw.step, n, k0 + kk, dst + kk * pitch + c);
    ring_tw_one(w, tw.idx[1], tw.step, n, k0 + kk + 4, dst + (kk + 4) * pitch + c);
    ring_tw_one(w, tw.idx[2], tw.step, n, k0 + kk + 8, dst + (kk + 8) * pitch + c);
    ring_tw_one(w, tw.idx[3], tw.step, n, k0 + kk + 12, dst + (kk + 12) * pitch + c);
}

// ROWS, thread t of the workgroup of tile (m0, n0) of pair `pair`: the LDS step at k0 (PACK happens here)
template <typename TA, typename TB>
RL_HD void ring_rows_load_thread(const RingRowsParams<TA, TB>& p, int pair, int m0, int k0, RingTw& tw, RingLds& lds, int t) {
#pragma clang fp contract(off)
    const TA* a = p.a + p.a_off[pair];
    const TB* b = p.b + p.b_off[pair];
    const double s = p.scale[pair];
    for (int i = 0; i < 4; ++i) {
        const int e = t + kRingThreads * i, kk = e & (kRingKT - 1), m = e >> 4;
        const int y = m0 + m, x = k0 + kk;
        double re = 0.0, im = 0.0;
        if (y < p.ny && x < p.nx) {
            const size_t o = (size_t)y * p.nx + x;
            re = (double)a[o];
            im = s * (double)b[o];
        }
        lds.a[kk][m].re = re;
        lds.a[kk][m].im = im;
    }
    ring_tw_fill(p.w, tw, p.nx, k0, &lds.b[0][0], kRingTile, t);
}

// COLS, likewise
RL_HD void ring_cols_load_thread(const RingColsParams& p, int pair, int n0, int k0, RingTw& tw, RingLds& lds, int t) {
    const RingC* src = p.in + (size_t)pair * p.ny * p.nx;
    ring_tw_fill(p.w, tw, p.ny, k0, &lds.a[0][0], kRingPitchA, t);
    for (int i = 0; i < 4; ++i) {
        const int kk = (t >> 6) + 4 * i, n = t & 63;
        const int y = k0 + kk, x = n0 + n;
        double re = 0.0, im = 0.0;
        if (y < p.ny && x < p.nx) {
            const RingC* e = src + (size_t)y * p.nx + x;
            re = e->re;
            im = e->im;
        }
        lds.b[kk][n].re = re;
        lds.b[kk][n].im = im;
    }
}

// the kRingKT rank-1 updates of one LDS step on the thread's 4 x 4 outputs acc[4 i + j]
RL_HD void ring_mac_thread(const RingLds& lds, RingC* acc, int t) {
    const int tx = t & 15, ty = t >> 4;
#pragma unroll 4
    for (int kk = 0; kk < kRingKT; ++kk) {
        RingC a[kRingMicro], b[kRingMicro];
        for (int i = 0; i < kRingMicro; ++i) a[i] = lds.a[kk][ty + 16 * i];
        for (int j = 0; j < kRingMicro; ++j) b[j] = lds.b[kk][tx + 16 * j];
        for (int i = 0; i < kRingMicro; ++i)
            for (int j = 0; j < kRingMicro; ++j) {
                RingC& c = acc[kRingMicro * i + j];
                c.re = fma(a[i].re, b[j].re, c.re);
                c.re = fma(-a[i].im, b[j].im, c.re);
                c.im = fma(a[i].re, b[j].im, c.im);
                c.im = fma(a[i].im, b[j].re, c.im);
            }
    }
}

RL_HD void ring_store_thread(RingC* out, int ny, int nx, int pair, int m0, int n0, const RingC* acc, int t) {
    const int tx = t & 15, ty = t >> 4;
    RingC* dst = out + (size_t)pair * ny * nx;
    for (int i = 0; i < kRingMicro; ++i)
        for (int j = 0; j < kRingMicro; ++j) {
            const int y = m0 + ty + 16 * i, x = n0 + tx + 16 * j;
            if (y < ny && x < nx) dst[(size_t)y * nx + x] = acc[kRingMicro * i + j];
        }
}

// the sums of fields 1..4 over the table entries begin, begin + stride, ... below end, in that order -> s[0..3]
RL_HD void ring_sum_bins(const RingC* f, int ny, int nx, const int* bins, int begin, int end, int stride, double* s) {
#pragma clang fp contract(off)
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (int i = begin; i < end; i += stride) {
        const int bin = bins[i], ky = bin / nx, kx = bin - ky * nx;
        const int my = ky ? ny - ky : 0, mx = kx ? nx - kx : 0;
        const RingC z = f[bin], zm = f[(size_t)my * nx + mx];
        const double ar = 0.5 * (z.re + zm.re), ai = 0.5 * (z.im - zm.im);
        const double br = 0.5 * (z.im + zm.im), bi = 0.5 * (zm.re - z.re);
        const double dr = ar - br, di = ai - bi;
        s1 = s1 + fma(ai, ai, ar * ar);
        s2 = s2 + fma(bi, bi, br * br);
        s3 = s3 + fma(ai, bi, ar * br);
        s4 = s4 + fma(di, di, dr * dr);
    }
    s[0] = s1;
    s[1] = s2;
    s[2] = s3;
    s[3] = s4;
}

// REDUCE, thread t of the workgroup of (pair, ring): its sums of fields 1..4 -> s[0..3]
RL_HD void ring_reduce_thread(const RingReduceParams& p, int pair, int ring, int t, double* s) {
    ring_sum_bins(p.f + (size_t)pair * p.ny * p.nx, p.ny, p.nx, p.bins, p.row_ptr[ring] + t, p.row_ptr[ring + 1], kRingThreads, s);
}

// one step of the workgroup tree on the four fields' slots s[field][kRingThreads]
RL_HD void ring_tree_step(double (*s)[kRingThreads], int t, int h) {
#pragma clang fp contract(off)
    if (t < h)
        for (int c = 0; c < 4; ++c) s[c][t] = s[c][t] + s[c][t + h];
}

RL_HD void ring_reduce_write(const RingReduceParams& p, int pair, int ring, const double (*s)[kRingThreads]) {
    double* o = p.out + ((size_t)pair * p.n_rings + ring) * kRingFields;
    o[0] = (double)(p.row_ptr[ring + 1] - p.row_ptr[ring]);
    for (int c = 0; c < 4; ++c) o[1 + c] = s[c][0];
}

// REDUCE BY SECTOR, lane l of the wave that owns cell (ring, sector) of `pair`: its sums of fields 1..4 -> v[0..3]
RL_HD void ring_sector_lane(const RingSectorParams& p, int pair, int ring, int sector, int lane, double* v) {
    const int c = ring * p.n_sectors + sector;
    ring_sum_bins(p.f + (size_t)pair * p.ny * p.nx, p.ny, p.nx, p.bins, p.cell_ptr[c] + lane, p.cell_ptr[c + 1], kRingWave, v);
}

// one step of the wave tree on a lane's four sums: `up` holds those of the lane h above it
RL_HD void ring_wave_step(double* v, const double* up) {
#pragma clang fp contract(off)
    for (int c = 0; c < 4; ++c) v[c] = v[c] + up[c];
}

// lane 0 of the wave, after the tree
RL_HD void ring_sector_write(const RingSectorParams& p, int pair, int ring, int sector, const double* v) {
    const int c = ring * p.n_sectors + sector;
    double* o = p.out + ((size_t)pair * p.n_rings * p.n_sectors + c) * kRingFields;
    o[0] = (double)(p.cell_ptr[c + 1] - p.cell_ptr[c]);
    for (int k = 0; k < 4; ++k) o[1 + k] = v[k];
}

// ---- the ring table (host).  ring(ky, kx) = isqrt(4 R^2 q) / M in exact integers, q = (sy nx)^2 + (sx ny)^2, M = ny nx, sy / sx
// the signed frequencies: the largest r with (r M)^2 <= 4 R^2 q.  4 R^2 q reaches 2^71 at 4096 x 4096: 128-bit compares.
inline int ring_of_bin(int ky, int kx, int ny, int nx, int n_rings) {
    typedef unsigned __int128 u128;
    const int64_t sy = ky <= ny / 2 ? ky : ky - ny, sx = kx <= nx / 2 ? kx : kx - nx;
    const uint64_t q = (uint64_t)(sy * nx) * (uint64_t)(sy * nx) + (uint64_t)(sx * ny) * (uint64_t)(sx * ny);
    const u128 x = (u128)4 * (u128)((uint64_t)n_rings * (uint64_t)n_rings) * (u128)q;
    const uint64_t m = (uint64_t)ny * (uint64_t)nx;
    int64_t r = (int64_t)(2.0 * (double)n_rings * std::sqrt((double)q) / (double)m);   // a first guess, then exact
    if (r < 0) r = 0;
    while ((u128)((uint64_t)(r + 1) * m) * (u128)((uint64_t)(r + 1) * m) <= x) ++r;
    while (r > 0 && (u128)((uint64_t)r * m) * (u128)((uint64_t)r * m) > x) --r;
    return r > 0x7fffffff ? 0x7fffffff : (int)r;
}

// CSR over rings 0 .. n_rings - 1: row_ptr [n_rings + 1], bins = ky * nx + kx in increasing order within a ring; bins whose ring
// is >= n_rings belong to none
inline void ring_build_table(int ny, int nx, int n_rings, std::vector<int>& row_ptr, std::vector<int>& bins) {
    std::vector<int> ring((size_t)ny * nx);
    row_ptr.assign((size_t)n_rings + 1, 0);
    for (int ky = 0; ky < ny; ++ky)
        for (int kx = 0; kx < nx; ++kx) {
            const int r = ring_of_bin(ky, kx, ny, nx, n_rings);
            ring[(size_t)ky * nx + kx] = r;
            if (r < n_rings) ++row_ptr[r + 1];
        }
    for (int r = 0; r < n_rings; ++r) row_ptr[r + 1] += row_ptr[r];
    bins.assign((size_t)row_ptr[n_rings], 0);
    std::vector<int> at(row_ptr.begin(), row_ptr.end() - 1);
    for (size_t i = 0; i < ring.size(); ++i)
        if (ring[i] < n_rings) bins[(size_t)at[ring[i]]++] = (int)i;
}

// ---- the sector of a bin (host; the definition: include/rlsted.h, rl_ring_sector_stats).  With Y = sy nx, X = sx ny folded into the
// upper half plane, theta = atan2(Y, X) in [0, pi) and sector = floor(S theta / pi + 1/2) mod S.  A bin lies exactly on a sector
// boundary only where that boundary is a multiple of 45 degrees (any other boundary has an irrational tangent): those directions
// -- Y = 0, X = 0, |Y| = |X| -- are decided in integers, floor((S + 2) / 4), floor((S + 1) / 2), floor((3 S + 2) / 4), which puts
// a tie into the upper sector.  Everything else goes through long double; a bin closer to a boundary than 2^-30 sets *too_close
// instead of being guessed (none is known: the closest seen is 7.8e-5, at 160 x 160 with S = 4).
inline int sector_of_bin(int ky, int kx, int ny, int nx, int n_sectors, bool* too_close) {
    const int64_t S = n_sectors;
    int64_t Y = (int64_t)(ky <= ny / 2 ? ky : ky - ny) * nx, X = (int64_t)(kx <= nx / 2 ? kx : kx - nx) * ny;
    if (Y < 0 || (Y == 0 && X < 0)) {
        Y = -Y;
        X = -X;
    }
    if (Y == 0) return 0;   // 0 degrees, and the DC bin
    if (X == 0) return (int)(((S + 1) / 2) % S);
    if (Y == X) return (int)(((S + 2) / 4) % S);
    if (Y == -X) return (int)(((3 * S + 2) / 4) % S);
    const long double u = (long double)S * atan2l((long double)Y, (long double)X) / 3.14159265358979323846264338327950288L + 0.5L;
    const long double f = floorl(u);
    if (u - f < 0x1p-30L || f + 1.0L - u < 0x1p-30L) *too_close = true;
    return (int)((int64_t)f % S);
}

// CSR over the cells c = ring * n_sectors + sector: cell_ptr [n_rings * n_sectors + 1], bins = ky * nx + kx in increasing order
// within a cell; bins whose ring is >= n_rings belong to none.  false: a bin too close to a sector boundary (sector_of_bin)
inline bool ring_build_sector_table(int ny, int nx, int n_rings, int n_sectors, std::vector<int>& cell_ptr, std::vector<int>& bins) {
    const size_t cells = (size_t)n_rings * n_sectors;
    std::vector<int> cell((size_t)ny * nx, -1);
    cell_ptr.assign(cells + 1, 0);
    bool too_close = false;
    for (int ky = 0; ky < ny; ++ky)
        for (int kx = 0; kx < nx; ++kx) {
            const int r = ring_of_bin(ky, kx, ny, nx, n_rings);
            if (r >= n_rings) continue;
            const int c = r * n_sectors + sector_of_bin(ky, kx, ny, nx, n_sectors, &too_close);
            cell[(size_t)ky * nx + kx] = c;
            ++cell_ptr[(size_t)c + 1];
        }
    for (size_t c = 0; c < cells; ++c) cell_ptr[c + 1] += cell_ptr[c];
    bins.assign((size_t)cell_ptr[cells], 0);
    std::vector<int> at(cell_ptr.begin(), cell_ptr.end() - 1);
    for (size_t i = 0; i < cell.size(); ++i)
        if (cell[i] >= 0) bins[(size_t)at[(size_t)cell[i]]++] = (int)i;
    return !too_close;
}

// ---- launchers (ring_kernels.hip, ring_sector_kernels.hip): `pairs` pairs on stream s; dtypes RL_F32 / RL_F64 of the two image buffers
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t ring_rows(int a_dtype, int b_dtype, const void* a, const void* b, const int64_t* a_off, const int64_t* b_off,
                     const double* scale, const void* wx, void* t_out, int ny, int nx, int pairs, hipStream_t s);
hipError_t ring_cols(const void* t_in, const void* wy, void* f_out, int ny, int nx, int pairs, hipStream_t s);
hipError_t ring_reduce(const void* f, const int* row_ptr, const int* bins, double* out, int ny, int nx, int n_rings, int pairs,
                       hipStream_t s);
hipError_t ring_reduce_sectors(const void* f, const int* cell_ptr, const int* bins, double* out, int ny, int nx, int n_rings,
                               int n_sectors, int pairs, hipStream_t s);
#endif

}  // namespace rl
