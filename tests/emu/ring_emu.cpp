// Host emulator of the ring-statistics kernels (rescan_line_sted_amd/csrc/ring_kernels.hpp): the very same thread bodies, run
// thread by thread and workgroup by workgroup over the launch grids of ring_kernels.hip, the phases of a workgroup separated where
// the device has its barriers; and the host builder of the ring table.  TEST INFRASTRUCTURE ONLY -- built by tests/test_ring_cpu.py
// with g++ (-ffp-contract=off) and never loaded by the product.
#include <vector>

#include "../../rescan_line_sted_amd/csrc/ring_kernels.hpp"

using namespace rl;

namespace {

struct Accs {
    RingC v[kRingThreads][kRingMicro * kRingMicro];
    RingTw tw[kRingThreads];
    void zero() {
        for (auto& t : v)
            for (auto& c : t) c = RingC{0.0, 0.0};
    }
};

template <typename TA, typename TB>
void rows(const RingRowsParams<TA, TB>& p, int pairs) {
    std::vector<RingLds> lds(1);
    std::vector<Accs> acc(1);
    for (int pair = 0; pair < pairs; ++pair)
        for (int by = 0; by < (p.ny + kRingTile - 1) / kRingTile; ++by)
            for (int bx = 0; bx < (p.nx + kRingTile - 1) / kRingTile; ++bx) {
                const int n0 = bx * kRingTile, m0 = by * kRingTile;
                acc[0].zero();
                for (int t = 0; t < kRingThreads; ++t) acc[0].tw[t] = ring_tw_init(n0 + (t & 63), p.nx, t);
                for (int k0 = 0; k0 < p.nx; k0 += kRingKT) {
                    for (int t = 0; t < kRingThreads; ++t) ring_rows_load_thread(p, pair, m0, k0, acc[0].tw[t], lds[0], t);
                    for (int t = 0; t < kRingThreads; ++t) ring_mac_thread(lds[0], acc[0].v[t], t);
                }
                for (int t = 0; t < kRingThreads; ++t) ring_store_thread(p.out, p.ny, p.nx, pair, m0, n0, acc[0].v[t], t);
            }
}

void cols(const RingColsParams& p, int pairs) {
    std::vector<RingLds> lds(1);
    std::vector<Accs> acc(1);
    for (int pair = 0; pair < pairs; ++pair)
        for (int by = 0; by < (p.ny + kRingTile - 1) / kRingTile; ++by)
            for (int bx = 0; bx < (p.nx + kRingTile - 1) / kRingTile; ++bx) {
                const int n0 = bx * kRingTile, m0 = by * kRingTile;
                acc[0].zero();
                for (int t = 0; t < kRingThreads; ++t) acc[0].tw[t] = ring_tw_init(m0 + (t & 63), p.ny, t);
                for (int k0 = 0; k0 < p.ny; k0 += kRingKT) {
                    for (int t = 0; t < kRingThreads; ++t) ring_cols_load_thread(p, pair, n0, k0, acc[0].tw[t], lds[0], t);
                    for (int t = 0; t < kRingThreads; ++t) ring_mac_thread(lds[0], acc[0].v[t], t);
                }
                for (int t = 0; t < kRingThreads; ++t) ring_store_thread(p.out, p.ny, p.nx, pair, m0, n0, acc[0].v[t], t);
            }
}

void reduce(const RingReduceParams& p, int pairs) {
    static double s[4][kRingThreads];
    for (int pair = 0; pair < pairs; ++pair)
        for (int ring = 0; ring < p.n_rings; ++ring) {
            for (int t = 0; t < kRingThreads; ++t) {
                double v[4];
                ring_reduce_thread(p, pair, ring, t, v);
                for (int c = 0; c < 4; ++c) s[c][t] = v[c];
            }
            for (int h = kRingThreads / 2; h > 0; h >>= 1)
                for (int t = 0; t < kRingThreads; ++t) ring_tree_step(s, t, h);
            ring_reduce_write(p, pair, ring, s);
        }
}

// plain_twiddles(n) of ctx.hpp
std::vector<RingC> twiddles(int n) {
    std::vector<RingC> w((size_t)n);
    for (int m = 0; m < n; ++m) {
        const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)m / (long double)n;
        w[m].re = (double)cosl(a);
        w[m].im = (double)sinl(a);
    }
    return w;
}

template <typename TA, typename TB>
void stats(const TA* a, const int64_t* a_off, const TB* b, const int64_t* b_off, const double* scale, int pairs, int ny, int nx,
           int n_rings, double* out, double* f_out) {
    const std::vector<RingC> wx = twiddles(nx), wy = twiddles(ny);
    std::vector<RingC> t((size_t)pairs * ny * nx), f((size_t)pairs * ny * nx);
    std::vector<int> row_ptr, bins;
    ring_build_table(ny, nx, n_rings, row_ptr, bins);
    RingRowsParams<TA, TB> r{a, b, a_off, b_off, scale, wx.data(), t.data(), ny, nx};
    rows(r, pairs);
    RingColsParams c{t.data(), wy.data(), f.data(), ny, nx};
    cols(c, pairs);
    RingReduceParams q{f.data(), row_ptr.data(), bins.data(), out, ny, nx, n_rings};
    reduce(q, pairs);
    if (f_out)
        for (size_t i = 0; i < f.size(); ++i) {
            f_out[2 * i] = f[i].re;
            f_out[2 * i + 1] = f[i].im;
        }
}

}  // namespace

extern "C" {
int emu_ring_of_bin(int ky, int kx, int ny, int nx, int n_rings) { return ring_of_bin(ky, kx, ny, nx, n_rings); }
// ring of every bin [ny][nx] (n_rings for "none") from the CSR table, and the table's own consistency: returns 0, or a negative
// code when a bin is listed twice, out of order within its ring, or disagrees with ring_of_bin
int emu_ring_table(int ny, int nx, int n_rings, int* ring_out, int* row_ptr_out) {
    std::vector<int> row_ptr, bins;
    ring_build_table(ny, nx, n_rings, row_ptr, bins);
    for (size_t i = 0; i < (size_t)ny * nx; ++i) ring_out[i] = -1;
    for (int r = 0; r < n_rings; ++r)
        for (int i = row_ptr[r]; i < row_ptr[r + 1]; ++i) {
            if (bins[i] < 0 || bins[i] >= ny * nx || ring_out[bins[i]] != -1) return -1;
            if (i > row_ptr[r] && bins[i] <= bins[i - 1]) return -2;
            ring_out[bins[i]] = r;
        }
    for (int ky = 0; ky < ny; ++ky)
        for (int kx = 0; kx < nx; ++kx) {
            int& r = ring_out[(size_t)ky * nx + kx];
            const int want = ring_of_bin(ky, kx, ny, nx, n_rings);
            if (r == -1) {
                if (want < n_rings) return -3;
                r = n_rings;
            } else if (r != want) {
                return -4;
            }
        }
    for (int r = 0; r <= n_rings; ++r) row_ptr_out[r] = row_ptr[r];
    return 0;
}
int emu_ring_geometry(int* out) {
    out[0] = kRingThreads; out[1] = kRingTile; out[2] = kRingKT; out[3] = kRingFields; out[4] = (int)sizeof(RingLds);
    return 5;
}
// a / b: element type by dtype (0 f32, 1 f64); out [pairs][n_rings][5]; f_out (may be NULL) [pairs][ny][nx][2] = fft2(a + i s b)
void emu_ring_stats(const void* a, int a_dtype, const int64_t* a_off, const void* b, int b_dtype, const int64_t* b_off,
                    const double* scale, int pairs, int ny, int nx, int n_rings, double* out, double* f_out) {
    if (a_dtype == 0 && b_dtype == 0) stats((const float*)a, a_off, (const float*)b, b_off, scale, pairs, ny, nx, n_rings, out, f_out);
    else if (a_dtype == 0) stats((const float*)a, a_off, (const double*)b, b_off, scale, pairs, ny, nx, n_rings, out, f_out);
    else if (b_dtype == 0) stats((const double*)a, a_off, (const float*)b, b_off, scale, pairs, ny, nx, n_rings, out, f_out);
    else stats((const double*)a, a_off, (const double*)b, b_off, scale, pairs, ny, nx, n_rings, out, f_out);
}
}
