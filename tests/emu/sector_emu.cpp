// Host emulator of the angle-resolved ring statistics (rescan_line_sted_amd/csrc/ring_kernels.hpp, ring_sector_kernels.hip): the
// host builder of the sector table, and the body of k_ring_reduce_sectors run lane by lane, wave by wave and workgroup by
// workgroup over its launch grid, on F from the emulated ROWS and COLS -- ring_emu.cpp is included whole, so this library also
// carries emu_ring_stats, the emulated rl_ring_stats the sector sums are compared with.  TEST INFRASTRUCTURE ONLY -- built by
// tests/test_sector_cpu.py with g++ (-ffp-contract=off), as a shared library and, with -DSECTOR_EMU_MAIN, as a stand-alone
// program for the sanitizers; never loaded by the product.
#include "ring_emu.cpp"

#include <cstdio>

namespace {

// k_ring_reduce_sectors: grid (n_rings, pairs), kRingThreads / kRingWave waves of kRingWave lanes; __shfl_down(v, h) gives lane l
// the value of lane l + h, its own where l + h is past the wave
void reduce_sectors(const RingSectorParams& p, int pairs) {
    double v[kRingWave][4], up[kRingWave][4];
    for (int pair = 0; pair < pairs; ++pair)
        for (int ring = 0; ring < p.n_rings; ++ring)
            for (int wave = 0; wave < kRingThreads / kRingWave; ++wave)
                for (int sector = wave; sector < p.n_sectors; sector += kRingThreads / kRingWave) {
                    for (int l = 0; l < kRingWave; ++l) ring_sector_lane(p, pair, ring, sector, l, v[l]);
                    for (int h = kRingWave / 2; h > 0; h >>= 1) {
                        for (int l = 0; l < kRingWave; ++l)
                            for (int c = 0; c < 4; ++c) up[l][c] = v[l + h < kRingWave ? l + h : l][c];
                        for (int l = 0; l < kRingWave; ++l) ring_wave_step(v[l], up[l]);
                    }
                    ring_sector_write(p, pair, ring, sector, v[0]);
                }
}

template <typename TA, typename TB>
int sector_stats(const TA* a, const int64_t* a_off, const TB* b, const int64_t* b_off, const double* scale, int pairs, int ny, int nx,
                 int n_rings, int n_sectors, double* out) {
    const std::vector<RingC> wx = twiddles(nx), wy = twiddles(ny);
    std::vector<RingC> t((size_t)pairs * ny * nx), f((size_t)pairs * ny * nx);
    std::vector<int> cell_ptr, bins;
    if (!ring_build_sector_table(ny, nx, n_rings, n_sectors, cell_ptr, bins)) return -1;
    RingRowsParams<TA, TB> r{a, b, a_off, b_off, scale, wx.data(), t.data(), ny, nx};
    rows(r, pairs);
    RingColsParams c{t.data(), wy.data(), f.data(), ny, nx};
    cols(c, pairs);
    RingSectorParams q{f.data(), cell_ptr.data(), bins.data(), out, ny, nx, n_rings, n_sectors};
    reduce_sectors(q, pairs);
    return 0;
}

}  // namespace

extern "C" {
// the sector of a bin, -1 where the builder would refuse to decide
int emu_sector_of_bin(int ky, int kx, int ny, int nx, int n_sectors) {
    bool too_close = false;
    const int s = sector_of_bin(ky, kx, ny, nx, n_sectors, &too_close);
    return too_close ? -1 : s;
}
// cell = ring * n_sectors + sector of every bin [ny][nx] (n_rings * n_sectors for "none") from the CSR table, and the table's own
// consistency: returns 0, or a negative code when the builder refuses, a bin is listed twice, out of order within its cell, or
// disagrees with ring_of_bin / sector_of_bin
int emu_sector_table(int ny, int nx, int n_rings, int n_sectors, int* cell_out, int* cell_ptr_out) {
    std::vector<int> cell_ptr, bins;
    if (!ring_build_sector_table(ny, nx, n_rings, n_sectors, cell_ptr, bins)) return -5;
    const int cells = n_rings * n_sectors;
    if ((int)cell_ptr.size() != cells + 1 || cell_ptr[0] != 0 || (size_t)cell_ptr[cells] != bins.size()) return -6;
    for (size_t i = 0; i < (size_t)ny * nx; ++i) cell_out[i] = -1;
    for (int c = 0; c < cells; ++c)
        for (int i = cell_ptr[c]; i < cell_ptr[c + 1]; ++i) {
            if (bins[i] < 0 || bins[i] >= ny * nx || cell_out[bins[i]] != -1) return -1;
            if (i > cell_ptr[c] && bins[i] <= bins[i - 1]) return -2;
            cell_out[bins[i]] = c;
        }
    for (int ky = 0; ky < ny; ++ky)
        for (int kx = 0; kx < nx; ++kx) {
            int& c = cell_out[(size_t)ky * nx + kx];
            const int r = ring_of_bin(ky, kx, ny, nx, n_rings);
            bool too_close = false;
            if (c == -1) {
                if (r < n_rings) return -3;
                c = cells;
            } else if (r >= n_rings || c != r * n_sectors + sector_of_bin(ky, kx, ny, nx, n_sectors, &too_close)) {
                return -4;
            }
        }
    for (int c = 0; c <= cells; ++c) cell_ptr_out[c] = cell_ptr[c];
    return 0;
}
// a / b: element type by dtype (0 f32, 1 f64); out [pairs][n_rings][n_sectors][5]
int emu_sector_stats(const void* a, int a_dtype, const int64_t* a_off, const void* b, int b_dtype, const int64_t* b_off,
                     const double* scale, int pairs, int ny, int nx, int n_rings, int n_sectors, double* out) {
    if (a_dtype == 0 && b_dtype == 0)
        return sector_stats((const float*)a, a_off, (const float*)b, b_off, scale, pairs, ny, nx, n_rings, n_sectors, out);
    if (a_dtype == 0) return sector_stats((const float*)a, a_off, (const double*)b, b_off, scale, pairs, ny, nx, n_rings, n_sectors, out);
    if (b_dtype == 0) return sector_stats((const double*)a, a_off, (const float*)b, b_off, scale, pairs, ny, nx, n_rings, n_sectors, out);
    return sector_stats((const double*)a, a_off, (const double*)b, b_off, scale, pairs, ny, nx, n_rings, n_sectors, out);
}
}

#ifdef SECTOR_EMU_MAIN
// The stand-alone program of the sanitizer run: the table builder over shapes and sector counts with the checks of
// emu_sector_table, and the emulated statistics of pseudo-random pairs at odd offsets whose sector sums must give the ring
// statistics' bin counts exactly and their sums closely.  Prints "ok <tables> <cells>" and returns 0, or says what failed.
int main() {
    const int shapes[][2] = {{2, 2}, {8, 8}, {24, 40}, {37, 50}, {65, 64}, {96, 160}};
    const int sectors[] = {1, 2, 3, 5, 6, 12, 64};
    long tables = 0, cells = 0;
    for (const auto& sh : shapes)
        for (int S : sectors)
            for (int extra = 0; extra < 2; ++extra) {
                const int ny = sh[0], nx = sh[1], R = std::min(ny, nx) / 2 + 3 * extra;
                std::vector<int> cell((size_t)ny * nx), cell_ptr((size_t)R * S + 1);
                const int rc = emu_sector_table(ny, nx, R, S, cell.data(), cell_ptr.data());
                if (rc != 0) {
                    std::printf("table %d x %d R %d S %d: %d\n", ny, nx, R, S, rc);
                    return 1;
                }
                ++tables;
                cells += (long)R * S;
            }
    unsigned state = 12345u;
    auto next = [&state]() {
        state = state * 1664525u + 1013904223u;
        return (double)(state >> 20);
    };
    const int cases[][3] = {{8, 8, 12}, {37, 50, 6}, {24, 40, 5}, {66, 70, 1}};
    for (const auto& cs : cases) {
        const int ny = cs[0], nx = cs[1], S = cs[2], R = std::min(ny, nx) / 2, pix = ny * nx, pairs = 2;
        std::vector<float> a((size_t)2 * pix + 3);
        std::vector<double> b((size_t)pix + 1);
        for (auto& x : a) x = (float)next();
        for (auto& x : b) x = next();
        const int64_t a_off[2] = {1, (int64_t)pix + 3}, b_off[2] = {1, 1};
        const double scale[2] = {1.0, 0.37};
        std::vector<double> sec((size_t)pairs * R * S * kRingFields, -1.0), ring((size_t)pairs * R * kRingFields, -1.0);
        if (emu_sector_stats(a.data(), 0, a_off, b.data(), 1, b_off, scale, pairs, ny, nx, R, S, sec.data()) != 0) {
            std::printf("stats %d x %d S %d refused\n", ny, nx, S);
            return 1;
        }
        emu_ring_stats(a.data(), 0, a_off, b.data(), 1, b_off, scale, pairs, ny, nx, R, ring.data(), nullptr);
        for (int p = 0; p < pairs; ++p)
            for (int r = 0; r < R; ++r)
                for (int k = 0; k < kRingFields; ++k) {
                    double sum = 0.0;
                    for (int s = 0; s < S; ++s) sum += sec[(((size_t)p * R + r) * S + s) * kRingFields + k];
                    const double* row = &ring[((size_t)p * R + r) * kRingFields];
                    const double want = row[k], mag = 2.0 * (row[1] + row[2]);   // every term of fields 3 and 4 is within |A|^2 + |B|^2 twice
                    if (k == 0 ? sum != want : !(std::fabs(sum - want) <= 1e-12 * mag)) {
                        std::printf("%d x %d S %d pair %d ring %d field %d: %.17g over sectors, %.17g\n", ny, nx, S, p, r, k, sum, want);
                        return 1;
                    }
                }
    }
    std::printf("ok %ld %ld\n", tables, cells);
    return 0;
}
#endif
