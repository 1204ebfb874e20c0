// sep_taps.hpp -- the host code that feeds the stencils of sep_kernels.hpp: the rank-1 test of a plan's PSFs, the tap tables of
// the three forms and the integral images of the box normaliser (aux_kernels.hpp box_norm_pixel).  Plain C++ on float64 vectors,
// called by deconv_build (rlsted.cpp) and by the host emulator of the CPU tests (tests/emu/sep_emu.cpp).
// psfs: [V][py][px] float64, p[a][b] = psfs[(v * py + a) * px + b].
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace rl {

// Is every view rank 1 (p = u v^T to 1e-12 of its largest element)?  If so u [V][py] and vv [V][px] hold the factors: cross
// approximation through the largest element (u its column, vv its row divided by it), exact for a rank-1 matrix.  A view without a
// non-zero finite maximum is not rank 1.
inline bool sep_rank1_factors(const double* psfs, size_t V, size_t py, size_t px, std::vector<double>& u, std::vector<double>& vv) {
    u.assign(V * py, 0.0);
    vv.assign(V * px, 0.0);
    bool rank1 = true;
    for (size_t v = 0; v < V && rank1; ++v) {
        const double* p = psfs + v * py * px;
        size_t a0 = 0, b0 = 0;
        double pmax = 0.0;
        for (size_t a = 0; a < py; ++a)
            for (size_t b = 0; b < px; ++b)
                if (std::fabs(p[a * px + b]) > pmax) { pmax = std::fabs(p[a * px + b]); a0 = a; b0 = b; }
        if (!(pmax > 0.0)) { rank1 = false; break; }
        // cross approximation through the largest element: exact for a rank-1 matrix
        for (size_t a = 0; a < py; ++a) u[v * py + a] = p[a * px + b0];
        for (size_t b = 0; b < px; ++b) vv[v * px + b] = p[a0 * px + b] / p[a0 * px + b0];
        for (size_t a = 0; a < py && rank1; ++a)
            for (size_t b = 0; b < px; ++b)
                if (std::fabs(p[a * px + b] - u[v * py + a] * vv[v * px + b]) > 1e-12 * pmax) { rank1 = false; break; }
    }
    return rank1;
}

// the one-kernel form's taps: uf [V][8 ceil(py / 8)], vf [V][8 ceil(px / 8)], FLIPPED (f[k] = taps[n - 1 - k]) and zero padded
inline void sep_flipped_taps(const std::vector<double>& u, const std::vector<double>& vv, size_t V, size_t py, size_t px,
                             std::vector<double>& uf, std::vector<double>& vf) {
    const size_t pyp = (py + 7) / 8 * 8, pxp = (px + 7) / 8 * 8;
    uf.assign(V * pyp, 0.0);
    vf.assign(V * pxp, 0.0);
    for (size_t v = 0; v < V; ++v) {
        for (size_t k = 0; k < py; ++k) uf[v * pyp + k] = u[v * py + (py - 1 - k)];
        for (size_t k = 0; k < px; ++k) vf[v * pxp + k] = vv[v * px + (px - 1 - k)];
    }
}

// the direct 2-D stencil's taps: f [V][px][8 ceil(py / 8)], F[l][k] = p[py-1-k][px-1-l], zero padded along k
inline void sep_direct_taps(const double* psfs, size_t V, size_t py, size_t px, std::vector<double>& f) {
    const size_t pyp = (py + 7) / 8 * 8;
    f.assign(V * px * pyp, 0.0);
    for (size_t v = 0; v < V; ++v)
        for (size_t l = 0; l < px; ++l)
            for (size_t k = 0; k < py; ++k) f[(v * px + l) * pyp + k] = psfs[(v * py + (py - 1 - k)) * px + (px - 1 - l)];
}

// integral images of the PSFs: integ [V][py+1][px+1], I[a][b] = sum of p[a' < a][b' < b] (row 0 and column 0 are zero); every entry
// is a float64 sum built from a running row sum (depth px) added to the entry above (depth py)
inline void box_integral_images(const double* psfs, size_t V, size_t py, size_t px, std::vector<double>& integ) {
    const size_t stride = (py + 1) * (px + 1);
    integ.assign(V * stride, 0.0);
    for (size_t v = 0; v < V; ++v)
        for (size_t a = 0; a < py; ++a) {
            double row = 0.0;   // running sum of PSF row a
            for (size_t b = 0; b < px; ++b) {
                row += psfs[(v * py + a) * px + b];
                integ[v * stride + (a + 1) * (px + 1) + (b + 1)] = integ[v * stride + a * (px + 1) + (b + 1)] + row;
            }
        }
}

}  // namespace rl
