// tile_layout.hpp -- the layout of overlapping tiles over one image axis and their blend weights (rl_tile_axis, rl_tile_weights,
// include/rlsted.h).  Host code only, exact integer and float64 arithmetic, no dependency beyond the
// standard library: the C ABI (tile_api.cpp), the CPU tests (tests/emu/tile_layout_test.cpp) and the emulation of the kernels
// (tests/emu/tile_emu.cpp) compile this very file; tests/tile_reference.py is its numpy twin, bit for bit.
//
// One axis of N pixels, tile t, overlap o, margin m (0 <= m, 2 m < o < t):
//   N <= t   one tile of length N at origin 0
//   N >  t   s = t - o, n = ceil((N - t) / s) + 1 tiles of length t at a_i = (i (N - t)) / (n - 1) (integer division): a_0 = 0,
//            a_{n-1} = N - t, consecutive tiles overlap by at least o; more than two tiles may cover a pixel
// Raw weight of tile i at local index j: min(1, left, right) with
//   left  (i > 0)      clamp((j - m + 0.5) / R, 0, 1),        R  = (a_{i-1} + t - a_i) - 2 m
//   right (i < n - 1)  clamp((t - m - j - 0.5) / R', 0, 1),   R' = (a_i + t - a_{i+1}) - 2 m
// (a side on the image border has neither margin nor ramp).  W[g] = the raw weights of the tiles that cover g summed in increasing
// i, from 0.0; the normalised weight w_i(j) / W[a_i + j] is what the device multiplies with.
#pragma once
#include <cstdint>
#include <vector>

namespace rl {

enum TileLayoutError { TILE_OK = 0, TILE_BAD_SIZE = 1, TILE_BAD_OVERLAP = 2, TILE_BAD_MARGIN = 3, TILE_BAD_ORIGINS = 4, TILE_UNCOVERED = 5 };

inline const char* tile_layout_message(int e) {
    switch (e) {
        case TILE_BAD_SIZE: return "the image length and the tile must be at least 1";
        case TILE_BAD_OVERLAP: return "the overlap must satisfy 0 < overlap < tile";
        case TILE_BAD_MARGIN: return "the margin must satisfy 0 <= margin and 2 * margin < overlap";
        case TILE_BAD_ORIGINS: return "the origins must be non-decreasing, start at 0, end at n - tile and overlap by more than 2 * margin";
        case TILE_UNCOVERED: return "a pixel is covered by no tile or its weights sum to 0";
        default: return "";
    }
}

// length of the tiles on an axis of n pixels
inline int tile_length(int n, int tile) { return n < tile ? n : tile; }

// number of tiles of the axis, or a negative TileLayoutError
inline int tile_count(int n, int tile, int overlap) {
    if (n < 1 || tile < 1) return -TILE_BAD_SIZE;
    if (overlap < 1 || overlap >= tile) return -TILE_BAD_OVERLAP;
    if (n <= tile) return 1;
    const int64_t s = tile - overlap, span = (int64_t)n - tile;
    return (int)((span + s - 1) / s) + 1;
}

// the origins of the axis' tiles -> origins[count] (count = tile_count(...) > 0)
inline void tile_origins(int n, int tile, int count, int* origins) {
    origins[0] = 0;
    for (int i = 1; i < count; ++i) origins[i] = (int)(((int64_t)i * ((int64_t)n - tile)) / (count - 1));
}

// what any list of origins must satisfy for the weights and the coverage tables: tiles of length t = tile_length(n, tile)
inline int tile_check_origins(int n, int tile, int margin, int count, const int* origins) {
    if (n < 1 || tile < 1) return TILE_BAD_SIZE;
    if (margin < 0) return TILE_BAD_MARGIN;
    const int t = tile_length(n, tile);
    if (count < 1 || !origins || origins[0] != 0 || origins[count - 1] != n - t) return TILE_BAD_ORIGINS;
    for (int i = 1; i < count; ++i) {
        if (origins[i] < origins[i - 1]) return TILE_BAD_ORIGINS;
        if ((int64_t)origins[i - 1] + t - origins[i] - 2 * (int64_t)margin <= 0) return TILE_BAD_ORIGINS;
    }
    return TILE_OK;
}

// raw weight of tile i at local index j
inline double tile_raw_weight(int t, int margin, int count, const int* origins, int i, int j) {
    double w = 1.0;
    if (i > 0) {
        const double R = (double)(origins[i - 1] + t - origins[i] - 2 * margin);
        double l = ((double)(j - margin) + 0.5) / R;
        l = l < 0.0 ? 0.0 : (l > 1.0 ? 1.0 : l);
        if (l < w) w = l;
    }
    if (i < count - 1) {
        const double R = (double)(origins[i] + t - origins[i + 1] - 2 * margin);
        double r = ((double)(t - margin - j) - 0.5) / R;
        r = r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);
        if (r < w) w = r;
    }
    return w;
}

// first covering tile and number of covering tiles of every pixel -> first[n], cover[n] (the covering tiles of a pixel are
// consecutive: the origins do not decrease).  TILE_UNCOVERED if a pixel has none.
inline int tile_coverage(int n, int tile, int count, const int* origins, int32_t* first, int32_t* cover) {
    const int t = tile_length(n, tile);
    int lo = 0, hi = 0;   // tiles [lo, hi) cover g
    for (int g = 0; g < n; ++g) {
        while (hi < count && origins[hi] <= g) ++hi;
        while (lo < hi && origins[lo] + t <= g) ++lo;
        if (lo == hi) return TILE_UNCOVERED;
        first[g] = lo;
        cover[g] = hi - lo;
    }
    return TILE_OK;
}

// normalised weights [count][t] and the coverage tables (either table pointer pair may be null)
inline int tile_weights(int n, int tile, int margin, int count, const int* origins, double* weights, int32_t* first, int32_t* cover) {
    if (int e = tile_check_origins(n, tile, margin, count, origins)) return e;
    const int t = tile_length(n, tile);
    std::vector<int32_t> f((size_t)n), c((size_t)n);
    if (int e = tile_coverage(n, tile, count, origins, f.data(), c.data())) return e;
    std::vector<double> W((size_t)n);
    for (int g = 0; g < n; ++g) {
        double s = 0.0;
        for (int i = f[g]; i < f[g] + c[g]; ++i) s = s + tile_raw_weight(t, margin, count, origins, i, g - origins[i]);
        if (!(s > 0.0)) return TILE_UNCOVERED;
        W[g] = s;
    }
    if (weights)
        for (int i = 0; i < count; ++i)
            for (int j = 0; j < t; ++j) weights[(size_t)i * t + j] = tile_raw_weight(t, margin, count, origins, i, j) / W[origins[i] + j];
    if (first && cover)
        for (int g = 0; g < n; ++g) {
            first[g] = f[g];
            cover[g] = c[g];
        }
    return TILE_OK;
}

}  // namespace rl
