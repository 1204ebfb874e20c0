// tile_kernels.hpp -- tiled Richardson-Lucy on images of any size (rl_tile_gather, rl_tile_blend, include/rlsted.h; DESIGN.md
// section 4i): the thread bodies of tile_kernels.hip, written as host-compilable templates so that the CPU tests run the very
// same code (tests/emu/tile_emu.cpp), and the launchers.  A tile is a frame of an ordinary plan; these two kernels only move data.
//
// GATHER  src [F][V][NY][NX] (TS) -> dst [slots][V][ty][tx] (TD), a plan's measurement buffer.  Slot k is the window at
//   (a_y, a_x) of frame `frame` (slot[3 k .. 3 k + 2]); frame = -1: a filler, written with ones.  A plain copy, one rounding at
//   most.  A thread writes one vector of W = 16 / sizeof(TD) values of one destination row (the last vector of a row partial):
//   through one 16-byte store where tx is a multiple of W and dst is 16-byte aligned, element by element otherwise.  The window's
//   origin is arbitrary, so its W source values are fetched as one unaligned run (tile_load_run).  Nothing is written past the
//   slots * V * ty * tx values of dst.
// BLEND   tiles [F][nyt][nxt][ty][tx] (TT) -> out [F][NY][NX] (TO):
//     out[f][gy][gx] = sum_iy sum_ix (wy[iy][gy - oy[iy]] * wx[ix][gx - ox[ix]]) * (double)tiles[f][iy][ix][gy - oy[iy]][gx - ox[ix]]
//   over the tiles that cover the pixel, in float64, from 0.0, iy ascending in the outer loop and ix ascending in the inner one,
//   each term (wy * wx) * e, no contraction, no atomics: bit-identical from run to run and to the numpy twin
//   (tests/tile_reference.py).  A gather per output pixel driven by the coverage tables (first covering tile and count, per
//   global row and per global column: tile_layout.hpp); any number of tiles may cover a pixel.  A thread forms one vector of
//   W = 16 / sizeof(TO) pixels of one output row and walks the tiles that cover any of them: a tile that covers all W gives its W
//   values and W column weights as unaligned runs, one that covers some (its first and last columns) pixel by pixel -- a pixel's
//   sum runs over its own covering tiles in the same order either way.  One 16-byte store where NX is a
//   multiple of W and out is 16-byte aligned, element stores otherwise.  No LDS.
// Grids: one thread per vector, kTileThreads threads per workgroup -- sized by the pixels, not by the CUs.
#pragma once
#include "accel_kernels.hpp"

#include <cstddef>
#include <cstdint>

namespace rl {

constexpr int kTileThreads = 256;   // four waves

template <typename TS, typename TD>
struct TileGatherParams {
    const TS* src;          // [F][V][NY][NX]
    TD* dst;                // [slots][V][ty][tx]
    const int32_t* slot;    // [slots][3]: frame (-1: filler), a_y, a_x (device)
    int slots, V, NY, NX, ty, tx;
    int cpr;                // vectors per destination row: ceil(tx / W)
    bool vec;               // 16-byte stores
};

template <typename TT, typename TO>
struct TileBlendParams {
    const TT* tiles;        // [F][nyt][nxt][ty][tx]
    TO* out;                // [F][NY][NX]
    const int32_t* oy;      // [nyt] origins (device)
    const int32_t* ox;      // [nxt]
    const double* wy;       // [nyt][ty] normalised weights
    const double* wx;       // [nxt][tx]
    const int32_t* first_y; // [NY] first covering tile row, cover_y [NY] how many
    const int32_t* cover_y;
    const int32_t* first_x; // [NX]
    const int32_t* cover_x;
    int F, NY, NX, nyt, nxt, ty, tx;
    int cpr;                // vectors per output row: ceil(NX / W)
    bool vec;               // 16-byte stores
};

// threads of a launch: one per vector
RL_HD size_t tile_gather_vectors(int slots, int V, int ty, int cpr) { return (size_t)slots * V * ty * cpr; }
RL_HD size_t tile_blend_vectors(int F, int NY, int cpr) { return (size_t)F * NY * cpr; }

// the parameters of a launch (the launchers' and the emulation's): the tables are the device's (the emulation's: host) pointers
template <typename TS, typename TD>
inline TileGatherParams<TS, TD> tile_gather_params(const void* src, void* dst, const int32_t* slot, int slots, int V, int NY, int NX,
                                                   int ty, int tx) {
    constexpr int W = 16 / sizeof(TD);
    TileGatherParams<TS, TD> p;
    p.src = (const TS*)src;
    p.dst = (TD*)dst;
    p.slot = slot;
    p.slots = slots; p.V = V; p.NY = NY; p.NX = NX; p.ty = ty; p.tx = tx;
    p.cpr = (tx + W - 1) / W;
    p.vec = tx % W == 0 && accel_aligned(dst);
    return p;
}
template <typename TT, typename TO>
inline TileBlendParams<TT, TO> tile_blend_params(const void* tiles, void* out, const int32_t* oy, const int32_t* ox, const double* wy,
                                                 const double* wx, const int32_t* first_y, const int32_t* cover_y, const int32_t* first_x,
                                                 const int32_t* cover_x, int F, int NY, int NX, int nyt, int nxt, int ty, int tx) {
    constexpr int W = 16 / sizeof(TO);
    TileBlendParams<TT, TO> p;
    p.tiles = (const TT*)tiles;
    p.out = (TO*)out;
    p.oy = oy; p.ox = ox; p.wy = wy; p.wx = wx;
    p.first_y = first_y; p.cover_y = cover_y; p.first_x = first_x; p.cover_x = cover_x;
    p.F = F; p.NY = NY; p.NX = NX; p.nyt = nyt; p.nxt = nxt; p.ty = ty; p.tx = tx;
    p.cpr = (NX + W - 1) / W;
    p.vec = NX % W == 0 && accel_aligned(out);
    return p;
}

// a = q b + r (the 32-bit division where a fits: the 64-bit one is a long sequence on the device)
RL_HD void tile_divmod(size_t a, int b, size_t& q, int& r) {
    if (a >> 32) {
        q = a / (size_t)b;
        r = (int)(a % (size_t)b);
    } else {
        const uint32_t a32 = (uint32_t)a;
        q = a32 / (uint32_t)b;
        r = (int)(a32 % (uint32_t)b);
    }
}

// W consecutive values from an address of any element alignment (the compiler's widest unaligned load)
template <typename T, int W>
RL_HD void tile_load_run(const T* p, T* v) {
    __builtin_memcpy(v, p, W * sizeof(T));
}

// GATHER, vector `id` of the launch (id < tile_gather_vectors)
template <typename TS, typename TD>
RL_HD void tile_gather_thread(const TileGatherParams<TS, TD>& p, size_t id) {
    constexpr int W = 16 / sizeof(TD);
    size_t row, sv, ks;                                   // row = (slot * V + v) * ty + ly
    int c, ly, v;
    tile_divmod(id, p.cpr, row, c);
    tile_divmod(row, p.ty, sv, ly);
    tile_divmod(sv, p.V, ks, v);
    const int k = (int)ks;
    const int x0 = c * W;
    const int frame = p.slot[3 * k], ay = p.slot[3 * k + 1], ax = p.slot[3 * k + 2];
    TD out[W];
    if (frame < 0) {
        for (int e = 0; e < W; ++e) out[e] = TD(1);
    } else {
        const TS* s = p.src + (((size_t)frame * p.V + v) * p.NY + (size_t)(ay + ly)) * p.NX + (size_t)(ax + x0);
        TS in[W];
        if (x0 + W <= p.tx) {
            tile_load_run<TS, W>(s, in);
        } else {
            for (int e = 0; e < W; ++e) in[e] = x0 + e < p.tx ? s[e] : TS(0);
        }
        for (int e = 0; e < W; ++e) out[e] = (TD)in[e];
    }
    // (row * tx + x0 is a multiple of W on the vector path: the row's n is then its end)
    accel_store(p.dst + row * p.tx, (size_t)x0, (size_t)p.tx, p.vec, out);
}

// BLEND, vector `id` of the launch (id < tile_blend_vectors)
template <typename TT, typename TO>
RL_HD void tile_blend_thread(const TileBlendParams<TT, TO>& p, size_t id) {
#pragma clang fp contract(off)
    constexpr int W = 16 / sizeof(TO);
    size_t row, f;                                        // row = f * NY + gy
    int c, gy;
    tile_divmod(id, p.cpr, row, c);
    tile_divmod(row, p.NY, f, gy);
    const int x0 = c * W;
    const int x1 = x0 + W <= p.NX ? x0 + W : p.NX;        // pixels [x0, x1)
    const int fy = p.first_y[gy], ny = p.cover_y[gy];
    const size_t tile_elems = (size_t)p.ty * p.tx;
    double acc[W];
    for (int e = 0; e < W; ++e) acc[e] = 0.0;
    // tiles [fx, ex) are those that cover a pixel of the vector (both tables do not decrease): each covers all W pixels -- one run of
    // estimates, one of column weights -- or, at its first and last columns, some of them
    const int fx = p.first_x[x0], ex = p.first_x[x1 - 1] + p.cover_x[x1 - 1];
    for (int iy = fy; iy < fy + ny; ++iy) {
        const int ly = gy - p.oy[iy];
        const double wyv = p.wy[(size_t)iy * p.ty + ly];
        const TT* trow = p.tiles + ((f * p.nyt + iy) * p.nxt) * tile_elems + (size_t)ly * p.tx;   // tile (f, iy, 0), row ly
        for (int ix = fx; ix < ex; ++ix) {
            const int lx = x0 - p.ox[ix];                                                          // (may lie outside the tile)
            const TT* ts = trow + (size_t)ix * tile_elems;
            const double* ws = p.wx + (size_t)ix * p.tx;
            if (lx >= 0 && lx + W <= p.tx) {
                TT e[W];
                double wxv[W];
                tile_load_run<TT, W>(ts + lx, e);
                tile_load_run<double, W>(ws + lx, wxv);
                for (int q = 0; q < W; ++q) {
                    const double w = wyv * wxv[q];
                    acc[q] = acc[q] + w * (double)e[q];
                }
            } else {
                for (int q = 0; q < W; ++q) {
                    const int l = lx + q;
                    if (l >= 0 && l < p.tx && x0 + q < x1) {
                        const double w = wyv * ws[l];
                        acc[q] = acc[q] + w * (double)ts[l];
                    }
                }
            }
        }
    }
    TO o[W];
    for (int e = 0; e < W; ++e) o[e] = (TO)acc[e];
    accel_store(p.out + row * p.NX, (size_t)x0, (size_t)p.NX, p.vec, o);
}

// ---- launchers (tile_kernels.hip), on stream s; dtypes RL_F32 / RL_F64.  The tables are device pointers.
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
hipError_t tile_gather(int src_dtype, int dst_dtype, const void* src, void* dst, const int32_t* slot, int slots, int V, int NY, int NX,
                       int ty, int tx, hipStream_t s);
hipError_t tile_blend(int tiles_dtype, int out_dtype, const void* tiles, void* out, const int32_t* oy, const int32_t* ox,
                      const double* wy, const double* wx, const int32_t* first_y, const int32_t* cover_y, const int32_t* first_x,
                      const int32_t* cover_x, int F, int NY, int NX, int nyt, int nxt, int ty, int tx, hipStream_t s);
#endif

}  // namespace rl
