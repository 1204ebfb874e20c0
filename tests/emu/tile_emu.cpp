// Host emulator of the tile kernels (rescan_line_sted_amd/csrc/tile_kernels.hpp, tile_kernels.hip): the very same thread bodies,
// run thread by thread over the launch grid (whole workgroups: the threads past the last vector take the kernels' early exit),
// with the launchers' own parameters; and the layout code (tile_layout.hpp) behind a C interface.  TEST INFRASTRUCTURE ONLY --
// built by tests/test_tile_cpu.py with g++ (-ffp-contract=off), as a shared library and, with -DTILE_EMU_MAIN, as a stand-alone
// program for the sanitizers; never loaded by the product.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/tile_kernels.hpp"
#include "../../rescan_line_sted_amd/csrc/tile_layout.hpp"

using namespace rl;

namespace {

template <typename TS, typename TD>
void gather(const void* src, void* dst, const int32_t* slot, int slots, int V, int NY, int NX, int ty, int tx) {
    const TileGatherParams<TS, TD> p = tile_gather_params<TS, TD>(src, dst, slot, slots, V, NY, NX, ty, tx);
    const size_t vectors = tile_gather_vectors(slots, V, ty, p.cpr), blocks = (vectors + kTileThreads - 1) / kTileThreads;
    for (size_t b = 0; b < blocks; ++b)
        for (int t = 0; t < kTileThreads; ++t) {
            const size_t id = b * kTileThreads + t;
            if (id < vectors) tile_gather_thread<TS, TD>(p, id);
        }
}

template <typename TT, typename TO>
int blend(const void* tiles, void* out, int F, int NY, int NX, int nyt, int nxt, int ty, int tx, const int32_t* oy, const int32_t* ox,
          const double* wy, const double* wx) {
    std::vector<int32_t> fy(NY), cy(NY), fx(NX), cx(NX);
    if (tile_coverage(NY, ty, nyt, oy, fy.data(), cy.data()) || tile_coverage(NX, tx, nxt, ox, fx.data(), cx.data())) return -1;
    const TileBlendParams<TT, TO> p =
        tile_blend_params<TT, TO>(tiles, out, oy, ox, wy, wx, fy.data(), cy.data(), fx.data(), cx.data(), F, NY, NX, nyt, nxt, ty, tx);
    const size_t vectors = tile_blend_vectors(F, NY, p.cpr), blocks = (vectors + kTileThreads - 1) / kTileThreads;
    for (size_t b = 0; b < blocks; ++b)
        for (int t = 0; t < kTileThreads; ++t) {
            const size_t id = b * kTileThreads + t;
            if (id < vectors) tile_blend_thread<TT, TO>(p, id);
        }
    return p.vec ? 1 : 0;
}

}  // namespace

extern "C" {
int emu_tile_threads() { return kTileThreads; }
// the layout: the return values of tile_layout.hpp (count > 0 or -error; 0 or error)
int emu_tile_count(int n, int tile, int overlap) { return tile_count(n, tile, overlap); }
void emu_tile_origins(int n, int tile, int count, int* origins) { tile_origins(n, tile, count, origins); }
int emu_tile_weights(int n, int tile, int margin, int count, const int* origins, double* weights, int32_t* first, int32_t* cover) {
    return tile_weights(n, tile, margin, count, origins, weights, first, cover);
}
// dtypes: 0 f32, 1 f64.  dst: exactly slots * V * ty * tx values.
void emu_tile_gather(const void* src, int src_dtype, int V, int NY, int NX, const int32_t* slot, int slots, int ty, int tx, void* dst,
                     int dst_dtype) {
    if (src_dtype == 0)
        dst_dtype == 0 ? gather<float, float>(src, dst, slot, slots, V, NY, NX, ty, tx) : gather<float, double>(src, dst, slot, slots, V, NY, NX, ty, tx);
    else
        dst_dtype == 0 ? gather<double, float>(src, dst, slot, slots, V, NY, NX, ty, tx) : gather<double, double>(src, dst, slot, slots, V, NY, NX, ty, tx);
}
// returns 1 if the launch takes the 16-byte store path, 0 for the element path, -1 on origins that leave a pixel uncovered
int emu_tile_blend(const void* tiles, int tiles_dtype, int F, int NY, int NX, int nyt, int nxt, int ty, int tx, const int32_t* oy,
                   const int32_t* ox, const double* wy, const double* wx, void* out, int out_dtype) {
    if (tiles_dtype == 0)
        return out_dtype == 0 ? blend<float, float>(tiles, out, F, NY, NX, nyt, nxt, ty, tx, oy, ox, wy, wx)
                              : blend<float, double>(tiles, out, F, NY, NX, nyt, nxt, ty, tx, oy, ox, wy, wx);
    return out_dtype == 0 ? blend<double, float>(tiles, out, F, NY, NX, nyt, nxt, ty, tx, oy, ox, wy, wx)
                          : blend<double, double>(tiles, out, F, NY, NX, nyt, nxt, ty, tx, oy, ox, wy, wx);
}
}

#ifdef TILE_EMU_MAIN
// The stand-alone program of the sanitizer run: exactly-sized buffers at aligned and odd element offsets (a read or a write past
// one is the sanitizer's to find), all dtype pairs, fillers, one-, two- and three-tile coverage; the results are held to plain
// loops written here.  Prints "ok <gathers> <blends>" and returns 0, or says what failed.
namespace {
unsigned g_state = 12345u;
double next() {
    g_state = g_state * 1664525u + 1013904223u;
    return 0.25 + (double)(g_state >> 20) / 4096.0;
}

struct Axis {
    int n, t, count;
    std::vector<int> o;
    std::vector<double> w;
};
bool make_axis(int n, int tile, int overlap, int margin, Axis* a) {
    a->n = n;
    a->t = tile_length(n, tile);
    a->count = tile_count(n, tile, overlap);
    if (a->count < 1) return false;
    a->o.resize(a->count);
    tile_origins(n, tile, a->count, a->o.data());
    a->w.resize((size_t)a->count * a->t);
    return tile_weights(n, tile, margin, a->count, a->o.data(), a->w.data(), nullptr, nullptr) == TILE_OK;
}

template <typename TS, typename TD>
int gather_case(int shift, long* done) {
    const int F = 2, V = 2, NY = 37, NX = 53;
    for (int tx : {24, 21})
        for (int ty : {16}) {
            std::vector<TS> src(shift + (size_t)F * V * NY * NX);
            for (auto& x : src) x = (TS)next();
            const int32_t slot[] = {0, 0, 0, 1, NY - ty, NX - tx, -1, 0, 0, 1, 5, 7, 0, 21, 29 - (tx == 24 ? 0 : 1), -1, 3, 3};
            const int slots = 6;
            std::vector<TD> dst(shift + (size_t)slots * V * ty * tx, TD(-7));
            emu_tile_gather(src.data() + shift, sizeof(TS) == 4 ? 0 : 1, V, NY, NX, slot, slots, ty, tx, dst.data() + shift, sizeof(TD) == 4 ? 0 : 1);
            for (int k = 0; k < slots; ++k)
                for (int v = 0; v < V; ++v)
                    for (int y = 0; y < ty; ++y)
                        for (int x = 0; x < tx; ++x) {
                            const TD got = dst[shift + (((size_t)k * V + v) * ty + y) * tx + x];
                            const TD want = slot[3 * k] < 0 ? TD(1)
                                                            : (TD)src[shift + (((size_t)slot[3 * k] * V + v) * NY + slot[3 * k + 1] + y) * NX + slot[3 * k + 2] + x];
                            if (got != want) {
                                std::printf("gather tx %d shift %d slot %d view %d (%d, %d): %.17g, want %.17g\n", tx, shift, k, v, y, x, (double)got, (double)want);
                                return 1;
                            }
                        }
            for (int i = 0; i < shift; ++i)
                if (dst[i] != TD(-7)) return 1;
            ++*done;
        }
    return 0;
}

template <typename TT, typename TO>
int blend_case(int NY, int NX, int tile, int overlap, int margin, int shift, long* done) {
    const int F = 2;
    Axis ay, ax;
    if (!make_axis(NY, tile, overlap, margin, &ay) || !make_axis(NX, tile, overlap, margin, &ax)) {
        std::printf("layout %d x %d tile %d overlap %d margin %d failed\n", NY, NX, tile, overlap, margin);
        return 1;
    }
    const size_t te = (size_t)ay.t * ax.t;
    std::vector<TT> tiles(shift + (size_t)F * ay.count * ax.count * te);
    for (auto& x : tiles) x = (TT)next();
    std::vector<TO> out(shift + (size_t)F * NY * NX, TO(-7));
    if (emu_tile_blend(tiles.data() + shift, sizeof(TT) == 4 ? 0 : 1, F, NY, NX, ay.count, ax.count, ay.t, ax.t, ay.o.data(), ax.o.data(),
                       ay.w.data(), ax.w.data(), out.data() + shift, sizeof(TO) == 4 ? 0 : 1) < 0)
        return 1;
    for (int f = 0; f < F; ++f)
        for (int gy = 0; gy < NY; ++gy)
            for (int gx = 0; gx < NX; ++gx) {
                double acc = 0.0, wsum = 0.0;
                for (int iy = 0; iy < ay.count; ++iy)
                    for (int ix = 0; ix < ax.count; ++ix) {
                        const int ly = gy - ay.o[iy], lx = gx - ax.o[ix];
                        if (ly < 0 || ly >= ay.t || lx < 0 || lx >= ax.t) continue;
                        const double w = ay.w[(size_t)iy * ay.t + ly] * ax.w[(size_t)ix * ax.t + lx];
                        wsum += w;
                        acc = acc + w * (double)tiles[shift + (((size_t)f * ay.count + iy) * ax.count + ix) * te + (size_t)ly * ax.t + lx];
                    }
                const TO got = out[shift + ((size_t)f * NY + gy) * NX + gx];
                if (got != (TO)acc || std::fabs(wsum - 1.0) > 1e-15) {
                    std::printf("blend %d x %d shift %d frame %d (%d, %d): %.17g, want %.17g, weights sum to %.17g\n", NY, NX, shift, f, gy, gx,
                                (double)got, acc, wsum);
                    return 1;
                }
            }
    ++*done;
    return 0;
}
}  // namespace

int main() {
    long gathers = 0, blends = 0;
    for (int shift = 0; shift < 2; ++shift) {
        if (gather_case<float, float>(shift, &gathers) || gather_case<float, double>(shift, &gathers) ||
            gather_case<double, float>(shift, &gathers) || gather_case<double, double>(shift, &gathers))
            return 1;
        const int shapes[][5] = {{150, 131, 64, 24, 8}, {64, 128, 64, 24, 0}, {105, 128, 64, 24, 8}, {70, 63, 64, 32, 8}, {5, 200, 64, 17, 0}};
        for (const auto& sh : shapes)
            if (blend_case<float, float>(sh[0], sh[1], sh[2], sh[3], sh[4], shift, &blends) ||
                blend_case<float, double>(sh[0], sh[1], sh[2], sh[3], sh[4], shift, &blends) ||
                blend_case<double, float>(sh[0], sh[1], sh[2], sh[3], sh[4], shift, &blends) ||
                blend_case<double, double>(sh[0], sh[1], sh[2], sh[3], sh[4], shift, &blends))
                return 1;
    }
    std::printf("ok %ld %ld\n", gathers, blends);
    return 0;
}
#endif
