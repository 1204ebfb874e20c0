// Stand-alone check of the tile layout (rescan_line_sted_amd/csrc/tile_layout.hpp) for the sanitizers: every (n, tile, overlap,
// margin) of a grid through tile_count / tile_origins / tile_weights into exactly-sized arrays, the invariants of the layout rule
// asserted on the way.  TEST INFRASTRUCTURE ONLY -- built and run by tests/test_tile_cpu.py (g++ -fsanitize=address,undefined).
// Prints "ok <layouts> <rejected>" and returns 0, or says what failed.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/tile_layout.hpp"

using namespace rl;

static int check(int n, int tile, int overlap, int margin, long* three) {
    const int count = tile_count(n, tile, overlap);
    if (count < 1) {
        std::printf("n %d tile %d overlap %d: count %d\n", n, tile, overlap, count);
        return 1;
    }
    const int t = tile_length(n, tile);
    std::vector<int> o(count);
    tile_origins(n, tile, count, o.data());
    if (o[0] != 0 || o[count - 1] != n - t) {
        std::printf("n %d tile %d overlap %d: origins run from %d to %d\n", n, tile, overlap, o[0], o[count - 1]);
        return 1;
    }
    for (int i = 1; i < count; ++i)
        if (o[i - 1] + t - o[i] < overlap || o[i] <= o[i - 1]) {
            std::printf("n %d tile %d overlap %d: tiles %d and %d overlap by %d\n", n, tile, overlap, i - 1, i, o[i - 1] + t - o[i]);
            return 1;
        }
    std::vector<double> w((size_t)count * t);
    std::vector<int32_t> first(n), cover(n);
    if (int e = tile_weights(n, tile, margin, count, o.data(), w.data(), first.data(), cover.data())) {
        std::printf("n %d tile %d overlap %d margin %d: %s\n", n, tile, overlap, margin, tile_layout_message(e));
        return 1;
    }
    for (int g = 0; g < n; ++g) {
        double s = 0.0;
        for (int i = first[g]; i < first[g] + cover[g]; ++i) {
            const double v = w[(size_t)i * t + (g - o[i])];
            if (!(v >= 0.0 && v <= 1.0)) return 1;
            s += v;
        }
        if (cover[g] >= 3) ++*three;
        for (int i = 0; i < count; ++i)   // the table names exactly the covering tiles
            if ((o[i] <= g && g < o[i] + t) != (i >= first[g] && i < first[g] + cover[g])) return 1;
        if (std::fabs(s - 1.0) > 4 * 2.220446049250313e-16) {
            std::printf("n %d tile %d overlap %d margin %d: the weights of pixel %d sum to %.17g\n", n, tile, overlap, margin, g, s);
            return 1;
        }
    }
    // the margin: weight 0 within `margin` pixels of an interior tile edge
    for (int i = 0; i < count; ++i)
        for (int j = 0; j < margin; ++j) {
            if (i > 0 && w[(size_t)i * t + j] != 0.0) return 1;
            if (i < count - 1 && w[(size_t)i * t + (t - 1 - j)] != 0.0) return 1;
        }
    return 0;
}

int main() {
    long layouts = 0, rejected = 0, three = 0;
    const int tile = 64;
    for (int overlap : {17, 24, 32})
        for (int margin : {0, 8}) {
            const int s = tile - overlap;
            for (int n : {1, 5, tile - 1, tile, tile + 1, 2 * tile - overlap, 2 * tile - overlap + 1, tile + s + 1, 150, 131, 1000, 4700}) {
                if (check(n, tile, overlap, margin, &three)) return 1;
                ++layouts;
            }
        }
    if (three == 0) {
        std::printf("no pixel under three tiles\n");
        return 1;
    }
    const int bad[][3] = {{64, 64, 0}, {64, 0, 0}, {64, 70, 0}, {0, 8, 0}, {64, -3, 0}};
    for (const auto& b : bad) {
        if (tile_count(150, b[0], b[1]) > 0) {
            std::printf("tile %d overlap %d accepted\n", b[0], b[1]);
            return 1;
        }
        ++rejected;
    }
    {   // a margin that eats the overlap; origins that do not reach the end
        int o3[3];
        tile_origins(150, 64, 3, o3);
        const int o_bad[3] = {0, 40, 80};
        std::vector<double> w(3 * 64);
        if (tile_weights(150, 64, 40, 3, o3, w.data(), nullptr, nullptr) == TILE_OK) return 1;
        if (tile_weights(150, 64, -1, 3, o3, w.data(), nullptr, nullptr) == TILE_OK) return 1;
        if (tile_weights(150, 64, 0, 3, o_bad, w.data(), nullptr, nullptr) == TILE_OK) return 1;
        rejected += 3;
    }
    std::printf("ok %ld %ld\n", layouts, rejected);
    return 0;
}
