// class_layout_test.cpp -- stand-alone driver of csrc/object_classes.hpp class_layout for tests/test_class_layout_cpu.py.
// stdin:   B cf, then cls[B]
// stdout:  compact classes, then nrep per slice / rep_frames / rate_of[B]   (each line: count, then the values)
#include <cstdio>
#include <iostream>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/object_classes.hpp"

template <typename V>
static void print_line(int head, const V& v) {
    std::printf("%d", head);
    for (auto x : v) std::printf(" %ld", (long)x);
    std::printf("\n");
}

int main() {
    int B = 0, cf = 0;
    std::cin >> B >> cf;
    if (!std::cin || B < 0) {
        std::fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<int> cls((size_t)B);
    for (int& c : cls) std::cin >> c;
    if (!std::cin) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    std::vector<rl::SliceShare> slices;
    std::vector<uint32_t> reps, rate;
    rl::share_layout(cls, cf, slices, reps, rate);
    const int total = rl::class_layout(cls, cf, slices, reps, rate);
    std::vector<int> nrep;
    for (const rl::SliceShare& s : slices) {
        if (s.c0 != 0) return 3;   // (no longer a position in the compact buffers)
        nrep.push_back(s.nrep);
    }
    print_line(total, nrep);
    print_line((int)reps.size(), reps);
    print_line((int)rate.size(), rate);
    return 0;
}
