// object_classes_test.cpp -- stand-alone driver of csrc/object_classes.hpp for tests/test_object_classes_cpu.py.
// stdin:   pixels B n max_reps cf has_brightness, then B * n pixel values [, B brightness values]
//      or  index  B max_reps cf has_brightness, then B object indices [, B brightness values]
// (a brightness is read as text: "nan", "-0" and the like are what strtod makes of them)
// stdout:  classes, then cls[B] / compact images, then c0 nrep per slice / rep_frames / rate_of[B]
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/object_classes.hpp"

static double read_double() {
    std::string w;
    if (!(std::cin >> w)) {
        std::fprintf(stderr, "short input\n");
        std::exit(2);
    }
    return std::strtod(w.c_str(), nullptr);
}

template <typename V>
static void print_line(int head, const V& v) {
    std::printf("%d", head);
    for (auto x : v) std::printf(" %ld", (long)x);
    std::printf("\n");
}

int main() {
    std::string mode;
    int B = 0, max_reps = 0, cf = 0, has_tb = 0;
    size_t n = 0;
    std::cin >> mode >> B;
    if (mode == "pixels") std::cin >> n;
    std::cin >> max_reps >> cf >> has_tb;
    if (!std::cin || B < 0 || (mode != "pixels" && mode != "index")) {
        std::fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<double> frames, tb;
    std::vector<uint32_t> idx;
    if (mode == "pixels") {
        frames.resize((size_t)B * n);
        for (double& x : frames) x = read_double();
    } else {
        idx.resize((size_t)B);
        for (uint32_t& x : idx) x = (uint32_t)read_double();
    }
    if (has_tb) {
        tb.resize((size_t)B);
        for (double& x : tb) x = read_double();
    }
    std::vector<int> cls;
    const int classes = mode == "pixels" ? rl::classify_by_pixels(frames.data(), n, B, has_tb ? tb.data() : nullptr, cls, max_reps)
                                         : rl::classify_by_index(idx.data(), has_tb ? tb.data() : nullptr, B, cls, max_reps);
    print_line(classes, cls);
    std::vector<rl::SliceShare> slices;
    std::vector<uint32_t> reps, rate;
    const int total = rl::share_layout(cls, cf, slices, reps, rate);
    std::vector<int> flat;
    for (const rl::SliceShare& s : slices) {
        flat.push_back(s.c0);
        flat.push_back(s.nrep);
    }
    print_line(total, flat);
    print_line((int)reps.size(), reps);
    print_line((int)rate.size(), rate);
    return 0;
}
