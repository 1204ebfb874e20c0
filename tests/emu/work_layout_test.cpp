// Stand-alone check of the workspace layout (rescan_line_sted_amd/csrc/work_layout.hpp) for the sanitizers.  TEST INFRASTRUCTURE
// ONLY -- built and run by tests/test_work_layout_cpu.py (g++ -fsanitize=address,undefined).
//   no argument   case A: a fixed list of region sequences, the invariants of WorkLayout asserted on each; case B: every sequence
//                 once more into a heap block of exactly bytes(), every region filled through at() over copies x count elements.
//                 Prints "ok <sequences> <regions>" and returns 0, or says what failed.
//   "short"       a block ONE BYTE shorter than bytes(), the last region filled: the address sanitizer must end the run.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/work_layout.hpp"

using namespace rl;

struct Odd { int32_t v[3]; };   // 12 bytes: no divisor of 256
static_assert(sizeof(Odd) == 12 && 256 % sizeof(Odd) != 0, "the odd element size");

struct Decl { size_t esize, count, copies; };

struct Placed {
    size_t esize, count, copies, offset, region_bytes, begin, end;   // begin, end: bytes() before and after the add
    std::function<void*(void*)> at;
    std::function<void(void*)> fill;
};

template <typename T>
static Placed place(WorkLayout& lay, const Decl& d) {
    Placed p{sizeof(T), d.count, d.copies, 0, 0, lay.bytes(), 0, nullptr, nullptr};
    const Region<T> r = d.copies == 1 ? lay.add<T>(d.count) : lay.add<T>(d.count, d.copies);   // (the default argument too)
    p.offset = r.offset;
    p.region_bytes = r.bytes();
    p.end = lay.bytes();
    p.at = [r](void* base) { return (void*)r.at(base); };
    p.fill = [r, d](void* base) {
        if (T* q = r.at(base)) std::fill_n(q, d.copies * d.count, T());
    };
    return p;
}

static Placed place(WorkLayout& lay, const Decl& d) {
    switch (d.esize) {
        case 1: return place<unsigned char>(lay, d);
        case 4: return place<float>(lay, d);
        case 8: return place<double>(lay, d);
        default: return place<Odd>(lay, d);
    }
}

static const std::vector<std::vector<Decl>> kSequences = {
    {{1, 0, 1}},                                                                           // nothing at all
    {{1, 1, 1}, {4, 1, 1}, {8, 1, 1}, {12, 1, 1}},                                        // one element of every size
    {{8, 37, 1}, {4, 38, 1}, {8, 0, 1}, {8, 37, 1}, {8, 1000, 1}, {8, 222, 1}},           // an optional region left out
    {{8, 10, 1}, {12, 21, 3}, {4, 169, 3}, {1, 300, 3}, {8, 0, 3}, {4, 64, 1}},           // padded slots
    {{12, 64, 1}, {1, 256, 1}, {1, 257, 1}, {8, 32, 3}, {12, 0, 1}},                      // exact multiples of 256; empty at the end
    {{4, 3, 1}, {12, 5, 3}, {8, 64, 1}},                                                   // ends on the block's last byte ("short")
};

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::printf("sequence %zu region %zu: %s\n", s, i, #cond);                     \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "short")) {
        WorkLayout lay;
        std::vector<Placed> placed;
        for (const Decl& d : kSequences.back()) placed.push_back(place(lay, d));
        const Placed& last = placed.back();
        if (last.offset + last.copies * last.count * last.esize != lay.bytes()) {
            std::printf("the last region does not end on the last byte\n");
            return 0;   // (the caller expects a sanitizer report: ending well is the failure)
        }
        char* block = (char*)std::malloc(lay.bytes() - 1);
        last.fill(block);
        std::free(block);
        std::printf("a write past the block went unreported\n");
        return 0;
    }
    size_t regions = 0;
    for (size_t s = 0; s < kSequences.size(); ++s) {
        WorkLayout lay;
        std::vector<Placed> placed;
        for (const Decl& d : kSequences[s]) placed.push_back(place(lay, d));
        char* block = (char*)std::malloc(lay.bytes() ? lay.bytes() : 1);
        size_t top = 0;
        for (size_t i = 0; i < placed.size(); ++i, ++regions) {
            const Placed& p = placed[i];
            const size_t slot = (p.count * p.esize + 255) / 256 * 256;
            CHECK(p.offset % kWorkAlign == 0);
            CHECK(p.begin == top && p.offset == top);                        // in declaration order, no gap, no overlap
            CHECK(p.end == p.offset + p.copies * slot);
            CHECK(p.offset + p.copies * p.count * p.esize <= p.end);         // what the kernels index stays inside
            CHECK(p.region_bytes == p.count * p.esize);
            CHECK((p.at(block) == nullptr) == (p.count == 0));
            CHECK(p.count == 0 || p.at(block) == (void*)(block + p.offset));
            top = p.end;
        }
        if (lay.bytes() != top) {
            std::printf("sequence %zu: bytes() is %zu, the last reservation ends at %zu\n", s, lay.bytes(), top);
            return 1;
        }
        for (const Placed& p : placed) p.fill(block);                        // case B: the sanitizer watches every store
        std::free(block);
    }
    std::printf("ok %zu %zu\n", kSequences.size(), regions);
    return 0;
}
