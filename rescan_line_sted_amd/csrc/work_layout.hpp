// work_layout.hpp -- the regions of one call's workspace, each declared once: the total and every pointer come from the same
// declarations (plain C++17, no HIP: tests/emu/work_layout_test.cpp compiles it on the host)
#pragma once
#include <cstddef>

namespace rl {
constexpr size_t kWorkAlign = 256;
inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

template <typename T>
struct Region {   // `count` elements of T from byte `offset` of the block
    size_t offset = 0, count = 0;
    T* at(void* base) const { return count ? (T*)((char*)base + offset) : nullptr; }
    size_t bytes() const { return count * sizeof(T); }
};

class WorkLayout {
    size_t top_ = 0;
public:
    // `copies` slots of round_up(count * sizeof(T), kWorkAlign) bytes each, the first on a kWorkAlign boundary (a kernel that
    // indexes [slot][...] with the unpadded stride stays inside: the padded slots are at least as long)
    template <typename T>
    Region<T> add(size_t count, size_t copies = 1) {
        const Region<T> r{top_, count};
        top_ += copies * round_up(count * sizeof(T), kWorkAlign);
        return r;
    }
    size_t bytes() const { return top_; }
};
}  // namespace rl
