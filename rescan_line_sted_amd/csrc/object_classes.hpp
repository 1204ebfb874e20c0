// object_classes.hpp -- which frames of a batch carry the same object, and which frame of a slice simulates for which.
// Host only, no HIP: the CPU tests compile it as it is (tests/emu/object_classes_test.cpp).
//
// A batch often holds one object many times over -- a sweep's seeds, the benchmark's frames -- and H(object) of two such
// frames is the same image bit for bit.  Frames are in one CLASS when their scaled objects are bit-identical by construction:
// the same float64 input pixels and the same brightness target (the device scales a frame by target / sum, the sum taken in an
// order that depends on the frame's pixels alone: aux_kernels.hip k_frame_sums).  A slice of the batch in which few classes
// cover many frames SHARES (share_layout); a cycle simulates each class its sharing slices hold once (class_layout), and the
// Poisson sampler draws every frame of such a slice from its class's rates (rlsted.cpp run_slices).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rl {

// Representatives a frame is compared against at most.  A frame that matches none of them while the list is full is a class of
// its own, which no later frame joins: a batch of all-distinct frames costs 8 first-difference comparisons per frame.
constexpr int kMaxClassReps = 8;

// cls[f] = class of frame f, numbered in order of first appearance; returns the number of classes.
// same(f, g): frame f is bit-identical to representative frame g (g < f).
template <class Same>
inline int classify_frames(int B, Same same, std::vector<int>& cls, int max_reps = kMaxClassReps) {
    cls.assign((size_t)(B > 0 ? B : 0), 0);
    std::vector<int> reps;   // frames others are compared against; frame reps[r] is of class cls[reps[r]]
    int classes = 0;
    for (int f = 0; f < B; ++f) {
        int c = -1;
        for (size_t r = 0; r < reps.size() && c < 0; ++r)
            if (same(f, reps[r])) c = cls[(size_t)reps[r]];
        if (c < 0) {
            c = classes++;
            if ((int)reps.size() < max_reps) reps.push_back(f);
        }
        cls[(size_t)f] = c;
    }
    return classes;
}

inline bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// rl_deconv_set_object: float64 frames [B][n] and (optionally) a brightness target per frame.  memcmp leaves at the first
// difference, so distinct frames cost next to nothing.
inline int classify_by_pixels(const double* frames, size_t n, int B, const double* brightness, std::vector<int>& cls,
                              int max_reps = kMaxClassReps) {
    return classify_frames(B, [&](int f, int g) {
        if (brightness && !same_bits(brightness[f], brightness[g])) return false;
        return std::memcmp(frames + (size_t)f * n, frames + (size_t)g * n, n * sizeof(double)) == 0;
    }, cls, max_reps);
}

// rl_batch_submit: frame f is staged object idx[f]; brightness == nullptr: the chunk is not scaled.
inline int classify_by_index(const uint32_t* idx, const double* brightness, int B, std::vector<int>& cls, int max_reps = kMaxClassReps) {
    return classify_frames(B, [&](int f, int g) {
        return idx[f] == idx[g] && (!brightness || same_bits(brightness[f], brightness[g]));
    }, cls, max_reps);
}

// What a slice of the batch simulates.  nrep > 0: the slice's representatives are compact images c0 .. c0 + nrep of the
// plan's compact buffers.  nrep == 0: every frame of the slice is simulated as it always was.
struct SliceShare {
    int c0 = 0, nrep = 0;
};

// Slices of cf frames.  Per slice the first frame of each class WITHIN the slice is its representative (no dependencies
// between slices, which run on different streams); a slice shares when at most half its frames are representatives.
//   rep_frames[c] = the frame whose object is compact image c                     (returned count entries)
//   rate_of[f]    = the compact image that holds frame f's rates                  (frames of sharing slices; 0 elsewhere)
// Returns the number of compact images.
inline int share_layout(const std::vector<int>& cls, int cf, std::vector<SliceShare>& slices, std::vector<uint32_t>& rep_frames,
                        std::vector<uint32_t>& rate_of) {
    const int B = (int)cls.size();
    slices.clear();
    rep_frames.clear();
    rate_of.assign((size_t)B, 0u);
    if (cf < 1) cf = 1;
    std::vector<int> seen_cls, seen_at;
    for (int f0 = 0; f0 < B; f0 += cf) {
        const int nf = f0 + cf <= B ? cf : B - f0;
        seen_cls.clear();
        seen_at.clear();
        std::vector<int> local((size_t)nf);
        for (int i = 0; i < nf && 2 * (int)seen_cls.size() <= nf; ++i) {   // (more than half: not shared, nothing more to learn)
            size_t r = 0;
            while (r < seen_cls.size() && seen_cls[r] != cls[(size_t)(f0 + i)]) ++r;
            if (r == seen_cls.size()) {
                seen_cls.push_back(cls[(size_t)(f0 + i)]);
                seen_at.push_back(f0 + i);
            }
            local[(size_t)i] = (int)r;
        }
        SliceShare s;
        const int nrep = (int)seen_cls.size();
        if (2 * nrep <= nf) {
            s.c0 = (int)rep_frames.size();
            s.nrep = nrep;
            for (int at : seen_at) rep_frames.push_back((uint32_t)at);
            for (int i = 0; i < nf; ++i) rate_of[(size_t)(f0 + i)] = (uint32_t)(s.c0 + local[(size_t)i]);
        }
        slices.push_back(s);
    }
    return (int)rep_frames.size();
}

// One simulation per class and CYCLE: H(object) of a class is the same image in every slice, so the sharing slices of a
// share_layout draw from ONE compact image per class instead of one per (slice, class).  Rewrites the layout in place:
//   rep_frames[c] = the first frame of a sharing slice that carries compact class c   (returned count entries)
//   rate_of[f]    = the compact class of frame f                                      (frames of sharing slices; 0 elsewhere)
// Which slices share, and each slice's nrep, stay as share_layout decided; c0 no longer means anything and is zeroed.
// Returns the number of compact classes: those that a sharing slice holds, numbered in order of first appearance.
inline int class_layout(const std::vector<int>& cls, int cf, std::vector<SliceShare>& slices, std::vector<uint32_t>& rep_frames,
                        std::vector<uint32_t>& rate_of) {
    const int B = (int)cls.size();
    rep_frames.clear();
    rate_of.assign((size_t)B, 0u);
    if (cf < 1) cf = 1;
    int n_cls = 0;
    for (int c : cls) n_cls = c + 1 > n_cls ? c + 1 : n_cls;
    std::vector<int> compact((size_t)n_cls, -1);
    for (size_t sl = 0; sl < slices.size(); ++sl) {
        slices[sl].c0 = 0;
        if (slices[sl].nrep == 0) continue;
        const int f0 = (int)sl * cf;
        for (int f = f0; f < f0 + cf && f < B; ++f) {
            int& c = compact[(size_t)cls[(size_t)f]];
            if (c < 0) {
                c = (int)rep_frames.size();
                rep_frames.push_back((uint32_t)f);
            }
            rate_of[(size_t)f] = (uint32_t)c;
        }
    }
    return (int)rep_frames.size();
}

}  // namespace rl
