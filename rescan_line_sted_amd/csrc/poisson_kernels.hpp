// poisson_kernels.hpp -- the Poisson draw of frames that share their rate image, as a workgroup body (aux_kernels.hip
// k_poisson_groups; tests/emu/poisson_groups_emu.cpp runs the same text on the host), and the Philox keys of a launch.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "philox_poisson.hpp"

namespace rl {

// Philox key / counter of an image of the launch: one seed and consecutive image indices from
// image0, or -- frame_seeds != nullptr -- a seed and an image id per frame (V views each), so that
// a frame's draws do not depend on which batch it was put in.
struct PoissonKeys {
    unsigned long long seed0;
    unsigned image0, V;
    const unsigned long long* frame_seeds;   // [frames] or nullptr
    const unsigned* frame_ids;               // [frames] (with frame_seeds)
    // [frames] or nullptr: frame f of the launch takes its rates from images rate_frame[f] * V + view of `noiseless` (frames that
    // carry the same object share one simulated image, object_classes.hpp); the counters above stay the frame's own
    const unsigned* rate_frame;
    // of view `view` of frame f of the launch, and of image img = f * V + view of the launch
    RL_HD unsigned long long frame_seed(unsigned f) const { return frame_seeds ? frame_seeds[f] : seed0; }
    RL_HD unsigned frame_image(unsigned f, unsigned view) const { return (frame_seeds ? frame_ids[f] * V : image0 + f * V) + view; }
    RL_HD unsigned long long seed(unsigned img) const { return frame_seeds ? frame_seeds[img / V] : seed0; }
    RL_HD unsigned image(unsigned img) const { return frame_seeds ? frame_ids[img / V] * V + img % V : image0 + img; }
    template <typename T>
    RL_HD T rate(const T* __restrict__ noiseless, unsigned i, unsigned n_pix) const {
        if (!rate_frame) return noiseless[i];   // (uniform)
        const unsigned img = i / n_pix, pix = i - img * n_pix;
        return noiseless[((size_t)rate_frame[img / V] * V + img % V) * n_pix + pix];
    }
    // the rates of image `img` of the launch, for a tile that lies inside it (img is workgroup uniform: scalar loads)
    template <typename T>
    RL_HD const T* image_rates(const T* __restrict__ noiseless, unsigned img, unsigned n_pix) const {
        return noiseless + (rate_frame ? (size_t)rate_frame[img / V] * V + img % V : (size_t)img) * n_pix;
    }
};

// ---- frame groups: the draw of a launch whose frames share rate images (keys.rate_frame != nullptr, Philox) --------------------
// k_poisson evaluates the PTRS set-up -- a float64 square root and division per attempt, another division and two logarithms on
// the way to the logarithm test -- for every pixel of every frame, although it depends on the rate alone and the frames of an
// object class read one rate image.  Here a work item is kPoissonGroupPix pixels of one view (one per thread) times a group of
// kPoissonGroup frames of the launch: 2048 draws, the tile of k_poisson, with its lists, rounds and barriers.
// The groups are cut from the launch's frames in the order of their rate images (a stable sort by rate_frame[f], worked out by
// every workgroup for itself in LDS), not in the order of the launch: a sweep's chunk holds its objects interleaved -- rate_frame =
// 0 1 2 0 1 2 ... --, and groups of consecutive frames would be eight runs of one frame each there, every run with the whole set-up,
// its barriers and lists of a few entries (measured: twice k_poisson's time on such launches; profiles/poisson_groups).  In sorted
// order a launch of C rate images has at most C - 1 groups with more than one run.  A launch of more than kPoissonGroupPix frames
// keeps the launch's order.
// Inside a group the frames are taken in maximal runs of equal rate_frame[f] (workgroup uniform; a batch of one object: one run).
// Per run a thread loads its rate once, keeps ptrs_rate() in registers and writes it, with the rate-only values of the logarithm
// test, to a table in LDS; then it forms every frame's first candidate and squeeze test with the frame's own Philox key and
// image id, writes the accepted ones and lists the others as (frame in group, pixel in tile).  The rounds are k_poisson's: one
// attempt per round over the packed list -- attempt 0 repeats the first candidate and goes on into the acceptance test --, the
// survivors repacked into the other list; 0 < lam < 10 is listed from the back of list 0 and drawn by the multiplication method
// at the end.  The set-up of a listed draw comes from the table.  Every value is philox_poisson(lam, seed, image, pixel): the
// pieces of philox_poisson.hpp are deterministic functions of the rate, evaluated once instead of per frame.
constexpr int kPoissonGroup = 8, kPoissonGroupPix = 256, kPoissonGroupDraws = kPoissonGroup * kPoissonGroupPix;
constexpr int kPoissonGroupTab = 6;   // lam, b, a, vr, log(lam), log(invalpha)
// two lists of entries, the table, the lists' counters (front of either list, back of list 0; one spare for alignment)
// and the Philox key and image id of the group's frames (seed low, seed high, image); the launch's frames in sorted order, a byte each
constexpr size_t kPoissonGroupLds = 2 * kPoissonGroupDraws * sizeof(unsigned) + kPoissonGroupTab * kPoissonGroupPix * sizeof(double) + (4 + 3 * kPoissonGroup) * sizeof(unsigned) + kPoissonGroupPix;

template <typename T>
struct PoissonGroupParams {
    const T* noiseless;   // the rate images rate_frame points into
    T* noisy;             // [frames][V][n_pix]
    unsigned n_pix, frames;
    PoissonKeys keys;     // rate_frame != nullptr
};
RL_HD unsigned poisson_group_items(unsigned n_pix, unsigned frames, unsigned V) {
    return (frames + kPoissonGroup - 1u) / kPoissonGroup * V * ((n_pix + kPoissonGroupPix - 1u) / kPoissonGroupPix);
}

// Sync: wg() the workgroup barrier, lds_add(p, v) an atomic add on a counter in LDS that returns the value before.
// lds_raw: kPoissonGroupLds bytes, 8-byte aligned.  grid workgroups of kPoissonGroupPix threads walk the items in rounds of one
// per workgroup; a workgroup's place in the round moves on by 0.618 of the grid from round to round (k_poisson, aux_kernels.hip).
template <typename T, class Sync>
RL_HD void poisson_groups_body(const PoissonGroupParams<T>& p, unsigned tid, unsigned bx, unsigned grid, unsigned char* lds_raw, const Sync& sync) {
    unsigned* const lst0 = reinterpret_cast<unsigned*>(lds_raw);
    unsigned* const lst1 = lst0 + kPoissonGroupDraws;
    double* const tab = reinterpret_cast<double*>(lst1 + kPoissonGroupDraws);
    unsigned* const cnt = reinterpret_cast<unsigned*>(tab + kPoissonGroupTab * kPoissonGroupPix);   // [0], [1]: the lists; [2]: small rates
    unsigned* const key = cnt + 4;   // [frame in group][3].  A listed draw finds its frame's key here: per-frame keys (frame_seeds) would be a gather from global memory per entry and round
    unsigned char* const ord = reinterpret_cast<unsigned char*>(key + 3 * kPoissonGroup);   // [place in sorted order]: the frame
    const PoissonKeys& keys = p.keys;
    const unsigned V = keys.V, n_pix = p.n_pix;
    // the frames sorted by rate image, frames of one rate image in the launch's order: a frame's place is the number of frames before
    // it.  Their rate images stand in list 0 meanwhile: one load from global memory per frame, the counting reads LDS
    const bool sorted = p.frames <= (unsigned)kPoissonGroupPix;
    if (sorted) {
        if (tid < p.frames) lst0[tid] = keys.rate_frame[tid];
        sync.wg();
        if (tid < p.frames) {
            const unsigned c = lst0[tid];
            unsigned place = 0;
            for (unsigned f = 0; f < p.frames; ++f) {
                const unsigned cf = lst0[f];   // (uniform address)
                place += (cf < c || (cf == c && f < tid)) ? 1u : 0u;
            }
            ord[place] = (unsigned char)tid;
        }
        sync.wg();                            // (list 0 is free for the first item)
    }
    auto frame_at = [ord, sorted](unsigned j) { return sorted ? (unsigned)ord[j] : j; };   // the frame at place j
    const unsigned tiles = (n_pix + kPoissonGroupPix - 1u) / kPoissonGroupPix;
    const unsigned n_items = poisson_group_items(n_pix, p.frames, V);
    const unsigned turn = (unsigned)((float)grid * 0.6180339887f) | 1u;
    auto table_rate = [tab](unsigned px) {
        PtrsRate r;
        r.lam = tab[px];
        r.b = tab[kPoissonGroupPix + px];
        r.a = tab[2 * kPoissonGroupPix + px];
        r.vr = tab[3 * kPoissonGroupPix + px];
        return r;
    };
    for (unsigned first = 0, round = 0; first < n_items; first += grid, ++round) {
        const unsigned item = first + (bx + round * turn) % grid;
        if (item >= n_items) continue;        // (uniform; the last round may be short)
        const unsigned tile = item % tiles, view = item / tiles % V, g0 = item / (tiles * V) * kPoissonGroup;
        const unsigned g1 = g0 + kPoissonGroup < p.frames ? g0 + kPoissonGroup : p.frames;
        const unsigned pix = tile * kPoissonGroupPix + tid;
        const bool inside = pix < n_pix;      // (the last tile of an image may be ragged)
        // g0 .. g1, fa .. fb and the lists' "frame in group" are places in the sorted order; frame_at() gives the frame of the launch
        if (tid < g1 - g0) {                  // (read from the first barrier below on; the last item's readers have passed its last barrier)
            const unsigned long long seed = keys.frame_seed(frame_at(g0 + tid));
            key[3u * tid] = (unsigned)seed;
            key[3u * tid + 1u] = (unsigned)(seed >> 32);
            key[3u * tid + 2u] = keys.frame_image(frame_at(g0 + tid), view);
        }
        for (unsigned fa = g0; fa < g1;) {    // a run of frames with one rate image
            const unsigned cls = keys.rate_frame[frame_at(fa)];
            unsigned fb = fa + 1;
            while (fb < g1 && keys.rate_frame[frame_at(fb)] == cls) ++fb;
            if (tid == 0) cnt[0] = cnt[2] = 0;
            sync.wg();
            if (inside) {
                const T lam_t = p.noiseless[((size_t)cls * V + view) * n_pix + pix];
                const double lam = (double)lam_t;
                tab[tid] = lam;
                if (!(lam > 0.0)) {
                    for (unsigned f = fa; f < fb; ++f) p.noisy[((size_t)frame_at(f) * V + view) * n_pix + pix] = (T)(0.0 + 1e-9);
                } else if (lam < 10.0) {
                    for (unsigned f = fa; f < fb; ++f) lst0[kPoissonGroupDraws - 1u - sync.lds_add(&cnt[2], 1u)] = (f - g0) << 8 | tid;
                } else {
                    const PtrsRate r = ptrs_rate(lam);
                    const PtrsSlow sl = ptrs_slow(r);
                    tab[kPoissonGroupPix + tid] = r.b;
                    tab[2 * kPoissonGroupPix + tid] = r.a;
                    tab[3 * kPoissonGroupPix + tid] = r.vr;
                    tab[4 * kPoissonGroupPix + tid] = sl.loglam;
                    tab[5 * kPoissonGroupPix + tid] = sl.log_invalpha;
                    for (unsigned f = fa; f < fb; ++f) {
                        const unsigned* const kf = key + 3u * (f - g0);
                        const PtrsCandidate c = ptrs_candidate(r, ptrs_block(kf[0], kf[1], kf[2], pix, 0u));
                        if (ptrs_squeeze(r, c)) p.noisy[((size_t)frame_at(f) * V + view) * n_pix + pix] = (T)(c.k + 1e-9);
                        else lst0[sync.lds_add(&cnt[0], 1u)] = (f - g0) << 8 | tid;
                    }
                }
            }
            sync.wg();
            // lam >= 10: attempt `blk` of every draw still listed
            unsigned n = cnt[0];
            const unsigned n_small = cnt[2];
            unsigned *cur = lst0, *nxt = lst1;
            unsigned ci = 0;
            for (unsigned blk = 0; n > 0; ++blk) {
                if (tid == 0) cnt[ci ^ 1u] = 0;
                sync.wg();
                const bool last = blk + 1 == kPoissonMaxBlocks;
                for (unsigned q = tid; q < n; q += (unsigned)kPoissonGroupPix) {
                    const unsigned e = cur[q], px = e & 255u, f = frame_at(g0 + (e >> 8));
                    const unsigned* const kf = key + 3u * (e >> 8);
                    const PtrsRate r = table_rate(px);
                    const PtrsCandidate c = ptrs_candidate(r, ptrs_block(kf[0], kf[1], kf[2], tile * kPoissonGroupPix + px, blk));
                    const bool done = ptrs_accept(r, c, [tab, px]() {
                        PtrsSlow s;
                        s.loglam = tab[4 * kPoissonGroupPix + px];
                        s.log_invalpha = tab[5 * kPoissonGroupPix + px];
                        return s;
                    });
                    if (done || last) p.noisy[((size_t)f * V + view) * n_pix + tile * kPoissonGroupPix + px] = (T)((done || c.k >= 0.0 ? c.k : 0.0) + 1e-9);
                    else nxt[sync.lds_add(&cnt[ci ^ 1u], 1u)] = e;   // (at most n <= front region: never reaches the small rates at the back of list 0)
                }
                sync.wg();
                n = cnt[ci ^ 1u];
                ci ^= 1u;
                unsigned* const t = cur;
                cur = nxt;
                nxt = t;
            }
            // 0 < lam < 10: multiplication method, one draw per lane
            for (unsigned q = tid; q < n_small; q += (unsigned)kPoissonGroupPix) {
                const unsigned e = lst0[kPoissonGroupDraws - 1u - q], px = e & 255u, f = frame_at(g0 + (e >> 8));
                p.noisy[((size_t)f * V + view) * n_pix + tile * kPoissonGroupPix + px] =
                    (T)(philox_poisson(tab[px], (unsigned long long)key[3u * (e >> 8) + 1u] << 32 | key[3u * (e >> 8)], key[3u * (e >> 8) + 2u], tile * kPoissonGroupPix + px) + 1e-9);
            }
            sync.wg();                        // the lists and the table are free for the next run
            fa = fb;
        }
    }
}

}  // namespace rl
