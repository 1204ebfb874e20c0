// cycle_schedule.hpp -- how a batch is cut into slices, and the streams and events of one run over those slices.
// Host only, no HIP: the CPU tests compile it as it is (tests/emu/cycle_schedule_test.cpp).
//
// A run (rlsted.cpp run_slices) iterates the slices of the batch on up to four LANES -- HIP streams of the plan -- that fork off
// the context's stream and join it again; a CYCLE is a run that first simulates and draws every slice's measurement.  Everything
// that decides which stream an operation goes to and which event it waits for is cycle_schedule() below: it returns the ordered
// list of stream operations, run_slices enqueues the list as it stands, and tests/test_cycle_schedule_cpu.py replays it into a
// happens-before model.  What a LOOP operation launches is not part of the schedule.
#pragma once

#include <algorithm>
#include <vector>

#include "object_classes.hpp"

namespace rl {

constexpr int kMaxLanes = 4;

// ---- frame chunks: run the whole K-iteration loop on a slice of the batch whose working set (spectra + measurement + estimate)
// fits the 256 MiB Infinity Cache, so the inter-kernel traffic is served on die instead of from HBM.
struct ChunkInputs {
    int B = 1, V = 1;
    size_t n_img = 0, n_spec = 0;   // pixels of an image, complex elements of a spectrum image
    size_t esize = 4;
    bool one_buffer = false, accel = false, tv = false, pair = false;   // the loop at hand
    bool chunk_mb_set = false;      // RLSTED_CHUNK_MB
    double chunk_mb = 0;
    int lanes = 2;
    int col_tile = 8, kx = 1;       // columns per tile of the column kernels, spectrum columns
};

inline int chunk_frames(const ChunkInputs& p) {
    const int B = p.B, V = p.V;
    // per slice; `lanes` slices are in flight at once, together about the 256 MiB Infinity Cache
    const double budget_mb = p.chunk_mb_set ? p.chunk_mb : (p.lanes > 1 ? 108.0 : 288.0);
    const double specs = p.one_buffer ? 1.0 : 1.0 + V;   // spectra alive in an iteration
    const double per_frame = (specs * 2.0 * p.n_spec + (1.0 + V + (p.accel ? 3.0 : 0.0) + (p.tv ? 1.0 : 0.0)) * p.n_img) * p.esize;   // (+ x, y, g; + w)
    // Frames of 32 MB and more (2048^2 up) do not live in the Infinity Cache whatever the slice: there the slice
    // only has to fill the chip -- ~1 GB per slice measured best at 2048^2 (point 658 -> 713, 4 views 180 -> 192
    // frames/s over 2-frame / 1-frame slices).
    int c = (int)((!p.chunk_mb_set && per_frame >= 32.0 * 1048576.0 ? 1024.0 : budget_mb) * 1048576.0 / per_frame);
    // many views: at least 8 frames per slice when no budget was given -- fewer leave the column
    // kernels (37 workgroups per 512^2 frame) too small to fill the chip (6 / 8 views: +10 % / +7 %)
    if (!p.chunk_mb_set && c < 8 && per_frame * 8.0 <= 300.0 * 1048576.0) c = 8;
    // ... and enough frames for the column launches to fill the chip once (two 8-wave workgroups per CU): 512^2 has 37 column
    // tiles per frame, so 16 frames -- measured 3 / 4 views 6968 -> 7826 / 5840 -> 6100 frames/s over 8-frame slices
    if (!p.chunk_mb_set && V > 1) {
        const int cw = p.col_tile > 0 ? p.col_tile : 8, tiles = (p.kx + cw - 1) / cw;
        const int need = ((512 + tiles - 1) / tiles + 7) / 8 * 8;
        if (c < need && per_frame * need <= 300.0 * 1048576.0) c = need;
    }
    if (c < 1) c = 1;
    if (c >= B) return B;
    // equal slices (a short last slice would run its 4 launches per iteration nearly empty; slices BALANCED to within one frame --
    // 6 6 5 5 5 5 instead of 6 6 6 6 6 2 for 32 frames -- measured +1 % at 2048^2 x 4 views and -1 % at 512^2 x 4 views, 250 frames: not done)
    const int fit = c;                       // frames the budget holds
    const int slices = (B + c - 1) / c;
    c = (B + slices - 1) / slices;
    if (c > 8) {                               // whole groups of 8 frames: up if that still fits the budget, down otherwise
        const int up = (c + 7) / 8 * 8;
        c = up <= fit ? up : std::max(8, fit / 8 * 8);
    }
    if (p.pair && (c & 1)) ++c;   // slices of whole frame pairs
    return c >= B ? B : c;
}

// ---- the schedule of one run
constexpr int kCtxStream = -1;   // the context's stream; 0 .. kMaxLanes - 1: the lanes
enum class OpKind { WAIT, RECORD, WORK };
// FORK: the context's stream where the lanes leave it.  DONE[l]: the end of lane l (the join).  RATES_READY: behind the class
// simulation.  DRAWN[l]: behind lane l's last in-lane draw from the class rates.  BEGUN[l]: on lane l in front of a slice's
// loop.  DRAWN_AHEAD[l]: behind the draw, on the context's stream, of the slice that lane l takes next.
enum class EventKind { NONE, FORK, DONE, DRAWN, BEGUN, DRAWN_AHEAD, RATES_READY };
// CLASS_SIM: H of every class the sharing slices hold.  SIMULATE_SLICE: H of every frame of a slice that does not share.
// DRAW_IN_LANE / DRAW_AHEAD: the slice's Poisson draw, at the head of its lane / on the context's stream.
// LOOP: start the estimate, the iterations, the checkpoints.
enum class WorkKind { NONE, CLASS_SIM, SIMULATE_SLICE, DRAW_IN_LANE, DRAW_AHEAD, LOOP };

struct StreamOp {
    OpKind op = OpKind::WORK;
    int stream = kCtxStream;
    EventKind event = EventKind::NONE;   // WAIT, RECORD
    int lane = 0;                        //   the lane of a per-lane event
    WorkKind work = WorkKind::NONE;      // WORK
    int slice = 0;                       //   (not CLASS_SIM)
    bool shared = false;                 //   a draw: from the class rates, not from the slice's own simulation
    bool join = false;                   // part of the join at the end: enqueued also after an earlier operation failed
};

// What a cycle leaves behind for the next one.
struct CycleState {
    bool lanes_open = false;                                  // the lanes were left unjoined (cycle_follows)
    bool begun_set[kMaxLanes] = {false, false, false, false};   // BEGUN[l] is of a loop that may still be running: its lane is open
    bool drawn_set[kMaxLanes] = {false, false, false, false};   // DRAWN[l] is behind a shared draw that no class simulation has waited for
};

struct CycleInputs {
    int B = 1, cf = 1, lanes = 1, V = 1;   // frames, frames per slice (chunk_frames), the plan's lane count, views
    bool draws = false;                    // a simulate + deconvolve cycle: every slice first draws its measurement
    bool share = false;                    // ... and the share layout is of slices of cf frames (share_possible() && share_cf == cf)
    int share_classes = 0;                 // compact images of that layout
    const SliceShare* share_slices = nullptr;   // [slices] of that layout (nrep > 0: the slice shares)
    bool draw_ahead = false;               // RLSTED_DRAW_AHEAD
    bool cycle_follows = false;            // another cycle follows at once (rl_deconv_bench_cycles)
    CycleState before;
};

struct CycleSchedule {
    std::vector<StreamOp> ops;
    int slices = 0, lanes = 0;             // lanes in use: min(slices, the plan's)
    bool forks = false, joins = false;
    int shared_slices = 0, draws_ahead = 0, sim_images = 0;   // sim_images: images H is computed for
    CycleState after;                      // (when every operation was enqueued)
};

// `out` is the caller's to keep between cycles: the list is rebuilt in place.
inline void cycle_schedule(const CycleInputs& in, CycleSchedule& out) {
    std::vector<StreamOp>& ops = out.ops;
    ops.clear();
    auto wait = [&](int stream, EventKind e, int lane, bool join = false) {
        ops.push_back({OpKind::WAIT, stream, e, lane, WorkKind::NONE, 0, false, join});
    };
    auto record = [&](EventKind e, int lane, int stream, bool join = false) {
        ops.push_back({OpKind::RECORD, stream, e, lane, WorkKind::NONE, 0, false, join});
    };
    auto work = [&](int stream, WorkKind w, int slice, bool shared = false) {
        ops.push_back({OpKind::WORK, stream, EventKind::NONE, 0, w, slice, shared, false});
    };

    const int B = in.B, cf = in.cf;
    const int slices = (B + cf - 1) / cf;
    const int nl = slices < in.lanes ? slices : in.lanes;
    CycleState st = in.before;
    out.slices = slices;
    out.lanes = nl;
    out.shared_slices = out.draws_ahead = out.sim_images = 0;
    // Lanes stay open between the back-to-back cycles of rl_deconv_bench_cycles (cycle_follows): slice s of every cycle
    // goes to the same lane, so stream order alone keeps each slice's buffers consistent and the lanes need not meet.
    const bool keep_open = in.cycle_follows && nl > 1;
    out.forks = nl > 1 && !st.lanes_open;
    if (out.forks) {
        record(EventKind::FORK, 0, kCtxStream);
        for (int l = 0; l < nl; ++l) wait(l, EventKind::FORK, 0);
        for (bool& b : st.begun_set) b = false;   // (nothing of an earlier cycle is still running)
    }
    const bool share = in.draws && in.share;
    auto shares = [&](int sl) { return share && in.share_slices[sl].nrep > 0; };
    auto lane_stream = [&](int sl) { return nl > 1 ? sl % nl : kCtxStream; };
    // Draws ahead (RLSTED_DRAW_AHEAD=1; what it measured and why it is off by default: plan_options.hpp PlanOptions).  The sampler is
    // bound by vector issue, the RL kernels by the memory system, yet a slice's full-width draw at the head of its lane floods
    // every SIMD and the other lane's loop all but stops beside it.  So the draw of a SHARING slice sl -- it reads the class rates
    // only -- goes to the context's stream, a capped number of workgroups wide, behind the "begun" event of the slice IN FRONT of
    // sl on its lane: it runs in the background of that slice's loop and is finished long before lane sl % nl wants it (the lane
    // waits for DRAWN_AHEAD).  The context's stream, not one more: it has nothing to do between the fork and the join of the lanes,
    // whatever it holds is in front of the join by stream order (error paths included), and it has a hardware queue of its own.  A
    // further stream does not: the runtime deals a process's streams to 4 hardware queues by default, the null stream, the context's
    // and two lanes take them, and a fifth stream shares a queue with one of the lanes, where its waits stop that lane's launches
    // -- measured, the headline on a stream of its own: 58.7 ms per cycle against the parent's 47.5 ms in a process with one plan
    // (profiles/draw_ahead).  The begun event is the throttle -- the context's stream is never more than one slice per lane ahead
    // of the loops -- and what frees `meas` of slice sl: the loop that read it last (the cycle before) precedes the slice in front
    // on the same lane.  Across cycles whose lanes stay open the slice in front is the lane's last of the cycle before; a lane that
    // holds ONE slice would draw into the measurement that slice still iterates on, and keeps its in-lane draw, as do the first
    // slices of a cycle that follows nothing (no loop to hide behind) and slices that do not share.
    // (Round 1 tried the simulation of all slices ahead of the RL lanes on a stream of its own and lost, 16.5 k against 17.2 k
    // frames/s: 2.3 GB of per-frame simulation spectra streamed through the Infinity Cache with nothing bounding the run-ahead
    // pushed the iterating slices' working sets out.  A sharing slice's draw reads one class image and writes its measurement,
    // 33.5 MB at 512^2, and at most one per lane is ahead.)
    const bool ahead = in.draw_ahead && share && in.share_classes > 0 && nl > 1 && slices > nl;
    auto draws_ahead = [&](int sl) {   // (a lane's first slice: before that lane's begun flag is set again below)
        if (!ahead || !shares(sl)) return false;
        const int on_lane = (slices - sl % nl + nl - 1) / nl;   // slices that go to this one's lane
        return sl >= nl || (st.begun_set[sl] && on_lane >= 2);
    };
    // The cycle's class simulation: H of every class the sharing slices hold, once, on the stream that starts the cycle's first
    // slice -- or, with draws ahead, on the context's stream: behind the last draw of the cycle before by stream order and beside
    // that cycle's tail, not behind lane 0's last slice.  It replaces the rates the cycle before drew from, so it first waits for
    // that cycle's last shared draw on every lane (lanes that stay open between cycles do not meet otherwise); the other lanes
    // wait for it before their first shared draw.
    bool lane_waits[kMaxLanes] = {false, false, false, false};   // lane l has yet to wait for RATES_READY
    int lane_last_shared[kMaxLanes] = {-1, -1, -1, -1};          // the last sharing slice that draws in lane l
    if (share && in.share_classes > 0) {
        const int s = ahead ? kCtxStream : lane_stream(0);
        for (int l = 0; l < kMaxLanes; ++l) {
            if (!st.drawn_set[l]) continue;
            st.drawn_set[l] = false;
            wait(s, EventKind::DRAWN, l);
        }
        work(s, WorkKind::CLASS_SIM, 0);
        out.sim_images += in.share_classes * in.V;
        if (nl > 1) {
            record(EventKind::RATES_READY, 0, s);
            for (int l = ahead ? 0 : 1; l < nl; ++l) lane_waits[l] = true;
            for (int sl = 0; sl < slices; ++sl)   // (in-lane draws; those on the context's stream precede the next simulation there)
                if (shares(sl) && !draws_ahead(sl)) lane_last_shared[sl % nl] = sl;
        }
    }
    for (int sl = 0, f0 = 0; f0 < B; f0 += cf, ++sl) {
        const int nf = f0 + cf <= B ? cf : B - f0;
        const int s = lane_stream(sl), lane = nl > 1 ? sl % nl : 0;
        if (in.draws && draws_ahead(sl)) {   // behind the class simulation by stream order: no wait for RATES_READY
            wait(kCtxStream, EventKind::BEGUN, lane);
            work(kCtxStream, WorkKind::DRAW_AHEAD, sl, true);
            record(EventKind::DRAWN_AHEAD, lane, kCtxStream);
            wait(s, EventKind::DRAWN_AHEAD, lane);
            ++out.shared_slices;
            ++out.draws_ahead;
        } else if (in.draws) {
            // (with draws ahead every lane waits once, a slice that does not share too: whatever the context's stream held before the
            // class simulation -- accel_reset's memset -- then precedes the lane's loops of this cycle as it does when the lanes fork)
            if ((shares(sl) || ahead) && lane_waits[lane]) {
                wait(s, EventKind::RATES_READY, 0);
                lane_waits[lane] = false;
            }
            if (shares(sl)) {   // every frame draws from its class's rates, which the class simulation left in the compact buffer
                ++out.shared_slices;
            } else {
                work(s, WorkKind::SIMULATE_SLICE, sl);
                out.sim_images += nf * in.V;
            }
            work(s, WorkKind::DRAW_IN_LANE, sl, shares(sl));
            if (lane_last_shared[lane] == sl) {   // (several lanes only)
                record(EventKind::DRAWN, lane, s);
                st.drawn_set[lane] = true;
            }
        }
        if (ahead) {   // the throttle of the draw of the next slice on this lane
            record(EventKind::BEGUN, sl % nl, s);
            st.begun_set[sl % nl] = true;
        }
        work(s, WorkKind::LOOP, sl);
    }
    out.joins = nl > 1 && !keep_open;
    if (out.joins) {   // the context's stream continues after every lane
        for (int l = 0; l < nl; ++l) {
            record(EventKind::DONE, l, l, true);
            wait(kCtxStream, EventKind::DONE, l, true);
        }
    }
    if (nl > 1) st.lanes_open = keep_open;
    out.after = st;
}

}  // namespace rl
