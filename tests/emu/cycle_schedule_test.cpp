// cycle_schedule_test.cpp -- stand-alone driver of csrc/cycle_schedule.hpp for tests/test_cycle_schedule_cpu.py.
// stdin, any number of cases:
//   chunk B V n_img n_spec esize one_buffer accel tv pair chunk_mb_set chunk_mb lanes col_tile kx
//   chain B cf lanes V draws share share_classes draw_ahead cycles, then nrep of every slice
//         a chain of `cycles` cycles: all but the last have cycle_follows, each is fed the state the one before returned
// stdout:
//   chunk: "chunk <frames per slice>"
//   chain, per cycle: "cycle <slices> <lanes> <forks> <joins> <shared_slices> <draws_ahead> <sim_images> <operations>", then one
//   line per operation -- "WAIT <stream> <event> <lane> <join>", "RECORD <stream> <event> <lane> <join>" or
//   "WORK <stream> <kind> <slice> <shared>" (stream -1: the context's) -- then "state <lanes_open> <begun x 4> <drawn x 4>"
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/cycle_schedule.hpp"

static const char* name(rl::EventKind e) {
    switch (e) {
        case rl::EventKind::FORK: return "FORK";
        case rl::EventKind::DONE: return "DONE";
        case rl::EventKind::DRAWN: return "DRAWN";
        case rl::EventKind::BEGUN: return "BEGUN";
        case rl::EventKind::DRAWN_AHEAD: return "DRAWN_AHEAD";
        case rl::EventKind::RATES_READY: return "RATES_READY";
        case rl::EventKind::NONE: break;
    }
    return "NONE";
}

static const char* name(rl::WorkKind w) {
    switch (w) {
        case rl::WorkKind::CLASS_SIM: return "CLASS_SIM";
        case rl::WorkKind::SIMULATE_SLICE: return "SIMULATE_SLICE";
        case rl::WorkKind::DRAW_IN_LANE: return "DRAW_IN_LANE";
        case rl::WorkKind::DRAW_AHEAD: return "DRAW_AHEAD";
        case rl::WorkKind::LOOP: return "LOOP";
        case rl::WorkKind::NONE: break;
    }
    return "NONE";
}

static int chunk() {
    rl::ChunkInputs p;
    int one_buffer = 0, accel = 0, tv = 0, pair = 0, mb_set = 0;
    std::cin >> p.B >> p.V >> p.n_img >> p.n_spec >> p.esize >> one_buffer >> accel >> tv >> pair >> mb_set >> p.chunk_mb >> p.lanes >>
        p.col_tile >> p.kx;
    if (!std::cin || p.B < 1 || p.V < 1) return 2;
    p.one_buffer = one_buffer != 0; p.accel = accel != 0; p.tv = tv != 0; p.pair = pair != 0; p.chunk_mb_set = mb_set != 0;
    std::printf("chunk %d\n", rl::chunk_frames(p));
    return 0;
}

static int chain() {
    rl::CycleInputs in;
    int draws = 0, share = 0, draw_ahead = 0, cycles = 0;
    std::cin >> in.B >> in.cf >> in.lanes >> in.V >> draws >> share >> in.share_classes >> draw_ahead >> cycles;
    if (!std::cin || in.B < 1 || in.cf < 1 || in.cf > in.B || in.lanes < 1 || in.lanes > rl::kMaxLanes || cycles < 1) return 2;
    std::vector<rl::SliceShare> slices((size_t)((in.B + in.cf - 1) / in.cf));
    for (rl::SliceShare& s : slices) std::cin >> s.nrep;
    if (!std::cin) return 2;
    in.draws = draws != 0; in.share = share != 0; in.draw_ahead = draw_ahead != 0;
    in.share_slices = slices.data();
    rl::CycleSchedule sch;   // kept between the cycles, as the plan keeps it
    for (int c = 0; c < cycles; ++c) {
        in.cycle_follows = c + 1 < cycles;
        rl::cycle_schedule(in, sch);
        std::printf("cycle %d %d %d %d %d %d %d %zu\n", sch.slices, sch.lanes, (int)sch.forks, (int)sch.joins, sch.shared_slices,
                    sch.draws_ahead, sch.sim_images, sch.ops.size());
        for (const rl::StreamOp& op : sch.ops) {
            if (op.op == rl::OpKind::WORK) std::printf("WORK %d %s %d %d\n", op.stream, name(op.work), op.slice, (int)op.shared);
            else std::printf("%s %d %s %d %d\n", op.op == rl::OpKind::WAIT ? "WAIT" : "RECORD", op.stream, name(op.event), op.lane, (int)op.join);
        }
        const rl::CycleState& st = sch.after;
        std::printf("state %d", (int)st.lanes_open);
        for (bool b : st.begun_set) std::printf(" %d", (int)b);
        for (bool b : st.drawn_set) std::printf(" %d", (int)b);
        std::printf("\n");
        in.before = st;
    }
    return 0;
}

int main() {
    std::string what;
    while (std::cin >> what) {
        const int rc = what == "chunk" ? chunk() : what == "chain" ? chain() : 2;
        if (rc != 0) {
            std::fprintf(stderr, "bad case: %s\n", what.c_str());
            return rc;
        }
    }
    return 0;
}
