// plan_options.hpp -- every RLSTED_* switch of a plan: the table (PlanOptions), the one lookup behind it (OptionLookup: the entries
// given to rl_deconv_create_with first, then the environment) and plan_options(), which fills the table.  Host only, no HIP: the
// CPU tests compile it on its own (tests/emu/plan_options_test.cpp).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/rlsted.h"
#include "cycle_schedule.hpp"   // kMaxLanes

namespace rl {

// Where plan_options() asks for a switch.  The given entries are the text of rl_deconv_create_with (include/rlsted.h); a name that
// is not among them falls back to the environment.  The lookup remembers which given names were asked for: one that nobody asked
// for is no switch of a plan (unasked), so the table below stays the only list of names.
class OptionLookup {
  public:
    // text: NULL or NAME=value entries separated by whitespace.  False, and *err names the offender: an entry without '=', with an
    // empty name or value, a name given twice.
    bool parse(const char* text, std::string* err) {
        const std::string s = text ? text : "";
        const char* blank = " \t\r\n\f\v";
        for (size_t at = s.find_first_not_of(blank); at != std::string::npos;) {
            const size_t end = std::min(s.find_first_of(blank, at), s.size());
            const std::string entry = s.substr(at, end - at);
            const size_t eq = entry.find('=');
            if (eq == std::string::npos) return refuse(err, "option '" + entry + "' has no '='");
            if (eq == 0) return refuse(err, "option '" + entry + "' has no name");
            if (eq + 1 == entry.size()) return refuse(err, "option '" + entry + "' has no value");
            const std::string name = entry.substr(0, eq);
            for (const Entry& e : given)
                if (e.name == name) return refuse(err, "option '" + name + "' is given twice");
            given.push_back({name, entry.substr(eq + 1), false});
            at = s.find_first_not_of(blank, end);
        }
        return true;
    }
    // the value of a switch, or nullptr: unset
    const char* operator()(const char* name) {
        for (Entry& e : given)
            if (e.name == name) {
                e.asked = true;
                return e.value.c_str();
            }
        return getenv(name);
    }
    // after plan_options(): a given name that it did not ask for
    const std::string* unasked() const {
        for (const Entry& e : given)
            if (!e.asked) return &e.name;
        return nullptr;
    }

  private:
    struct Entry {
        std::string name, value;
        bool asked;
    };
    std::vector<Entry> given;
    static bool refuse(std::string* err, const std::string& msg) {
        if (err) *err = msg;
        return false;
    }
};

// Every RLSTED_* switch of a plan (RLSTED_DEBUG_SYNC is process wide: rl::debug_sync).  Read once,
// when the plan is created; nothing after plan_options() looks at the lookup or the environment.  The defaults are the measured optimum.
struct PlanOptions {
    // ---- schedule
    bool chunk_mb_set = false;   // RLSTED_CHUNK_MB: working set of one batch slice in MB; unset: 108 (one lane: 288) and the
    double chunk_mb = 0;         //   rules of chunk_frames() that only apply when no budget was given
    // Slices of the batch are independent: they are iterated on `lanes` HIP streams at once so that
    // the tail of one slice's kernel (the last, partly filled round of workgroups) overlaps another
    // slice's kernels.  RLSTED_LANES=1: one slice after the other on the context's stream (at most kMaxLanes).
    int lanes = 2;
    // RLSTED_DRAW_AHEAD=1: a sharing slice's Poisson draw goes to the context's stream -- idle while the lanes run --, one slice
    // per lane ahead of the loops and RLSTED_DRAW_GRID workgroups wide (at most aux_kernels.hpp kPoissonGrid), beside the loop of
    // the slice in front (cycle_schedule.hpp); unset: every slice draws at the head of its lane.  OFF by default: bench.py's
    // lone plan gains nothing (46.44 ms off, 46.59 ms on, four alternating runs each), plans in a crowded process 0.4 - 0.7 ms --
    // unless the context's stream shares a hardware queue with a lane (8 plans on 4 queues), where the same cycle takes
    // 52 - 59 ms (DESIGN.md section 4 "Draws ahead", profiles/draw_ahead).  Grid, same tables: 64 .. 512 within 0.2 ms of each other.
    bool draw_ahead = false;
    int draw_grid = 128;
    // RLSTED_POISSON_GROUPS=0: k_poisson for every draw; unset: a sharing slice's Philox draw runs k_poisson_groups, which evaluates
    // the sampler's rate-only set-up once per pixel and group of 8 frames instead of once per frame (poisson_kernels.hpp; the same
    // bits; DESIGN.md section 4 "Frame groups", profiles/poisson_groups)
    bool poisson_groups = true;
    bool inplace = true;         // RLSTED_INPLACE=0: single-view RL iterations spec_a -> spec_b -> spec_a instead of entirely in spec_a
    // RLSTED_COL_ORDER: column kernel work order, images per block of the tile order (fft_kernels.hip k_colconv):
    // 1 image-major ... >= images per launch: tile-major.  Measured at 512^2, 32-frame
    // slices: 1: 16.80 k, 2: 16.88 k, 4: 16.98 k, 8: 16.81 k, 32: 16.56 k frames/s.
    int col_order = 4;
    bool pair = false;           // RLSTED_PAIR: frame pairs in the RL loop; unset: single-view f32 plans (deconv_build)
    double pair_max_ratio = 4.0; // RLSTED_PAIR_MAX_RATIO: largest level ratio inside a pair (rl_deconv::levels_ok)
    // ---- arithmetic (each identical in exact arithmetic)
    bool sub_one = false;        // RLSTED_SUB_ONE: the second half of every iteration on `ratio - 1`; unset: f32 plans of the product build
    int fuse_views = -1;         // RLSTED_FUSE_VIEWS: -1 unset (H_t views summed in the Fourier domain on f32 plans, not on f64), 0 / 1 as
                                 //   given; 0 also asks for the reference's per-view clamp, which `ratio - 1` cannot give (rl_deconv_create)
    bool col_split = true;       // RLSTED_COL_SPLIT=0: no split column pass (rl_deconv::col_split)
    bool real_psf = true;        // RLSTED_REAL_PSF=0: keep the complex multiplier for real PSF spectra
    bool ones_shortcut = true;   // RLSTED_ONES_SHORTCUT=0: the first iteration transforms its frame of ones instead of reading spec_ones
    bool share_objects = true;   // RLSTED_SHARE_OBJECTS=0: every frame's H(object) is computed, also of frames that carry the same object
    // ---- strategy (deconv_build)
    int sep = 1;                 // RLSTED_SEP: separable stencils 0 never, 1 rank-1 PSFs with py + px <= 16, 2 whenever rank 1
    int sep_one = 1;             // RLSTED_SEP_ONE: 0 two passes, 1 one kernel up to 24 taps a side, 2 one kernel whenever the tile fits LDS
    int direct = 1;              // RLSTED_DIRECT: direct 2-D stencil 0 never, 1 up to 49 taps, 2 whenever the tile fits LDS
    int sep_th = 32;             // RLSTED_SEP_TH: tile height of the one-kernel stencils (sep_kernels.hpp sep2d): 64 when the value is
                                 //   exactly 64 and the plan is f32, else 32
    // ---- storage-precision study builds (conv_kernels.hpp RL_SPEC_QUANT): log2 of the DC bound of an estimate-type / ratio-type spectrum
    bool q_exp_est_set = false, q_exp_ratio_set = false;   // RLSTED_Q_EXP_EST, RLSTED_Q_EXP_RATIO
    int q_exp_est = 14, q_exp_ratio = 14;
};

// max_draw_grid: aux_kernels.hpp kPoissonGrid; spec_quant: conv_kernels.hpp RL_SPEC_QUANT (both headers need HIP)
inline PlanOptions plan_options(OptionLookup& get, int dtype, int n_psf, int max_draw_grid, int spec_quant) {
    PlanOptions o;
    auto flag = [&get](const char* name, bool unset) {
        const char* s = get(name);
        return s ? atoi(s) != 0 : unset;
    };
    auto number = [&get](const char* name, int unset, bool* set = nullptr) {
        const char* s = get(name);
        if (set) *set = s != nullptr;
        return s ? atoi(s) : unset;
    };
    if (const char* s = get("RLSTED_CHUNK_MB")) {
        o.chunk_mb_set = true;
        o.chunk_mb = atof(s);
    }
    o.lanes = std::min(std::max(number("RLSTED_LANES", o.lanes), 1), kMaxLanes);
    o.draw_ahead = flag("RLSTED_DRAW_AHEAD", o.draw_ahead);
    o.draw_grid = std::min(std::max(number("RLSTED_DRAW_GRID", o.draw_grid), 1), max_draw_grid);
    o.poisson_groups = flag("RLSTED_POISSON_GROUPS", o.poisson_groups);
    o.inplace = flag("RLSTED_INPLACE", o.inplace);
    o.col_order = std::max(number("RLSTED_COL_ORDER", o.col_order), 1);
    o.pair = flag("RLSTED_PAIR", dtype == RL_F32 && n_psf == 1);
    if (const char* s = get("RLSTED_PAIR_MAX_RATIO")) o.pair_max_ratio = atof(s);
    o.sub_one = flag("RLSTED_SUB_ONE", dtype == RL_F32 && spec_quant == 0);
    if (const char* s = get("RLSTED_FUSE_VIEWS")) o.fuse_views = atoi(s) != 0 ? 1 : 0;
    o.col_split = flag("RLSTED_COL_SPLIT", o.col_split);
    o.real_psf = flag("RLSTED_REAL_PSF", o.real_psf);
    o.ones_shortcut = flag("RLSTED_ONES_SHORTCUT", o.ones_shortcut);
    o.share_objects = flag("RLSTED_SHARE_OBJECTS", o.share_objects);
    o.sep = number("RLSTED_SEP", o.sep);
    o.sep_one = number("RLSTED_SEP_ONE", o.sep_one);
    o.direct = number("RLSTED_DIRECT", o.direct);
    const int th = number("RLSTED_SEP_TH", o.sep_th);   // (asked for on f64 plans too: the name is a switch there, without effect)
    o.sep_th = dtype == RL_F32 && th == 64 ? 64 : 32;
    o.q_exp_est = number("RLSTED_Q_EXP_EST", o.q_exp_est, &o.q_exp_est_set);
    o.q_exp_ratio = number("RLSTED_Q_EXP_RATIO", o.q_exp_ratio, &o.q_exp_ratio_set);
    return o;
}

}  // namespace rl
