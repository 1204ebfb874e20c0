// plan_options_test.cpp -- the switch table of a plan (csrc/plan_options.hpp) on the CPU: tests/test_plan_options_cpu.py builds this
// with the address and undefined-behaviour sanitizers and feeds it cases on stdin.
//   env NAME VALUE            the environment of the next plan (unset again after it)
//   plan DTYPE N_PSF [TEXT]   DTYPE f32 / f64; TEXT: the options text, the rest of the line
// Per plan one line: `ok` and the table as name=value words, or `error` and the message.  max_draw_grid and spec_quant are what
// rlsted.cpp passes in a product build: aux_kernels.hpp kPoissonGrid = 4096, conv_kernels.hpp RL_SPEC_QUANT = 0.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../rescan_line_sted_amd/csrc/plan_options.hpp"

int main() {
    std::string line;
    std::vector<std::string> set;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string word;
        if (!(in >> word)) continue;
        if (word == "env") {
            std::string name, value;
            in >> name >> value;
            setenv(name.c_str(), value.c_str(), 1);
            set.push_back(name);
            continue;
        }
        if (word != "plan") {
            std::fprintf(stderr, "unknown line: %s\n", line.c_str());
            return 2;
        }
        std::string dtype, text;
        int n_psf = 0;
        in >> dtype >> n_psf;
        std::getline(in, text);
        rl::OptionLookup lookup;
        std::string err;
        if (!lookup.parse(text.c_str(), &err)) {
            std::printf("error %s\n", err.c_str());
        } else {
            const rl::PlanOptions o = rl::plan_options(lookup, dtype == "f32" ? RL_F32 : RL_F64, n_psf, 4096, 0);
            if (const std::string* name = lookup.unasked()) {
                std::printf("error option '%s' is no switch of a plan\n", name->c_str());
            } else {
                std::printf("ok chunk_mb_set=%d chunk_mb=%.17g lanes=%d draw_ahead=%d draw_grid=%d poisson_groups=%d inplace=%d col_order=%d "
                            "pair=%d pair_max_ratio=%.17g sub_one=%d fuse_views=%d col_split=%d real_psf=%d ones_shortcut=%d share_objects=%d "
                            "sep=%d sep_one=%d direct=%d sep_th=%d q_exp_est_set=%d q_exp_ratio_set=%d q_exp_est=%d q_exp_ratio=%d\n",
                            o.chunk_mb_set, o.chunk_mb, o.lanes, o.draw_ahead, o.draw_grid, o.poisson_groups, o.inplace, o.col_order, o.pair,
                            o.pair_max_ratio, o.sub_one, o.fuse_views, o.col_split, o.real_psf, o.ones_shortcut, o.share_objects, o.sep,
                            o.sep_one, o.direct, o.sep_th, o.q_exp_est_set, o.q_exp_ratio_set, o.q_exp_est, o.q_exp_ratio);
            }
        }
        for (const std::string& name : set) unsetenv(name.c_str());
        set.clear();
    }
    return 0;
}
