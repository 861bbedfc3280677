// Driver of genome-downsampler_amd/csrc/pm_grid_plan.h for tests/test_pm_grid_model.py and lab/pm_grid_slots.py (g++
// alone, no HIP).  One plan per stdin line:
//   <shift> <want> <n_contigs> <length(0)> ... <length(n-1)> <reads(0)> ... <reads(n-1)>
// Answer, five lines:
//   aligned=<0|1> n_ranges=<n> aligned_ranges=<n> heaviest_global=<x> heaviest_aligned=<x>
//   pos0 / live / contig of every range of the grid taken, one line each; vbase of every contig and the axis' end
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pm_grid_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned shift = 0, n_contigs = 0;
        int want = 0;
        if (!(in >> shift >> want >> n_contigs)) continue;
        std::vector<uint64_t> poff(n_contigs + 1, 0), roff(n_contigs + 1, 0);
        for (unsigned c = 0; c < n_contigs; ++c) { unsigned long long v = 0; in >> v; poff[c + 1] = poff[c] + v; }
        for (unsigned c = 0; c < n_contigs; ++c) { unsigned long long v = 0; in >> v; roff[c + 1] = roff[c] + v; }
        const qmcp::PmGridPlan g = qmcp::pm_grid_plan(roff.data(), poff.data(), n_contigs, shift, 8192u, want);
        std::printf("aligned=%d n_ranges=%u aligned_ranges=%u heaviest_global=%.3f heaviest_aligned=%.3f\n", g.aligned, g.n_ranges,
                    g.aligned_ranges, g.heaviest_global, g.heaviest_aligned);
        const bool tables = !g.words.empty();
        auto row = [&](const uint32_t* p, unsigned count) {
            for (unsigned i = 0; tables && i < count; ++i) std::printf(i ? " %u" : "%u", p[i]);
            std::printf("\n");
        };
        row(g.pos0(), g.n_ranges);
        row(g.live(), g.n_ranges);
        row(g.contig(), g.n_ranges);
        row(g.vbase(), n_contigs + 1);
    }
    return 0;
}
