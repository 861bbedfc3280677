// Driver of genome-downsampler_amd/csrc/budget_plan.h for tests/test_budget_cpu.py (g++ alone, no HIP).
// One search per stdin line:
//   <top> <budget> <max_span> <curve_n> <slope> <knee> <kind> <a> <b> <c> [<count(1)> ... <count(top)>]
// The curve is S(M) = slope * min(M, knee) for M < curve_n; total_bases = slope * min(top, knee); count(0) = 0 and
//   kind L: count(M) = a * M + b          kind J: count(M) = M < a ? b : c          kind T: the table that follows
// reads_placed = count(top).  Answer:
//   "m=<M*> probes=<n> limit=<n> outside=<probes outside (lo, hi)> twice=<coverages probed twice> count=<count(M*)>
//    above=<count_hi> bound=<bound_hi> hi=<hi> seq=<M1,M2,...>"
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "budget_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned long long top, budget, max_span, curve_n, slope, knee, a, b, c;
        char kind = 0;
        if (!(in >> top >> budget >> max_span >> curve_n >> slope >> knee >> kind >> a >> b >> c)) continue;
        std::vector<uint64_t> table;
        if (kind == 'T') {
            table.assign(top + 1, 0);
            for (unsigned long long m = 1; m <= top; ++m) in >> table[m];
        }
        auto count = [&](uint64_t M) -> uint64_t {
            if (M == 0) return 0;
            if (kind == 'L') return a * M + b;
            if (kind == 'J') return M < a ? b : c;
            return table[M];
        };
        std::vector<uint64_t> curve(curve_n);
        for (uint64_t m = 0; m < curve_n; ++m) curve[m] = slope * (m < knee ? m : knee);
        qmcp::BudgetPlan plan;
        plan.start(curve.data(), (uint32_t)curve_n, (uint32_t)top, (uint32_t)max_span, slope * (top < knee ? top : knee),
                   count(top), budget);
        std::set<uint32_t> seen;
        std::string seq;
        unsigned outside = 0, twice = 0;
        while (!plan.done() && plan.probes < 1000) {
            const uint32_t M = plan.next();
            if (M <= plan.lo || M >= plan.hi) ++outside;
            if (!seen.insert(M).second) ++twice;
            seq += (seq.empty() ? "" : ",") + std::to_string(M);
            plan.report(M, count(M));
        }
        std::printf("m=%u probes=%u limit=%u outside=%u twice=%u count=%llu above=%llu bound=%llu hi=%u seq=%s\n", plan.lo,
                    plan.probes, qmcp::budget_probe_limit((uint32_t)top), outside, twice, (unsigned long long)plan.count_lo,
                    (unsigned long long)plan.count_hi, (unsigned long long)plan.bound_hi, plan.hi, seq.c_str());
    }
    return 0;
}
