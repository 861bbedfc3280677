// Driver of genome-downsampler_amd/csrc/ladder_plan.h for tests/test_ladder_cpu.py (g++ alone, no HIP).
// One request per stdin line:
//   c <n_levels> <coverage>...         -> "rc=<code> bad=<level>"      ("c -1" passes a NULL list with n_levels 1)
//   n <n_contigs> <off>... | <rank>... -> "rc=<code> next=<o0,o1,...>" (n_contigs + 1 offsets, then as many ranks)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ladder_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind == 'c') {
            long long n = 0;
            in >> n;
            std::vector<uint32_t> cov;
            unsigned long long v;
            while (in >> v) cov.push_back((uint32_t)v);
            uint32_t bad = 77;
            const int rc = n < 0 ? qmcp::check_ladder_coverages(nullptr, 1, &bad)
                                 : qmcp::check_ladder_coverages(cov.data(), (uint32_t)n, &bad);
            std::printf("rc=%d bad=%u\n", rc, bad);
        } else if (kind == 'n') {
            uint32_t n_contigs = 0;
            in >> n_contigs;
            std::vector<uint64_t> offs((size_t)n_contigs + 1);
            std::vector<uint32_t> ranks((size_t)n_contigs + 1);
            for (auto& o : offs) in >> o;
            std::string bar;
            in >> bar;
            for (auto& r : ranks) in >> r;
            std::vector<uint64_t> next;
            const int rc = qmcp::ladder_next_offsets(offs.data(), ranks.data(), n_contigs, next);
            std::printf("rc=%d next=", rc);
            for (size_t k = 0; k < next.size(); ++k) std::printf("%s%llu", k ? "," : "", (unsigned long long)next[k]);
            std::printf("\n");
        }
    }
    return 0;
}
