// Driver of genome-downsampler_amd/csrc/pair_plan.h for tests/test_pairs_cpu.py (g++ alone, no HIP).
// One request per stdin line:
//   s <M> <n_stages> <target>...       -> "rc=<code> bad=<entry> stages=<t0,t1,...>"   (n_stages -1: a NULL list, the default)
//   n <n_contigs> <off>... | <rank>... -> "rc=<code> next=<o0,o1,...>" (n_contigs + 1 offsets, then as many ranks)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pair_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind == 's') {
            unsigned long long M = 0;
            long long n = 0;
            in >> M >> n;
            std::vector<uint32_t> targets;
            unsigned long long v;
            while (in >> v) targets.push_back((uint32_t)v);
            if (n >= 0 && targets.size() < (size_t)(n > 0 ? n : 1)) targets.resize((size_t)(n > 0 ? n : 1), 0);  // (never a NULL list)
            uint32_t bad = 77;
            std::vector<uint32_t> out;
            const int rc = n < 0 ? qmcp::pair_schedule(nullptr, 0, (uint32_t)M, out, &bad)
                                 : qmcp::pair_schedule(targets.data(), (uint32_t)n, (uint32_t)M, out, &bad);
            std::printf("rc=%d bad=%u stages=", rc, bad);
            for (size_t k = 0; k < out.size(); ++k) std::printf("%s%u", k ? "," : "", out[k]);
            std::printf("\n");
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
            const int rc = qmcp::pair_candidate_offsets(offs.data(), ranks.data(), n_contigs, next);
            std::printf("rc=%d next=", rc);
            for (size_t k = 0; k < next.size(); ++k) std::printf("%s%llu", k ? "," : "", (unsigned long long)next[k]);
            std::printf("\n");
        }
    }
    return 0;
}
