// Driver of genome-downsampler_amd/csrc/replicates_plan.h for tests/test_replicates_cpu.py (g++ alone, no HIP).
// One request per stdin line:
//   c <n_replicates> <flags> <n_reads> <coverage>... -> "rc=<code> bad=<replicate>"   (n_replicates -1: a NULL list)
//   n <n_contigs> <off>... | <free rank>...         -> "rc=<code> next=<o0,o1,...>"  (n_contigs + 1 of each)
//   f <short positions>...                          -> "rc=0 full=<n_full>"
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "replicates_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind == 'c') {
            long long n = 0;
            unsigned long long flags = 0, n_reads = 0, v = 0;
            in >> n >> flags >> n_reads;
            std::vector<uint32_t> cov;
            while (in >> v) cov.push_back((uint32_t)v);
            uint32_t bad = 77;
            const int rc = n < 0 ? qmcp::check_replicates_call(nullptr, 1, (uint32_t)flags, n_reads, &bad)
                                 : qmcp::check_replicates_call(cov.data(), (uint32_t)n, (uint32_t)flags, n_reads, &bad);
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
            const int rc = qmcp::replicates_next_offsets(offs.data(), ranks.data(), n_contigs, next);
            std::printf("rc=%d next=", rc);
            for (size_t k = 0; k < next.size(); ++k) std::printf("%s%llu", k ? "," : "", (unsigned long long)next[k]);
            std::printf("\n");
        } else if (kind == 'f') {
            std::vector<uint64_t> sp;
            unsigned long long v = 0;
            while (in >> v) sp.push_back(v);
            std::printf("rc=0 full=%u\n", qmcp::replicates_n_full(sp.data(), (uint32_t)sp.size()));
        }
    }
    return 0;
}
