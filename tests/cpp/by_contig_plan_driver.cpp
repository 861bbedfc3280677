// by_contig_plan_driver.cpp -- the by-contig batch planner (genome-downsampler_amd/csrc/by_contig_plan.h) on the CPU, for
// tests/test_by_contig_cpu.py.  One table per line of stdin:
//   max_reads max_positions n_contigs reads_0 length_0 reads_1 length_1 ...     (max_* == 0: the library's limits)
// one line per table on stdout:
//   rc=<status> bad=<contig or -1> batches=<first_contig>,<n_contigs>,<first_read>,<n_reads>,<positions>;...
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "by_contig_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned long long max_reads = 0, max_positions = 0;
        unsigned n = 0;
        if (!(in >> max_reads >> max_positions >> n)) continue;
        std::vector<uint64_t> reads(n);
        std::vector<uint32_t> lengths(n);
        for (unsigned c = 0; c < n; ++c) {
            unsigned long long r = 0, l = 0;
            in >> r >> l;
            reads[c] = r;
            lengths[c] = (uint32_t)l;
        }
        std::vector<qmcp::ContigBatch> batches;
        uint32_t bad = 0xFFFFFFFFu;
        const int rc = qmcp::plan_contig_batches(reads.data(), lengths.data(), n, batches, &bad,
                                                 max_reads ? max_reads : qmcp::kBatchMaxReads,
                                                 max_positions ? max_positions : qmcp::kBatchMaxPositions);
        std::printf("rc=%d bad=%lld batches=", rc, bad == 0xFFFFFFFFu ? -1ll : (long long)bad);
        for (size_t b = 0; b < batches.size(); ++b)
            std::printf("%s%u,%u,%llu,%llu,%llu", b ? ";" : "", batches[b].first_contig, batches[b].n_contigs,
                        (unsigned long long)batches[b].first_read, (unsigned long long)batches[b].n_reads,
                        (unsigned long long)batches[b].positions);
        std::printf("\n");
    }
    return 0;
}
