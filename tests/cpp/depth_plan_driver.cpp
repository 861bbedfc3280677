// The position batches of qmcp_hip_depth_report_*: by_contig_plan.h's plan_contig_batches with read counts of 0 and the
// position budget as a parameter.  g++ only (no HIP).  stdin: budget, n, then n contig lengths.  stdout: the return
// code (and the refused contig), then one line per batch: first_contig n_contigs positions.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "by_contig_plan.h"

int main() {
    unsigned long long budget = 0, n = 0;
    if (std::scanf("%llu %llu", &budget, &n) != 2) return 2;
    std::vector<uint32_t> lengths(n);
    for (auto& l : lengths) {
        unsigned long long v = 0;
        if (std::scanf("%llu", &v) != 1) return 2;
        l = (uint32_t)v;
    }
    const std::vector<uint64_t> no_reads(n, 0);
    std::vector<qmcp::ContigBatch> batches;
    uint32_t bad = 0xFFFFFFFFu;
    const int rc = qmcp::plan_contig_batches(no_reads.data(), lengths.data(), (uint32_t)n, batches, &bad,
                                             qmcp::kBatchMaxReads, budget ? budget : qmcp::kBatchMaxPositions);
    std::printf("%d %u\n", rc, bad);
    for (const auto& b : batches)
        std::printf("%u %u %llu\n", b.first_contig, b.n_contigs, (unsigned long long)b.positions);
    return 0;
}
