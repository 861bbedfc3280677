// by_contig_plan.h -- how a by-contig solve (qmcp_hip_solve_by_contig_*) is cut into calls of the solver.
//
// Plain C++17 (no HIP): api/by_contig.inc.hip includes it, and so can a host-only test.  The reads have been grouped
// by contig on the device once; what is left is to pack the contigs, in id order, into batches that each fit one
// solver call -- at most kBatchMaxReads reads and kBatchMaxPositions positions (check_problem's limits) -- and run the
// batches back to back.  Contigs are independent problems, so the keep mask does not depend on where the cuts fall.
#ifndef QMCP_BY_CONTIG_PLAN_H
#define QMCP_BY_CONTIG_PLAN_H
#include <cstdint>
#include <vector>

#include "qmcp_hip.h"

namespace qmcp {

constexpr uint64_t kBatchMaxReads = 1ull << 30;            // reads per solver call
constexpr uint64_t kBatchMaxPositions = (1ull << 31) - 2;  // sum of contig lengths per solver call

// contigs [first_contig, first_contig + n_contigs) of the grouped reads [first_read, first_read + n_reads)
struct ContigBatch {
    uint32_t first_contig = 0, n_contigs = 0;
    uint64_t first_read = 0, n_reads = 0;
    uint64_t positions = 0;
};

// Greedy packing in id order: a contig joins the open batch if both sums stay within the limits, else it opens the next
// one.  Every contig, empty ones included, lands in exactly one batch.  read_counts[c] is contig c's number of reads.
// QMCP_ERANGE, with the contig's id in *bad_contig, when one contig alone exceeds a limit; QMCP_EINVAL when
// n_contigs == 0.
inline int plan_contig_batches(const uint64_t* read_counts, const uint32_t* lengths, uint32_t n_contigs,
                               std::vector<ContigBatch>& out, uint32_t* bad_contig,
                               uint64_t max_reads = kBatchMaxReads, uint64_t max_positions = kBatchMaxPositions) {
    out.clear();
    if (n_contigs == 0) return QMCP_EINVAL;
    ContigBatch open;
    uint64_t next_read = 0;
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const uint64_t r = read_counts[c], p = lengths[c];
        if (r > max_reads || p > max_positions) {
            if (bad_contig) *bad_contig = c;
            out.clear();
            return QMCP_ERANGE;
        }
        if (open.n_contigs != 0 && (open.n_reads + r > max_reads || open.positions + p > max_positions)) {
            out.push_back(open);
            open = ContigBatch();
        }
        if (open.n_contigs == 0) {
            open.first_contig = c;
            open.first_read = next_read;
        }
        open.n_contigs++;
        open.n_reads += r;
        open.positions += p;
        next_read += r;
    }
    out.push_back(open);
    return QMCP_OK;
}

}  // namespace qmcp
#endif
