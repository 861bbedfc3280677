// replicates_plan.h -- the host side of a replicate split (qmcp_hip_solve_replicates_*): which coverage lists and flags
// are accepted, and how one replicate's contig offsets and the device's free ranks become the next replicate's offsets.
//
// Plain C++17 (no HIP): api/replicates.inc.hip includes it, and so can a host-only test.  Replicate r + 1 is solved on
// the reads replicate r left free, so the coverages may come in any order and repeat; each only has to be a coverage
// the solver takes (1 .. 2^31 - 1).
#ifndef QMCP_REPLICATES_PLAN_H
#define QMCP_REPLICATES_PLAN_H
#include <cstdint>
#include <vector>

#include "qmcp_hip.h"

namespace qmcp {

constexpr uint32_t kReplicateFlags = QMCP_REPLICATES_WHOLE_PAIRS | QMCP_REPLICATES_SHORTFALL;
constexpr uint32_t kReplicateCoverageLimit = 1u << 31;

// QMCP_OK for 1 <= n_replicates <= QMCP_REPLICATES_MAX coverages in 1 .. 2^31 - 1, known flag bits and, under
// QMCP_REPLICATES_WHOLE_PAIRS, an even n_reads.  Otherwise QMCP_EINVAL -- or QMCP_ERANGE for a coverage of 2^31 or
// more in a call that is otherwise well-formed up to that replicate -- with *bad (may be NULL) the first replicate whose
// coverage breaks the rule (0 for everything else).
inline int check_replicates_call(const uint32_t* coverages, uint32_t n_replicates, uint32_t flags, uint64_t n_reads,
                                 uint32_t* bad) {
    if (bad) *bad = 0;
    if (!coverages || n_replicates == 0 || n_replicates > QMCP_REPLICATES_MAX) return QMCP_EINVAL;
    if (flags & ~kReplicateFlags) return QMCP_EINVAL;
    if ((flags & QMCP_REPLICATES_WHOLE_PAIRS) && (n_reads & 1ull)) return QMCP_EINVAL;
    for (uint32_t r = 0; r < n_replicates; ++r) {
        if (coverages[r] == 0 || coverages[r] >= kReplicateCoverageLimit) {
            if (bad) *bad = r;
            return coverages[r] == 0 ? QMCP_EINVAL : QMCP_ERANGE;
        }
    }
    return QMCP_OK;
}

// One replicate on.  offs: this replicate's contig_read_offsets (n_contigs + 1 entries); free_ranks[k]: the number of
// reads before read offs[k] that stay free, offs[k] - kept_rank(offs[k]) (what k_rep_offsets returns).  The free reads
// stay in order, so contig k's run in the next replicate is [free_ranks[k], free_ranks[k + 1]): next = free_ranks,
// widened.  A contig whose reads are all taken stays in the table with a zero-length run.  QMCP_EINVAL when the ranks
// cannot come from a mask over these offsets: they must start at 0, never fall, and leave no contig more reads than it
// had.
inline int replicates_next_offsets(const uint64_t* offs, const uint32_t* free_ranks, uint32_t n_contigs,
                                   std::vector<uint64_t>& next) {
    next.clear();
    if (!offs || !free_ranks || n_contigs == 0 || free_ranks[0] != 0 || offs[0] != 0) return QMCP_EINVAL;
    next.assign((size_t)n_contigs + 1, 0);
    for (uint32_t k = 0; k < n_contigs; ++k) {
        if (offs[k + 1] < offs[k] || free_ranks[k + 1] < free_ranks[k] ||
            (uint64_t)(free_ranks[k + 1] - free_ranks[k]) > offs[k + 1] - offs[k]) {
            next.clear();
            return QMCP_EINVAL;
        }
        next[k + 1] = free_ranks[k + 1];
    }
    return QMCP_OK;
}

// the number of leading replicates without a short position
inline uint32_t replicates_n_full(const uint64_t* short_positions, uint32_t n_replicates) {
    uint32_t r = 0;
    while (r < n_replicates && short_positions[r] == 0) ++r;
    return r;
}

}  // namespace qmcp
#endif
