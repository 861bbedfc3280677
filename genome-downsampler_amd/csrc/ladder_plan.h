// ladder_plan.h -- the host side of a coverage ladder (qmcp_hip_solve_ladder_*): which coverage lists are accepted, and
// how one level's contig offsets and the device's kept ranks become the next level's offsets.
//
// Plain C++17 (no HIP): api/ladder.inc.hip includes it, and so can a host-only test.  A ladder solves level 0 on all
// reads and level j + 1 on the reads level j kept, so the coverages must fall strictly -- a level at the same or a higher
// coverage would keep every read it is given -- and stay >= 1, which is what keeps a contig that has reads from losing
// all of them.
#ifndef QMCP_LADDER_PLAN_H
#define QMCP_LADDER_PLAN_H
#include <cstdint>
#include <vector>

#include "qmcp_hip.h"

namespace qmcp {

// QMCP_OK for 1 <= n_levels <= QMCP_LADDER_MAX_LEVELS coverages that fall strictly and end at >= 1.  Otherwise
// QMCP_EINVAL, with *bad_level (may be NULL) the first level that breaks the rule (0 for a bad count or a NULL list).
inline int check_ladder_coverages(const uint32_t* coverages, uint32_t n_levels, uint32_t* bad_level) {
    if (bad_level) *bad_level = 0;
    if (!coverages || n_levels == 0 || n_levels > QMCP_LADDER_MAX_LEVELS) return QMCP_EINVAL;
    for (uint32_t j = 0; j < n_levels; ++j) {
        if (coverages[j] == 0 || (j > 0 && coverages[j] >= coverages[j - 1])) {
            if (bad_level) *bad_level = j;
            return QMCP_EINVAL;
        }
    }
    return QMCP_OK;
}

// One level down.  offs: this level's contig_read_offsets (n_contigs + 1 entries); ranks[k]: the number of reads this
// level kept before read offs[k] (what k_ladder_offsets returns).  The kept reads stay in order, so contig k's run in
// the next level is [ranks[k], ranks[k + 1]): next = ranks, widened.  An empty contig stays in the table with a
// zero-length run.  QMCP_EINVAL when the ranks cannot come from a keep mask over these offsets: they must start at 0,
// never fall, and give no contig more reads than it had.
inline int ladder_next_offsets(const uint64_t* offs, const uint32_t* ranks, uint32_t n_contigs,
                               std::vector<uint64_t>& next) {
    next.clear();
    if (!offs || !ranks || n_contigs == 0 || ranks[0] != 0 || offs[0] != 0) return QMCP_EINVAL;
    next.assign((size_t)n_contigs + 1, 0);
    for (uint32_t k = 0; k < n_contigs; ++k) {
        if (offs[k + 1] < offs[k] || ranks[k + 1] < ranks[k] ||
            (uint64_t)(ranks[k + 1] - ranks[k]) > offs[k + 1] - offs[k]) {
            next.clear();
            return QMCP_EINVAL;
        }
        next[k + 1] = ranks[k + 1];
    }
    return QMCP_OK;
}

}  // namespace qmcp
#endif
