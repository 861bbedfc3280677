// pair_plan.h -- the host side of pair-aware downsampling (qmcp_hip_solve_pairs_*): which stage lists are accepted, the
// default schedule, and how one batch's contig offsets and the device's candidate ranks become the offsets of the
// stage's candidates.
//
// Plain C++17 (no HIP): api/pairs.inc.hip includes it, and so can a host-only test.  A staged solve brings the kept set
// to min(cov, T_1) first, completes the pairs, and tops up to T_2, ..., T_k = M against what is already there, so the
// targets must rise strictly -- a stage at the same or a lower target has nothing left to ask for -- begin at >= 1 and
// end at M.
#ifndef QMCP_PAIR_PLAN_H
#define QMCP_PAIR_PLAN_H
#include <cstdint>
#include <vector>

#include "qmcp_hip.h"

namespace qmcp {

constexpr uint32_t kPairTargetLimit = 0x80000000u;  // need[] carries its cut flag in the top bit: targets stay below

// The schedule of a call at max_coverage M.  stages == NULL: the default {ceil(M / 2), M} ({1} for M == 1); otherwise
// the n_stages targets as given.  QMCP_OK with the targets in `out`; QMCP_ERANGE when M or a target is 2^31 or more;
// QMCP_EINVAL for M == 0, a count that is not in 1 .. QMCP_PAIR_MAX_STAGES, a target of 0, a list that does not rise
// strictly, or a last target that is not M.  *bad (may be NULL) is the entry that breaks the rule (0 for M, a bad count).
inline int pair_schedule(const uint32_t* stages, uint32_t n_stages, uint32_t M, std::vector<uint32_t>& out, uint32_t* bad) {
    out.clear();
    if (bad) *bad = 0;
    if (M >= kPairTargetLimit) return QMCP_ERANGE;
    if (!stages) {
        if (M == 0) return QMCP_EINVAL;
        if (M > 1) out.push_back(M - M / 2);
        out.push_back(M);
        return QMCP_OK;
    }
    for (uint32_t j = 0; j < n_stages && j < QMCP_PAIR_MAX_STAGES; ++j) {
        if (stages[j] >= kPairTargetLimit) {
            if (bad) *bad = j;
            return QMCP_ERANGE;
        }
    }
    if (M == 0 || n_stages == 0 || n_stages > QMCP_PAIR_MAX_STAGES) return QMCP_EINVAL;
    for (uint32_t j = 0; j < n_stages; ++j) {
        if (stages[j] == 0 || (j > 0 && stages[j] <= stages[j - 1])) {
            if (bad) *bad = j;
            return QMCP_EINVAL;
        }
    }
    if (stages[n_stages - 1] != M) {
        if (bad) *bad = n_stages - 1;
        return QMCP_EINVAL;
    }
    out.assign(stages, stages + n_stages);
    return QMCP_OK;
}

// A stage's candidates of one batch.  offs: the batch's contig_read_offsets (n_contigs + 1 entries); ranks[k]: the
// number of candidates (reads not yet kept) before read offs[k] (what k_ladder_offsets returns on the complement
// mask).  The candidates stay in order, so contig k's run among them is [ranks[k], ranks[k + 1]): next = ranks,
// widened.  A contig without candidates stays in the table with a zero-length run.  QMCP_EINVAL when the ranks cannot
// come from a mask over these offsets: they must start at 0, never fall, and give no contig more reads than it had.
inline int pair_candidate_offsets(const uint64_t* offs, const uint32_t* ranks, uint32_t n_contigs,
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
