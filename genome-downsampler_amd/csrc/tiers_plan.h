// tiers_plan.h -- what a tiered solve (qmcp_hip_solve_tiers_*) decides on the host: whether the call is legal, and how
// every tier is cut into calls of the solver.
//
// Plain C++17 (no HIP): api/tiers.inc.hip includes it, and so can a host-only test.  The reads have been grouped on the
// device once by the tier-major key  tier * n_contigs + contig,  so a tier's contigs are adjacent in grouped order.  A
// tier is a stratum whose cap is the call's M: the cuts are stratified_plan.h's (by_contig_plan.h's packing, one tier at
// a time), so a batch never crosses a tier boundary and a tier without reads has none.
#ifndef QMCP_TIERS_PLAN_H
#define QMCP_TIERS_PLAN_H
#include <cstdint>
#include <vector>

#include "qmcp_hip.h"
#include "stratified_plan.h"

namespace qmcp {

constexpr uint32_t kMaxTiers = QMCP_TIERS_MAX;     // tiers per call
constexpr uint64_t kMaxTierGroups = 1ull << 24;    // n_tiers * n_contigs: the grouping key's limit
constexpr uint32_t kTierCoverageLimit = 1u << 31;  // M stays below it: need[] keeps its top bit for the cut flag

// why check_tiers_call refused, in the order it checks
enum TierRefusal : uint32_t {
    kTierCallOk = 0,
    kTierNoContigs,       // contig_lengths missing or n_contigs == 0                    QMCP_EINVAL
    kTierNoColumn,        // tiers == NULL                                               QMCP_EINVAL
    kTierNoTiers,         // n_tiers == 0                                                QMCP_EINVAL
    kTierTooManyTiers,    // n_tiers > QMCP_TIERS_MAX                                    QMCP_ERANGE
    kTierTooManyGroups,   // n_tiers * n_contigs > 2^24                                  QMCP_ERANGE
    kTierCoverage,        // M >= 2^31                                                   QMCP_ERANGE
    kTierTooManyReads,    // n_reads > 2^31                                              QMCP_ERANGE
};

// has_tiers: the tier column is there (a call without reads needs none)
inline int check_tiers_call(bool has_lengths, uint32_t n_contigs, bool has_tiers, uint32_t n_tiers, uint32_t M,
                            uint64_t n_reads, TierRefusal* why) {
    TierRefusal w = kTierCallOk;
    if (!has_lengths || n_contigs == 0) w = kTierNoContigs;
    else if (!has_tiers) w = kTierNoColumn;
    else if (n_tiers == 0) w = kTierNoTiers;
    else if (n_tiers > kMaxTiers) w = kTierTooManyTiers;
    else if ((uint64_t)n_tiers * n_contigs > kMaxTierGroups) w = kTierTooManyGroups;
    else if (M >= kTierCoverageLimit) w = kTierCoverage;
    else if (n_reads > (1ull << 31)) w = kTierTooManyReads;
    if (why) *why = w;
    if (w == kTierCallOk) return QMCP_OK;
    return w <= kTierNoTiers ? QMCP_EINVAL : QMCP_ERANGE;
}

// contigs [first_contig, first_contig + n_contigs) of tier `stratum`: the grouped reads [first_read, first_read +
// n_reads)
using TierBatch = StratumBatch;

// read_counts[t * n_contigs + c]: the placed reads of tier t on contig c (the grouped order is exactly this order).
// A tier without reads produces no batch; every other tier's contigs -- those without reads included -- land in exactly
// one batch each, tier by tier.  M == 0 produces none at all: nothing can be kept.  QMCP_ERANGE, with the pair in
// *bad_tier / *bad_contig, when one (tier, contig) exceeds a limit on its own.
inline int plan_tier_batches(const uint64_t* read_counts, const uint32_t* lengths, uint32_t n_contigs, uint32_t n_tiers,
                             uint32_t M, std::vector<TierBatch>& out, uint32_t* bad_tier, uint32_t* bad_contig,
                             uint64_t max_reads = kBatchMaxReads, uint64_t max_positions = kBatchMaxPositions) {
    const std::vector<uint32_t> caps(n_tiers, M);
    return plan_stratum_batches(read_counts, lengths, n_contigs, caps.data(), n_tiers, out, bad_tier, bad_contig, max_reads,
                                max_positions);
}

}  // namespace qmcp
#endif
