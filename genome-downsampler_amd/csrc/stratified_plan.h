// stratified_plan.h -- how a stratified solve (qmcp_hip_solve_stratified_*) is cut into calls of the solver.
//
// Plain C++17 (no HIP): api/stratified.inc.hip includes it, and so can a host-only test.  The reads have been grouped
// on the device once by the stratum-major key  stratum * n_contigs + contig,  so a stratum's contigs are adjacent in
// grouped order and one solver call can carry one coverage cap.  What is left is to cut every stratum that has a cap
// and reads into batches that each fit one solver call; the packing rule itself is by_contig_plan.h's, applied to one
// stratum at a time, so a batch never crosses a stratum boundary.
#ifndef QMCP_STRATIFIED_PLAN_H
#define QMCP_STRATIFIED_PLAN_H
#include <cstdint>
#include <vector>

#include "by_contig_plan.h"
#include "qmcp_hip.h"

namespace qmcp {

constexpr uint32_t kMaxStrata = 65536;                // strata per stratified call
constexpr uint64_t kMaxStratumGroups = 1ull << 24;    // n_strata * n_contigs: the grouping key's limit

// contigs [first_contig, first_contig + n_contigs) of stratum `stratum`: the grouped reads [first_read, first_read +
// n_reads), solved at coverage M (the stratum's cap)
struct StratumBatch {
    uint32_t stratum = 0;
    uint32_t first_contig = 0, n_contigs = 0;
    uint64_t first_read = 0, n_reads = 0;
    uint64_t positions = 0;
    uint32_t M = 0;
};

// read_counts[s * n_contigs + c]: the placed reads of stratum s on contig c (the grouped order is exactly this order).
// A stratum with cap 0 or without reads produces no batch; every other stratum's contigs -- those without reads
// included -- land in exactly one batch each.  QMCP_ERANGE, with the pair in *bad_stratum / *bad_contig, when one
// (stratum, contig) of a stratum that is solved exceeds a limit on its own; QMCP_EINVAL when a table is missing or a
// count is 0.
inline int plan_stratum_batches(const uint64_t* read_counts, const uint32_t* lengths, uint32_t n_contigs,
                                const uint32_t* max_coverages, uint32_t n_strata, std::vector<StratumBatch>& out,
                                uint32_t* bad_stratum, uint32_t* bad_contig, uint64_t max_reads = kBatchMaxReads,
                                uint64_t max_positions = kBatchMaxPositions) {
    out.clear();
    if (!read_counts || !lengths || !max_coverages || n_contigs == 0 || n_strata == 0) return QMCP_EINVAL;
    uint64_t first_read = 0;  // of the stratum, in grouped order
    std::vector<ContigBatch> part;
    for (uint32_t s = 0; s < n_strata; ++s) {
        const uint64_t* counts = read_counts + (uint64_t)s * n_contigs;
        uint64_t total = 0;
        for (uint32_t c = 0; c < n_contigs; ++c) total += counts[c];
        if (max_coverages[s] != 0 && total != 0) {
            uint32_t bad = 0;
            const int rc = plan_contig_batches(counts, lengths, n_contigs, part, &bad, max_reads, max_positions);
            if (rc != QMCP_OK) {
                if (bad_stratum) *bad_stratum = s;
                if (bad_contig) *bad_contig = bad;
                out.clear();
                return rc;
            }
            for (const ContigBatch& b : part) {
                StratumBatch sb;
                sb.stratum = s;
                sb.first_contig = b.first_contig;
                sb.n_contigs = b.n_contigs;
                sb.first_read = first_read + b.first_read;
                sb.n_reads = b.n_reads;
                sb.positions = b.positions;
                sb.M = max_coverages[s];
                out.push_back(sb);
            }
        }
        first_read += total;
    }
    return QMCP_OK;
}

}  // namespace qmcp
#endif
