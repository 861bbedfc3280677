#include "qmcp-solver/quasi_mcp_hip_quality_solver.hpp"

#include <chrono>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace qmcp {

// SOAPairedReads::qualities holds each read's MAPQ, or its graded quality under AmpliconBehaviour::GRADE.  Reads of
// several references (per_reference) take the by-contig entry, as QuasiMcpHipSolver does; unplaced reads are never kept.
// As there, a failed device call ends the process, like the reference's GPU solver.
std::unique_ptr<Solution> QuasiMcpHipQualitySolver::solve(std::uint32_t required_cover, bam_api::BamApi& bam_api) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    if (reads.has_strata())
        throw std::invalid_argument("stratified downsampling does not take a solver that grades by quality");
    const bool by_contig = reads.has_contig_ids();
    if (by_contig && !one_contig_id_each(reads)) die("per-reference reads without one contig id each", QMCP_EINVAL);
    if (reads.qualities.size() != n) die("reads without one quality each", QMCP_EINVAL);
    if (!by_contig && reads.ref_genome_length > UINT32_MAX) die("narrowing ref_genome_length", QMCP_ERANGE);
    context();
    if (bam_api.has_targets()) return solve_targets(required_cover, reads, bam_api.get_targets(), true, t0);
    const Columns c = narrowed(reads);
    const std::uint32_t* q = reads.qualities.data();
    std::vector<std::uint64_t> mask((n + 63) / 64, 0);
    if (by_contig) {
        ok_or_die("qmcp_hip_solve_quality_by_contig_host",
                  qmcp_hip_solve_quality_by_contig_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), q, n,
                                                        reads.contig_lengths.data(),
                                                        (std::uint32_t)reads.contig_lengths.size(), required_cover,
                                                        mask.data(), &stats_, &qstats_));
    } else {
        const std::uint64_t offsets[2] = {0, n};
        const std::uint32_t length = static_cast<std::uint32_t>(reads.ref_genome_length);
        ok_or_die("qmcp_hip_solve_quality_host",
                  qmcp_hip_solve_quality_host(ctx_, c.starts.data(), c.ends.data(), q, n, offsets, &length, 1,
                                              required_cover, mask.data(), &stats_, &qstats_));
    }
    return finish(mask, n, t0);
}

}  // namespace qmcp
