#include "qmcp-solver/quasi_mcp_hip_quality_solver.hpp"

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <stdexcept>
#include <vector>

namespace qmcp {
namespace {

// as QuasiMcpHipSolver: a failed device call ends the process, like the reference's GPU solver
[[noreturn]] void die(const char* what, int rc) {
    std::fprintf(stderr, "[ERROR] quasi-mcp-hip-quality: %s failed (%d): %s\n", what, rc, qmcp_hip_last_error());
    std::terminate();
}

}  // namespace

// SOAPairedReads::qualities holds each read's MAPQ, or its graded quality under AmpliconBehaviour::GRADE.  Reads of
// several references (per_reference) take the by-contig entry, as QuasiMcpHipSolver does; unplaced reads are never kept.
std::unique_ptr<Solution> QuasiMcpHipQualitySolver::solve(std::uint32_t required_cover, bam_api::BamApi& bam_api) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    if (reads.has_strata())
        throw std::invalid_argument("stratified downsampling does not take a solver that grades by quality");
    const bool by_contig = reads.has_contig_ids();
    if (by_contig && reads.contig_ids.size() != n) die("per-reference reads without one contig id each", QMCP_EINVAL);
    if (reads.qualities.size() != n) die("reads without one quality each", QMCP_EINVAL);
    if (!by_contig && reads.ref_genome_length > UINT32_MAX) die("narrowing ref_genome_length", QMCP_ERANGE);
    if (ctx_ == nullptr) {
        const int rc = qmcp_hip_create(device_, &ctx_);
        if (rc != QMCP_OK) die("qmcp_hip_create", rc);
    }
    if (bam_api.has_targets()) return solve_targets(required_cover, reads, bam_api.get_targets(), true, t0);
    std::vector<std::uint32_t> starts(n), ends(n);
    for (std::size_t i = 0; i < n; ++i) {
        if (by_contig && reads.contig_ids[i] == QMCP_NO_CONTIG) continue;  // (zero-initialised)
        if (reads.start_inds[i] > UINT32_MAX || reads.end_inds[i] > UINT32_MAX) die("narrowing a coordinate", QMCP_ERANGE);
        starts[i] = static_cast<std::uint32_t>(reads.start_inds[i]);
        ends[i] = static_cast<std::uint32_t>(reads.end_inds[i]);
    }
    static_assert(sizeof(bam_api::ReadQuality) == sizeof(std::uint32_t), "ReadQuality is uint32 (read.hpp)");
    const std::uint32_t* q = reads.qualities.data();
    std::vector<std::uint64_t> mask((n + 63) / 64, 0);
    int rc;
    if (by_contig) {
        rc = qmcp_hip_solve_quality_by_contig_host(ctx_, starts.data(), ends.data(), reads.contig_ids.data(), q, n,
                                                   reads.contig_lengths.data(),
                                                   (std::uint32_t)reads.contig_lengths.size(), required_cover,
                                                   mask.data(), &stats_, &qstats_);
        if (rc != QMCP_OK) die("qmcp_hip_solve_quality_by_contig_host", rc);
    } else {
        const std::uint64_t offsets[2] = {0, n};
        const std::uint32_t length = static_cast<std::uint32_t>(reads.ref_genome_length);
        rc = qmcp_hip_solve_quality_host(ctx_, starts.data(), ends.data(), q, n, offsets, &length, 1, required_cover,
                                         mask.data(), &stats_, &qstats_);
        if (rc != QMCP_OK) die("qmcp_hip_solve_quality_host", rc);
    }
    breakdown_ = qmcp_hip_host_breakdown{};
    if (complete_pairs_) {
        rc = qmcp_hip_complete_pairs_host(ctx_, mask.data(), n);  // (leaves the completed mask in the context)
        if (rc != QMCP_OK) die("qmcp_hip_complete_pairs_host", rc);
    }
    return expand_kept(n, t0);
}

}  // namespace qmcp
