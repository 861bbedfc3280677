#include "qmcp-solver/quasi_mcp_hip_solver.hpp"

#include <chrono>
#include <cstdio>
#include <exception>
#include <algorithm>
#include <fstream>
#include <limits>
#include <stdexcept>
#include <vector>

namespace qmcp {

static_assert(sizeof(bam_api::Index) == sizeof(std::uint64_t), "Index is size_t on an LP64 host (read.hpp:11)");
static_assert(sizeof(bam_api::ReadIndex) == sizeof(std::uint64_t), "ReadIndex is size_t on an LP64 host");
static_assert(sizeof(bam_api::ReadQuality) == sizeof(std::uint32_t), "ReadQuality is uint32 (read.hpp)");

QuasiMcpHipSolver::~QuasiMcpHipSolver() {
    if (ctx_ != nullptr) qmcp_hip_destroy(ctx_);
}

void QuasiMcpHipSolver::set_device(int device) { device_ = device; }

// ------------------------------------------------------------------------------------------ the shared steps

// The reference's GPU solver has no error channel: any device failure ends in
// std::terminate() (libs/qmcp-solver/include/qmcp-solver/cuda_helpers.cuh:13-22).
// The C ABI returns codes; the adapter restores the reference behaviour.
void QuasiMcpHipSolver::die(const char* what, int rc) const {
    std::fprintf(stderr, "[ERROR] %s: %s failed (%d): %s\n", name(), what, rc, qmcp_hip_last_error());
    std::terminate();
}

void QuasiMcpHipSolver::ok_or_die(const char* what, int rc) const {
    if (rc != QMCP_OK) die(what, rc);
}

void QuasiMcpHipSolver::ok_or_throw(const char* what, int rc) const {
    if (rc == QMCP_EINVAL || rc == QMCP_ERANGE) throw std::invalid_argument(qmcp_hip_last_error());
    ok_or_die(what, rc);
}

qmcp_hip_ctx* QuasiMcpHipSolver::context() {
    if (ctx_ == nullptr) ok_or_die("qmcp_hip_create", qmcp_hip_create(device_, &ctx_));
    return ctx_;
}

QuasiMcpHipSolver::Columns QuasiMcpHipSolver::narrowed(const bam_api::SOAPairedReads& reads) const {
    const std::size_t n = reads.start_inds.size();
    Columns c;
    c.starts.resize(n);
    c.ends.resize(n);
    const Narrowed r = narrow_columns(reads.start_inds.data(), reads.end_inds.data(),
                                      reads.has_contig_ids() ? reads.contig_ids.data() : nullptr, n, c.starts.data(),
                                      c.ends.data());
    if (r.bad != n) die("narrowing a coordinate", QMCP_ERANGE);
    c.placed = r.placed;
    return c;
}

bool QuasiMcpHipSolver::one_contig_id_each(const bam_api::SOAPairedReads& reads) {
    return reads.has_contig_ids() && reads.contig_ids.size() == reads.start_inds.size();
}

void QuasiMcpHipSolver::need_per_reference(bool configured, const bam_api::SOAPairedReads& reads, const char* message) {
    if (!configured || !one_contig_id_each(reads)) throw std::invalid_argument(message);
}

void QuasiMcpHipSolver::check_regions(const std::vector<std::uint32_t>& offsets, const std::vector<std::uint32_t>& starts,
                                      const std::vector<std::uint32_t>& ends, const std::vector<std::uint32_t>& caps,
                                      std::size_t n_refs) {
    if (offsets.size() != n_refs + 1) throw std::invalid_argument("cap regions of other references");
    if (starts.size() < offsets.back() || ends.size() < offsets.back() || caps.size() < offsets.back())
        throw std::invalid_argument("cap region arrays are shorter than their offsets say");
}

// ascending ReadIndex, as obtain_sequence produces (quasi_mcp_cpu_max_flow_solver.cpp:93-97): expanded from
// the keep mask on the device (popcounts, scan, scatter) and copied out -- 5 % of the reads at cfg4's depth
std::unique_ptr<Solution> QuasiMcpHipSolver::expand(std::uint64_t n, std::uint64_t upper,
                                                    std::chrono::steady_clock::time_point t0) {
    const auto t1 = std::chrono::steady_clock::now();
    auto kept = std::make_unique<Solution>();
    kept->resize(upper);
    std::uint64_t n_out = 0;
    ok_or_die("qmcp_hip_kept_indices_host",
              qmcp_hip_kept_indices_host(ctx_, n, reinterpret_cast<std::uint64_t*>(kept->data()), upper, &n_out));
    kept->resize(n_out);
    const auto t2 = std::chrono::steady_clock::now();
    ms_expand_ = std::chrono::duration<float, std::milli>(t2 - t1).count();
    ms_solve_call_ = std::chrono::duration<float, std::milli>(t2 - t0).count();
    return kept;
}

std::unique_ptr<Solution> QuasiMcpHipSolver::expand_kept(std::uint64_t n, std::chrono::steady_clock::time_point t0) {
    return expand(n, complete_pairs_ ? std::min<std::uint64_t>(n, 2 * stats_.n_kept) : stats_.n_kept, t0);
}

std::unique_ptr<Solution> QuasiMcpHipSolver::finish(std::vector<std::uint64_t>& mask, std::uint64_t n,
                                                    std::chrono::steady_clock::time_point t0) {
    breakdown_ = qmcp_hip_host_breakdown{};
    if (complete_pairs_)  // (leaves the completed mask in the context)
        ok_or_die("qmcp_hip_complete_pairs_host", qmcp_hip_complete_pairs_host(ctx_, mask.data(), n));
    return expand_kept(n, t0);
}

namespace {

std::vector<std::uint64_t> empty_mask(std::size_t n) { return std::vector<std::uint64_t>((n + 63) / 64, 0); }

std::uint32_t n_contigs(const bam_api::SOAPairedReads& reads) { return (std::uint32_t)reads.contig_lengths.size(); }

float ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

// ------------------------------------------------------------------------------------------ solve() and its routes

std::unique_ptr<Solution> QuasiMcpHipSolver::solve(std::uint32_t required_cover,
                                                   bam_api::BamApi& bam_api) {
    // The reference solvers deep-copy the whole container (quasi_mcp_cpu_max_flow_solver.cpp:13,
    // quasi_mcp_cuda_max_flow_solver.cu:321); only two columns are needed, narrowed to the
    // uint32 coordinates the CUDA solver already uses (quasi_mcp_cuda_max_flow_solver.hpp:19).
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    constexpr std::size_t kMax = std::numeric_limits<std::uint32_t>::max();
    if (reads.ref_genome_length > kMax && !reads.has_contig_ids()) die("narrowing ref_genome_length", QMCP_ERANGE);
    context();

    if (reads.has_strata()) return solve_stratified(required_cover, reads, bam_api.stratify_by(), t0);
    if (bam_api.has_targets()) return solve_targets(required_cover, reads, bam_api.get_targets(), false, t0);
    if (reads.has_contig_ids()) return solve_by_contig(required_cover, reads, t0);

    // the 64-bit columns go to the library as they are: it narrows them chunk by chunk on several
    // threads straight into pinned staging, each chunk's copy to the device issued as it is ready
    const std::uint64_t offsets[2] = {0, n};
    const std::uint32_t length = static_cast<std::uint32_t>(reads.ref_genome_length);
    // complete_pairs needs the mask on the host side of the ABI; otherwise it stays on the device and only
    // the Solution comes back
    std::vector<std::uint64_t> mask;
    if (complete_pairs_) mask = empty_mask(n);
    ok_or_die("qmcp_hip_solve_host64",
              qmcp_hip_solve_host64(ctx_, reinterpret_cast<const std::uint64_t*>(reads.start_inds.data()),
                                    reinterpret_cast<const std::uint64_t*>(reads.end_inds.data()), n, offsets, &length, 1,
                                    required_cover, complete_pairs_ ? mask.data() : nullptr, &stats_, &breakdown_));
    // (the library's breakdown stands: not finish())
    if (complete_pairs_) ok_or_die("qmcp_hip_complete_pairs_host", qmcp_hip_complete_pairs_host(ctx_, mask.data(), n));
    return expand_kept(n, t0);
}

// Reads of several references (BamApiConfig::per_reference): one coverage problem per reference, through
// qmcp_hip_solve_by_contig_host -- the reads stay in pairing order, the library groups them by contig on the device.
// Unplaced reads (QMCP_NO_CONTIG) are never kept; their coordinates do not matter and go over as 0.
std::unique_ptr<Solution> QuasiMcpHipSolver::solve_by_contig(std::uint32_t required_cover,
                                                             const bam_api::SOAPairedReads& reads,
                                                             std::chrono::steady_clock::time_point t0) {
    const std::size_t n = reads.start_inds.size();
    if (!one_contig_id_each(reads)) die("per-reference reads without one contig id each", QMCP_EINVAL);
    const Columns c = narrowed(reads);
    std::vector<std::uint64_t> mask = empty_mask(n);
    ok_or_die("qmcp_hip_solve_by_contig_host",
              qmcp_hip_solve_by_contig_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), n,
                                            reads.contig_lengths.data(), n_contigs(reads), required_cover, mask.data(),
                                            &stats_));
    return finish(mask, n, t0);
}

// STRAND: the two strands share M, the forward strand taking the odd one; every other stratification brings every
// stratum to M ("every sample to M x")
std::vector<std::uint32_t> QuasiMcpHipSolver::stratum_caps(std::uint32_t required_cover, bam_api::Stratify by,
                                                           std::size_t n_strata) {
    std::vector<std::uint32_t> caps(n_strata, required_cover);
    if (by == bam_api::Stratify::STRAND && n_strata == 2) {
        caps[0] = required_cover - required_cover / 2;
        caps[1] = required_cover / 2;
    }
    return caps;
}

// Per-reference reads with a stratum each (BamApiConfig::stratify_by): one cap per stratum, through
// qmcp_hip_solve_stratified_host; otherwise as solve_by_contig.
std::unique_ptr<Solution> QuasiMcpHipSolver::solve_stratified(std::uint32_t required_cover,
                                                              const bam_api::SOAPairedReads& reads, bam_api::Stratify by,
                                                              std::chrono::steady_clock::time_point t0) {
    const std::size_t n = reads.start_inds.size();
    if (!one_contig_id_each(reads)) die("strata without one contig id per read", QMCP_EINVAL);
    if (reads.strata.size() != n) die("stratified reads without one stratum each", QMCP_EINVAL);
    const Columns c = narrowed(reads);
    stratum_caps_ = stratum_caps(required_cover, by, reads.stratum_names.size());
    stratum_rows_.assign(stratum_caps_.size(), qmcp_hip_stratum_row{});
    std::vector<std::uint64_t> mask = empty_mask(n);
    ok_or_die("qmcp_hip_solve_stratified_host",
              qmcp_hip_solve_stratified_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(),
                                             reads.strata.data(), n, reads.contig_lengths.data(), n_contigs(reads),
                                             stratum_caps_.data(), (std::uint32_t)stratum_caps_.size(), mask.data(),
                                             stratum_rows_.data(), &stats_));
    return finish(mask, n, t0);
}

// Per-reference reads with target regions (BamApiConfig::targets_filepath): coverage capped inside the regions only,
// through qmcp_hip_solve_targets_host; otherwise as solve_by_contig.
std::unique_ptr<Solution> QuasiMcpHipSolver::solve_targets(std::uint32_t required_cover,
                                                           const bam_api::SOAPairedReads& reads,
                                                           const bam_api::TargetRegions& targets, bool with_qualities,
                                                           std::chrono::steady_clock::time_point t0) {
    const std::size_t n = reads.start_inds.size();
    if (!one_contig_id_each(reads)) die("target regions without one contig id per read", QMCP_EINVAL);
    if (with_qualities && reads.qualities.size() != n) die("reads without one quality each", QMCP_EINVAL);
    if (targets.offsets.size() != reads.contig_lengths.size() + 1) die("target regions of other references", QMCP_EINVAL);
    const Columns c = narrowed(reads);
    std::vector<std::uint64_t> mask = empty_mask(n);
    ok_or_die("qmcp_hip_solve_targets_host",
              qmcp_hip_solve_targets_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(),
                                          with_qualities ? reads.qualities.data() : nullptr, n,
                                          reads.contig_lengths.data(), n_contigs(reads), targets.offsets.data(),
                                          targets.starts.data(), targets.ends.data(), targets.padding, required_cover,
                                          targets.keep_off_target ? QMCP_TARGETS_KEEP_OFF_TARGET : 0u, mask.data(),
                                          &stats_, &tstats_));
    if (targets.keep_off_target) stats_.n_kept += tstats_.reads_off_target;  // (expand_kept sizes the Solution by it)
    return finish(mask, n, t0);
}

// ------------------------------------------------------------------------------------------ the entries by mode

std::unique_ptr<Solution> QuasiMcpHipSolver::solve_dedup(std::uint32_t required_cover, bam_api::BamApi& bam_api,
                                                         std::uint32_t hist_bins) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    need_per_reference(bam_api.dedup() && reads.strata.size() == n, reads,
                       "duplicate-aware downsampling needs a BamApi built with BamApiConfig::dedup");
    if (reads.qualities.size() != n) throw std::invalid_argument("reads without one quality each");
    context();
    const Columns c = narrowed(reads);
    dedup_hist_.assign(hist_bins, 0);
    std::vector<std::uint64_t> mask = empty_mask(n);
    ok_or_die("qmcp_hip_solve_dedup_host",
              qmcp_hip_solve_dedup_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), reads.strata.data(),
                                        reads.qualities.data(), n, reads.contig_lengths.data(), n_contigs(reads),
                                        required_cover, QMCP_DEDUP_PAIRS | QMCP_DEDUP_COMPLETE_PAIRS, mask.data(), nullptr,
                                        hist_bins ? dedup_hist_.data() : nullptr, hist_bins, &stats_, &dstats_));
    breakdown_ = qmcp_hip_host_breakdown{};
    // the context holds the completed mask: at most two reads per read the solve kept
    return expand(n, std::min<std::uint64_t>(n, 2 * stats_.n_kept), t0);
}

std::unique_ptr<Solution> QuasiMcpHipSolver::solve_start_cap(std::uint32_t required_cover, bam_api::BamApi& bam_api,
                                                             std::uint32_t hist_bins) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    const bool by_strand = bam_api.start_cap_by_strand();
    need_per_reference(bam_api.start_cap() && (!by_strand || reads.strata.size() == n), reads,
                       "a start cap needs a BamApi built with BamApiConfig::start_cap");
    if (reads.qualities.size() != n) throw std::invalid_argument("reads without one quality each");
    context();
    const Columns c = narrowed(reads);
    start_cap_hist_.assign(hist_bins, 0);
    std::vector<std::uint64_t> mask = empty_mask(n);
    ok_or_die("qmcp_hip_solve_start_cap_host",
              qmcp_hip_solve_start_cap_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(),
                                            by_strand ? reads.strata.data() : nullptr, reads.qualities.data(), n,
                                            reads.contig_lengths.data(), n_contigs(reads), required_cover,
                                            bam_api.start_cap(), QMCP_START_CAP_SHORTFALL, mask.data(), nullptr,
                                            hist_bins ? start_cap_hist_.data() : nullptr, hist_bins, &stats_, &scstats_));
    return finish(mask, n, t0);
}

std::unique_ptr<Solution> QuasiMcpHipSolver::solve_amplicons(std::uint32_t required_cover, bam_api::BamApi& bam_api) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    const bam_api::ReferenceAmpliconSet& set = bam_api.reference_amplicons();
    need_per_reference(bam_api.primer_clip() || bam_api.per_amplicon() || !bam_api.amplicon_report_filepath().empty(), reads,
                       "amplicon-aware downsampling needs a BamApi built with BamApiConfig::primer_clip, per_amplicon or "
                       "amplicon_report_filepath");
    if (set.n_references() != reads.contig_lengths.size()) throw std::invalid_argument("amplicons of other references");
    if (reads.qualities.size() != n || reads.seq_lengths.size() != n)
        throw std::invalid_argument("reads without one quality and one length each");
    context();
    const Columns c = narrowed(reads);
    const auto narrow = [](const std::vector<bam_api::Index>& v) {
        std::vector<std::uint32_t> out(v.size());
        for (std::size_t k = 0; k < v.size(); ++k) {
            if (v[k] > std::numeric_limits<std::uint32_t>::max()) throw std::invalid_argument("an amplicon beyond 2^32");
            out[k] = (std::uint32_t)v[k];
        }
        return out;
    };
    const std::vector<std::uint32_t> a0 = narrow(set.starts), a1 = narrow(set.ends);
    std::vector<std::uint32_t> i0, i1;
    if (bam_api.primer_clip()) {
        i0 = narrow(set.insert_starts);
        i1 = narrow(set.insert_ends);
    }
    amplicon_labels_.assign(n / 2, QMCP_NO_AMPLICON);
    amplicon_rows_.assign(a0.size(), qmcp_hip_depth_row{});
    std::vector<std::uint64_t> mask = empty_mask(n);
    // (the ingest applied the length / MAPQ filters and the FILTER already: the entry sees the pairs that passed)
    ok_or_throw("qmcp_hip_solve_amplicons_host",
                qmcp_hip_solve_amplicons_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), nullptr, nullptr,
                                              n, reads.contig_lengths.data(), n_contigs(reads), set.offsets.data(),
                                              a0.data(), a1.data(), bam_api.primer_clip() ? i0.data() : nullptr,
                                              bam_api.primer_clip() ? i1.data() : nullptr, 0, 0, required_cover,
                                              QMCP_AMPLICONS_COMPLETE_PAIRS |
                                                  (bam_api.per_amplicon() ? QMCP_AMPLICONS_PER_AMPLICON : 0u),
                                              mask.data(), amplicon_labels_.data(), amplicon_rows_.data(), &stats_,
                                              &astats_));
    breakdown_ = qmcp_hip_host_breakdown{};
    // the context holds the completed mask: at most two reads per read the solve kept
    return expand(n, std::min<std::uint64_t>(n, 2 * stats_.n_kept), t0);
}

std::unique_ptr<Solution> QuasiMcpHipSolver::solve_profile(std::uint32_t required_cover, bam_api::BamApi& bam_api,
                                                           const std::vector<std::uint32_t>& offsets,
                                                           const std::vector<std::uint32_t>& region_starts,
                                                           const std::vector<std::uint32_t>& region_ends,
                                                           const std::vector<std::uint32_t>& caps) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    need_per_reference(true, reads, "a coverage profile needs per_reference reads (one contig id per read)");
    check_regions(offsets, region_starts, region_ends, caps, reads.contig_lengths.size());
    context();
    const Columns c = narrowed(reads);
    std::vector<std::uint64_t> mask = empty_mask(n);
    ok_or_throw("qmcp_hip_solve_profile_host",
                qmcp_hip_solve_profile_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), n,
                                            reads.contig_lengths.data(), n_contigs(reads), offsets.data(),
                                            region_starts.data(), region_ends.data(), caps.data(), required_cover, 0u,
                                            mask.data(), &stats_, &pstats_));
    return finish(mask, n, t0);
}

std::unique_ptr<Solution> QuasiMcpHipSolver::solve_proportional(std::uint32_t required_cover, bam_api::BamApi& bam_api) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    need_per_reference(bam_api.proportion().has_value(), reads,
                       "proportional downsampling needs a BamApi built with BamApiConfig::proportion");
    context();
    const Columns c = narrowed(reads);
    const bam_api::BamApiConfig::Proportion& f = *bam_api.proportion();
    std::vector<std::uint64_t> mask = empty_mask(n);
    ok_or_throw("qmcp_hip_solve_proportional_host",
                qmcp_hip_solve_proportional_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), n,
                                                 reads.contig_lengths.data(), n_contigs(reads), f.num, f.den, f.floor,
                                                 required_cover, 0u, mask.data(), &stats_, &ppstats_));
    return finish(mask, n, t0);
}

std::unique_ptr<Solution> QuasiMcpHipSolver::solve_tiers(std::uint32_t required_cover, bam_api::BamApi& bam_api) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    const std::vector<std::uint32_t>& bands = bam_api.mapq_tiers();
    need_per_reference(!bands.empty(), reads, "tiered downsampling needs a BamApi built with BamApiConfig::mapq_tiers");
    context();
    const Columns c = narrowed(reads);
    std::vector<std::uint32_t> tiers(std::max<std::size_t>(n, 1), QMCP_NO_TIER);  // (never NULL, also without reads)
    for (std::size_t i = 0; i < n; ++i)
        for (std::size_t t = 0; t < bands.size(); ++t)
            if (reads.qualities[i] >= bands[t]) {
                tiers[i] = (std::uint32_t)t;
                break;
            }
    tier_rows_.assign(bands.size(), qmcp_hip_tier_row{});
    std::vector<std::uint64_t> mask = empty_mask(n);
    ok_or_throw("qmcp_hip_solve_tiers_host",
                qmcp_hip_solve_tiers_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), tiers.data(), n,
                                          reads.contig_lengths.data(), n_contigs(reads), required_cover,
                                          (std::uint32_t)bands.size(), mask.data(), tier_rows_.data(), &stats_, &trstats_));
    // (stats_ are tier 0's solver calls: the mask holds the kept reads of every tier)
    std::uint64_t kept = 0;
    for (const qmcp_hip_tier_row& row : tier_rows_) kept += row.n_kept;
    breakdown_ = qmcp_hip_host_breakdown{};
    if (complete_pairs_) ok_or_die("qmcp_hip_complete_pairs_host", qmcp_hip_complete_pairs_host(ctx_, mask.data(), n));
    return expand(n, complete_pairs_ ? std::min<std::uint64_t>(n, 2 * kept) : kept, t0);
}

std::unique_ptr<Solution> QuasiMcpHipSolver::solve_pairs(std::uint32_t required_cover, bam_api::BamApi& bam_api) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    need_per_reference(bam_api.pair_aware(), reads,
                       "pair-aware downsampling needs a BamApi built with BamApiConfig::pair_aware");
    context();
    const Columns c = narrowed(reads);
    const std::vector<std::uint32_t>& stages = bam_api.pair_stages();
    std::vector<std::uint64_t> mask = empty_mask(n);
    ok_or_throw("qmcp_hip_solve_pairs_host",
                qmcp_hip_solve_pairs_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), n,
                                          reads.contig_lengths.data(), n_contigs(reads), required_cover,
                                          stages.empty() ? nullptr : stages.data(), (std::uint32_t)stages.size(),
                                          mask.data(), &stats_, &prstats_));
    breakdown_ = qmcp_hip_host_breakdown{};
    // the context holds the last stage's completed mask
    return expand(n, prstats_.n_kept[prstats_.n_stages - 1], t0);
}

std::vector<std::uint8_t> QuasiMcpHipSolver::solve_replicates(std::uint32_t required_cover, bam_api::BamApi& bam_api) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    need_per_reference(bam_api.replicates().has_value(), reads,
                       "disjoint replicates need a BamApi built with BamApiConfig::replicates");
    std::vector<std::uint32_t> coverages{required_cover};
    coverages.insert(coverages.end(), bam_api.replicates()->begin(), bam_api.replicates()->end());
    context();
    const Columns c = narrowed(reads);
    std::vector<std::uint8_t> labels(n, 0);
    ok_or_throw("qmcp_hip_solve_replicates_host",
                qmcp_hip_solve_replicates_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), n,
                                               reads.contig_lengths.data(), n_contigs(reads), coverages.data(),
                                               (std::uint32_t)coverages.size(),
                                               QMCP_REPLICATES_WHOLE_PAIRS | QMCP_REPLICATES_SHORTFALL, labels.data(),
                                               &stats_, nullptr, &rpstats_));
    breakdown_ = qmcp_hip_host_breakdown{};
    ms_solve_call_ = ms_since(t0);
    return labels;
}

std::unique_ptr<Solution> QuasiMcpHipSolver::solve_ceiling(std::uint32_t required_cover, bam_api::BamApi& bam_api,
                                                           const std::vector<std::uint32_t>& offsets,
                                                           const std::vector<std::uint32_t>& region_starts,
                                                           const std::vector<std::uint32_t>& region_ends,
                                                           const std::vector<std::uint32_t>& caps) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    need_per_reference(bam_api.ceiling(), reads, "ceiling downsampling needs a BamApi built with BamApiConfig::ceiling");
    const bool with_regions = !offsets.empty();
    if (with_regions) check_regions(offsets, region_starts, region_ends, caps, reads.contig_lengths.size());
    context();
    const Columns c = narrowed(reads);
    std::vector<std::uint64_t> mask = empty_mask(n);
    ok_or_throw("qmcp_hip_solve_ceiling_host",
                qmcp_hip_solve_ceiling_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), n,
                                            reads.contig_lengths.data(), n_contigs(reads),
                                            with_regions ? offsets.data() : nullptr, region_starts.data(),
                                            region_ends.data(), caps.data(), required_cover, QMCP_CEILING_WHOLE_PAIRS,
                                            mask.data(), &stats_, &clstats_));
    breakdown_ = qmcp_hip_host_breakdown{};
    // the context holds the final mask
    return expand(n, clstats_.reads_placed - clstats_.reads_dropped, t0);
}

std::unique_ptr<Solution> QuasiMcpHipSolver::solve_thresholds(bam_api::BamApi& bam_api) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    need_per_reference(bam_api.thresholds(), reads,
                       "coverage thresholds need a BamApi built with BamApiConfig::thresholds_hi");
    context();
    const Columns c = narrowed(reads);
    const std::uint32_t lo = bam_api.thresholds_lo(), hi = bam_api.thresholds_hi();
    thresholds_.assign(n, (std::uint16_t)QMCP_THRESHOLD_NEVER);
    threshold_counts_.assign(hi >= lo ? (std::size_t)(hi - lo) + 1 : 0, 0);
    ok_or_throw("qmcp_hip_solve_thresholds_host",
                qmcp_hip_solve_thresholds_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), n,
                                               reads.contig_lengths.data(), n_contigs(reads), lo, hi,
                                               QMCP_THRESHOLDS_WHOLE_PAIRS, thresholds_.data(), threshold_counts_.data(),
                                               (std::uint32_t)threshold_counts_.size(), &stats_, &thstats_));
    threshold_counts_.resize(thstats_.count_entries);
    breakdown_ = qmcp_hip_host_breakdown{};
    auto kept = std::make_unique<Solution>();
    kept->reserve(thstats_.n_kept);
    for (std::size_t i = 0; i < n; ++i)
        if (thresholds_[i] != QMCP_THRESHOLD_NEVER) kept->push_back(i);
    ms_solve_call_ = ms_since(t0);
    return kept;
}

std::unique_ptr<Solution> QuasiMcpHipSolver::solve_budget(std::uint32_t required_cover, bam_api::BamApi& bam_api) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    need_per_reference(bam_api.budget(), reads,
                       "budget downsampling needs a BamApi built with BamApiConfig::budget_reads or budget_fraction");
    context();
    const Columns c = narrowed(reads);
    std::vector<std::uint64_t> mask = empty_mask(n);
    budget_curve_.assign(QMCP_BUDGET_CURVE_MAX + 1u, 0);
    ok_or_throw("qmcp_hip_solve_budget_host",
                qmcp_hip_solve_budget_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), n,
                                           reads.contig_lengths.data(), n_contigs(reads), required_cover,
                                           bam_api.budget_for(c.placed), QMCP_BUDGET_WHOLE_PAIRS, budget_curve_.data(),
                                           (std::uint32_t)budget_curve_.size(), mask.data(), &stats_, &bgstats_));
    budget_curve_.resize(bgstats_.curve_entries);
    breakdown_ = qmcp_hip_host_breakdown{};
    // the context holds the final mask
    return expand(n, bgstats_.n_kept, t0);
}

std::unique_ptr<Solution> QuasiMcpHipSolver::solve_mean_depth(std::uint32_t required_cover, bam_api::BamApi& bam_api) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = reads.start_inds.size();
    need_per_reference(bam_api.mean_depth(), reads,
                       "mean-depth downsampling needs a BamApi built with BamApiConfig::mean_depth or budget_bases");
    context();
    const Columns c = narrowed(reads);
    const bam_api::TargetRegions* regions = bam_api.has_mean_depth_regions() ? &bam_api.mean_depth_regions() : nullptr;
    if (regions && regions->offsets.size() != reads.contig_lengths.size() + 1)
        throw std::invalid_argument("the mean-depth regions do not match the file's references");
    const std::uint64_t budget = bam_api.base_budget_for(bam_api.mean_depth_positions(reads.contig_lengths));
    std::vector<std::uint64_t> mask = empty_mask(n);
    mean_depth_curve_.assign(QMCP_BUDGET_CURVE_MAX + 1u, 0);
    ok_or_throw("qmcp_hip_solve_mean_depth_host",
                qmcp_hip_solve_mean_depth_host(
                    ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), n, reads.contig_lengths.data(),
                    n_contigs(reads), required_cover, budget, regions ? regions->offsets.data() : nullptr,
                    regions ? regions->starts.data() : nullptr, regions ? regions->ends.data() : nullptr,
                    QMCP_MEAN_DEPTH_WHOLE_PAIRS, mean_depth_curve_.data(), (std::uint32_t)mean_depth_curve_.size(),
                    mask.data(), &stats_, &mdstats_));
    mean_depth_curve_.resize(mdstats_.curve_entries);
    breakdown_ = qmcp_hip_host_breakdown{};
    // the context holds the final mask
    return expand(n, mdstats_.n_kept, t0);
}

// a record is written iff one of its segments is kept; its segments are consecutive, in file order
static std::vector<bam_api::BAMReadId> records_of_kept_segments(const bam_api::TemplateSegments& seg,
                                                                const std::vector<std::uint64_t>& mask) {
    std::vector<bam_api::BAMReadId> records;
    for (std::size_t i = 0; i < seg.starts.size(); ++i)
        if (((mask[i >> 6] >> (i & 63)) & 1ull) && (records.empty() || records.back() != seg.segment_records[i]))
            records.push_back(seg.segment_records[i]);
    return records;
}

std::vector<bam_api::BAMReadId> QuasiMcpHipSolver::solve_templates(std::uint32_t required_cover, bam_api::BamApi& bam_api) {
    if (!bam_api.template_aware())
        throw std::invalid_argument("template-aware downsampling needs a BamApi built with BamApiConfig::template_aware");
    const bam_api::TemplateSegments& seg = bam_api.get_template_segments();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = seg.starts.size();
    context();
    const std::vector<std::uint32_t>& stages = bam_api.template_stages();
    std::vector<std::uint64_t> mask = empty_mask(n);
    frstats_ = qmcp_hip_fragment_stats{};
    const bool fragments = bam_api.fragment_depth();
    const int rc = fragments
        ? qmcp_hip_solve_fragments_host(ctx_, seg.starts.data(), seg.ends.data(), seg.contig_ids.data(),
                                        seg.template_ids.data(), n, seg.n_templates, seg.contig_lengths.data(),
                                        (std::uint32_t)seg.contig_lengths.size(), required_cover,
                                        stages.empty() ? nullptr : stages.data(), (std::uint32_t)stages.size(), mask.data(),
                                        &stats_, &tpstats_, &frstats_)
        : qmcp_hip_solve_templates_host(ctx_, seg.starts.data(), seg.ends.data(), seg.contig_ids.data(),
                                        seg.template_ids.data(), n, seg.n_templates, seg.contig_lengths.data(),
                                        (std::uint32_t)seg.contig_lengths.size(), required_cover,
                                        stages.empty() ? nullptr : stages.data(), (std::uint32_t)stages.size(), mask.data(),
                                        &stats_, &tpstats_);
    ok_or_throw(fragments ? "qmcp_hip_solve_fragments_host" : "qmcp_hip_solve_templates_host", rc);
    breakdown_ = qmcp_hip_host_breakdown{};
    std::vector<bam_api::BAMReadId> records = records_of_kept_segments(seg, mask);
    ms_solve_call_ = ms_since(t0);
    return records;
}

std::vector<bam_api::BAMReadId> QuasiMcpHipSolver::solve_templates_profile(std::uint32_t required_cover,
                                                                           bam_api::BamApi& bam_api,
                                                                           const std::vector<std::uint32_t>& offsets,
                                                                           const std::vector<std::uint32_t>& region_starts,
                                                                           const std::vector<std::uint32_t>& region_ends,
                                                                           const std::vector<std::uint32_t>& caps,
                                                                           std::uint32_t default_cap) {
    if (!bam_api.template_aware())
        throw std::invalid_argument("template-aware downsampling needs a BamApi built with BamApiConfig::template_aware");
    const bam_api::TemplateSegments& seg = bam_api.get_template_segments();
    const auto t0 = std::chrono::steady_clock::now();
    const std::size_t n = seg.starts.size();
    check_regions(offsets, region_starts, region_ends, caps, seg.contig_lengths.size());
    context();
    const std::vector<std::uint32_t>& stages = bam_api.template_stages();
    std::vector<std::uint64_t> mask = empty_mask(n);
    // fragment depth: the clip first, the profile entry on its columns (two calls)
    frstats_ = qmcp_hip_fragment_stats{};
    std::vector<std::uint32_t> clipped_starts, clipped_ids;
    if (bam_api.fragment_depth()) {
        clipped_starts.resize(n);
        clipped_ids.resize(n);
        ok_or_throw("qmcp_hip_clip_templates_host",
                    qmcp_hip_clip_templates_host(ctx_, seg.starts.data(), seg.ends.data(), seg.contig_ids.data(),
                                                 seg.template_ids.data(), n, seg.n_templates, seg.contig_lengths.data(),
                                                 (std::uint32_t)seg.contig_lengths.size(), clipped_starts.data(),
                                                 clipped_ids.data(), &frstats_));
    }
    const std::uint32_t* starts = bam_api.fragment_depth() ? clipped_starts.data() : seg.starts.data();
    const std::uint32_t* contig_ids = bam_api.fragment_depth() ? clipped_ids.data() : seg.contig_ids.data();
    ok_or_throw("qmcp_hip_solve_templates_profile_host",
                qmcp_hip_solve_templates_profile_host(
                    ctx_, starts, seg.ends.data(), contig_ids, seg.template_ids.data(), n, seg.n_templates,
                    seg.contig_lengths.data(), (std::uint32_t)seg.contig_lengths.size(), offsets.data(),
                    region_starts.data(), region_ends.data(), caps.data(), default_cap, 0u, required_cover,
                    stages.empty() ? nullptr : stages.data(), (std::uint32_t)stages.size(), mask.data(), &stats_,
                    &tpstats_, &tqstats_));
    breakdown_ = qmcp_hip_host_breakdown{};
    std::vector<bam_api::BAMReadId> records = records_of_kept_segments(seg, mask);
    ms_solve_call_ = ms_since(t0);
    return records;
}

std::vector<std::unique_ptr<Solution>> QuasiMcpHipSolver::solve_ladder(std::uint32_t required_cover,
                                                                       bam_api::BamApi& bam_api,
                                                                       const std::vector<std::uint32_t>& levels) {
    std::vector<std::uint32_t> coverages{required_cover};
    coverages.insert(coverages.end(), levels.begin(), levels.end());
    if (coverages.size() > QMCP_LADDER_MAX_LEVELS)
        throw std::invalid_argument("a coverage ladder has at most " + std::to_string(QMCP_LADDER_MAX_LEVELS - 1) +
                                    " levels below max_coverage");
    for (std::size_t j = 1; j < coverages.size(); ++j)
        if (coverages[j] >= coverages[j - 1])
            throw std::invalid_argument(j == 1 ? "the levels of a coverage ladder must be strictly below max_coverage"
                                               : "the levels of a coverage ladder must be strictly decreasing");
    if (coverages.back() == 0) throw std::invalid_argument("a coverage ladder ends at a coverage >= 1");
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const std::size_t n = reads.start_inds.size();
    need_per_reference(true, reads, "a coverage ladder needs per_reference reads (one contig id each)");
    context();
    const Columns c = narrowed(reads);
    std::vector<std::uint8_t> bytes(n, 0);
    ok_or_die("qmcp_hip_solve_ladder_host",
              qmcp_hip_solve_ladder_host(ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), n,
                                         reads.contig_lengths.data(), n_contigs(reads), coverages.data(),
                                         (std::uint32_t)coverages.size(), bytes.data(), &stats_, &lstats_));
    breakdown_ = qmcp_hip_host_breakdown{};
    std::vector<std::unique_ptr<Solution>> out;
    for (std::size_t j = 0; j < coverages.size(); ++j) {
        auto kept = std::make_unique<Solution>();
        kept->reserve(lstats_.n_kept[j]);
        for (std::size_t i = 0; i < n; ++i)
            if (bytes[i] > j) kept->push_back(i);
        out.push_back(std::move(kept));
    }
    return out;
}

// ------------------------------------------------------------------------------------------ depth before and after

void QuasiMcpHipSolver::depth_report(std::uint32_t required_cover, bam_api::BamApi& bam_api,
                                     const std::vector<bam_api::ReadIndex>& kept, std::uint32_t n_bins, DepthReport& out) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const std::size_t n = reads.start_inds.size();
    if (!one_contig_id_each(reads)) die("a depth report without one contig id per read", QMCP_EINVAL);
    context();
    const Columns c = narrowed(reads);
    const std::vector<std::uint64_t> mask = keep_mask_of(kept, n);
    const bool regions = bam_api.has_targets();
    const bam_api::TargetRegions& t = bam_api.get_targets();
    out = DepthReport();
    out.contig_rows.resize(n_contigs(reads));
    out.region_rows.resize(regions ? t.starts.size() : 0);
    out.hist_in.assign(n_bins, 0);
    out.hist_kept.assign(n_bins, 0);
    std::uint64_t n_rows = 0;
    ok_or_die("qmcp_hip_depth_report_host",
              qmcp_hip_depth_report_host(
                  ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), n, reads.contig_lengths.data(),
                  n_contigs(reads), mask.data(), required_cover, regions ? t.offsets.data() : nullptr,
                  regions ? t.starts.data() : nullptr, regions ? t.ends.data() : nullptr, regions ? t.padding : 0u, n_bins,
                  out.contig_rows.data(), out.region_rows.data(), out.region_rows.size(), &n_rows,
                  n_bins ? out.hist_in.data() : nullptr, n_bins ? out.hist_kept.data() : nullptr, &out.stats));
    out.region_rows.resize(n_rows);
}

void QuasiMcpHipSolver::depth_track(std::uint32_t required_cover, bam_api::BamApi& bam_api,
                                    const std::vector<bam_api::ReadIndex>& kept, std::uint32_t flags,
                                    std::uint32_t depth_cap, DepthTrack& out) {
    const bam_api::SOAPairedReads& reads = bam_api.get_paired_reads_soa();
    const std::size_t n = reads.start_inds.size();
    if (!one_contig_id_each(reads)) die("a depth track without one contig id per read", QMCP_EINVAL);
    context();
    const Columns c = narrowed(reads);
    const std::vector<std::uint64_t> mask = keep_mask_of(kept, n);
    const bool regions = bam_api.has_targets();
    const bam_api::TargetRegions& t = bam_api.get_targets();
    out = DepthTrack();
    std::uint64_t n_runs = 0;
    for (int pass = 0; pass < 2; ++pass) {  // the count, then the records at that size
        ok_or_die("qmcp_hip_depth_track_host",
                  qmcp_hip_depth_track_host(
                      ctx_, c.starts.data(), c.ends.data(), reads.contig_ids.data(), n, reads.contig_lengths.data(),
                      n_contigs(reads), mask.data(), required_cover, regions ? t.offsets.data() : nullptr,
                      regions ? t.starts.data() : nullptr, regions ? t.ends.data() : nullptr, regions ? t.padding : 0u,
                      flags, depth_cap, pass ? out.runs.data() : nullptr, out.runs.size(), &n_runs, &out.stats));
        if (pass == 0) {
            if (n_runs == 0) break;
            out.runs.resize(n_runs);
        }
    }
}

bool write_depth_track_bedgraph(const std::filesystem::path& path, const DepthTrack& track,
                                const std::vector<std::string>& reference_names, const std::string& channel) {
    const bool both = channel == "both", in = channel == "in";
    if (!both && !in && channel != "kept") return false;
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (f == nullptr) return false;
    if (both) std::fputs("#chrom\tstart\tend\tdepth_in\tdepth_kept\n", f);
    const std::vector<qmcp_hip_track_run>& v = track.runs;
    for (std::size_t i = 0; i < v.size();) {
        std::size_t k = i + 1;  // the runs joined to run i
        while (k < v.size() && v[k].contig == v[i].contig && v[k].start == v[k - 1].end + 1 &&
               (in || v[k].depth_kept == v[i].depth_kept) && (!in && !both ? true : v[k].depth_in == v[i].depth_in))
            ++k;
        const char* name = v[i].contig < reference_names.size() ? reference_names[v[i].contig].c_str() : "*";
        const unsigned long long end = (unsigned long long)v[k - 1].end + 1;
        if (both) std::fprintf(f, "%s\t%u\t%llu\t%u\t%u\n", name, v[i].start, end, v[i].depth_in, v[i].depth_kept);
        else std::fprintf(f, "%s\t%u\t%llu\t%u\n", name, v[i].start, end, in ? v[i].depth_in : v[i].depth_kept);
        i = k;
    }
    return std::fclose(f) == 0;
}

bool write_depth_report_tsv(const std::filesystem::path& path, const DepthReport& report,
                            const std::vector<std::string>& reference_names) {
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (f == nullptr) return false;
    std::fputs("#kind\treference\tstart\tend\tpositions\tmean_in\tmean_kept\tmin_in\tmax_in\tmin_kept\tmax_kept\t"
               "capped_positions\tdeficit_positions\tdeficit_sum\n", f);
    auto rows = [&](const char* kind, const std::vector<qmcp_hip_depth_row>& v) {
        for (const qmcp_hip_depth_row& r : v) {
            const unsigned long long pos = r.positions;
            const unsigned long long end = pos ? (unsigned long long)r.end + 1 : r.start;
            const double mean_in = pos ? (double)r.sum_in / (double)pos : 0.0;
            const double mean_kept = pos ? (double)r.sum_kept / (double)pos : 0.0;
            const char* name = r.contig < reference_names.size() ? reference_names[r.contig].c_str() : "*";
            std::fprintf(f, "%s\t%s\t%u\t%llu\t%llu\t%.6f\t%.6f\t%u\t%u\t%u\t%u\t%llu\t%llu\t%llu\n", kind, name, r.start,
                         end, pos, mean_in, mean_kept, r.min_in, r.max_in, r.min_kept, r.max_kept,
                         (unsigned long long)r.capped_positions, (unsigned long long)r.deficit_positions,
                         (unsigned long long)r.deficit_sum);
        }
    };
    rows("contig", report.contig_rows);
    rows("region", report.region_rows);
    for (std::size_t b = 0; b < report.hist_in.size(); ++b)
        std::fprintf(f, "#hist\t%zu\t%llu\t%llu\n", b, (unsigned long long)report.hist_in[b],
                     (unsigned long long)report.hist_kept[b]);
    return std::fclose(f) == 0;
}

}  // namespace qmcp
