// "quasi-mcp-hip": the MI355X solver behind the reference's plugin surface.
// Takes the place QuasiMcpCudaMaxFlowSolver has in the reference
// (libs/qmcp-solver/include/qmcp-solver/quasi_mcp_cuda_max_flow_solver.hpp:17-36):
// same base class, same two overrides, uses_quality_of_reads() == false so the app selects
// amplicon FILTER (src/app.cpp:121-127).  All device work goes through the C ABI in
// include/qmcp_hip.h; this class only hands over the SoA columns and expands the keep mask.
#ifndef QMCP_AMD_QUASI_MCP_HIP_SOLVER_HPP
#define QMCP_AMD_QUASI_MCP_HIP_SOLVER_HPP

#include <chrono>
#include <cstdint>
#include <filesystem>
#include <memory>
#include <string>
#include <vector>

#include "qmcp-solver/adapter_columns.hpp"
#include "qmcp-solver/solver.hpp"
#include "qmcp_hip.h"

namespace qmcp {

// qmcp_hip_depth_report_host's outputs
struct DepthReport {
    std::vector<qmcp_hip_depth_row> contig_rows, region_rows;
    std::vector<std::uint64_t> hist_in, hist_kept;
    qmcp_hip_depth_stats stats{};
};

// the report as TSV: a '#'-prefixed header line, one line per contig row and per region row (start 0-based, end
// exclusive, means with six decimals), then '#hist' lines when there are histograms.  false: the file cannot be written
bool write_depth_report_tsv(const std::filesystem::path& path, const DepthReport& report,
                            const std::vector<std::string>& reference_names);

// qmcp_hip_depth_track_host's outputs
struct DepthTrack {
    std::vector<qmcp_hip_track_run> runs;
    qmcp_hip_track_stats stats{};
};

// the runs as bedGraph (chrom, start, end + 1, value; 0-based half-open): channel "kept" or "in" writes that depth, "both"
// writes depth_in and depth_kept under a '#' header line.  Neighbouring runs of one contig that touch and have the same
// written value(s) are joined.  false: another channel, or the file cannot be written
bool write_depth_track_bedgraph(const std::filesystem::path& path, const DepthTrack& track,
                                const std::vector<std::string>& reference_names, const std::string& channel);

class QuasiMcpHipSolver : public Solver {
   public:
    QuasiMcpHipSolver() = default;  // trivial: solvers are built eagerly (src/app.hpp:35)
    ~QuasiMcpHipSolver() override;
    QuasiMcpHipSolver(const QuasiMcpHipSolver&) = delete;
    QuasiMcpHipSolver& operator=(const QuasiMcpHipSolver&) = delete;

    std::unique_ptr<Solution> solve(std::uint32_t required_cover,
                                    bam_api::BamApi& bam_api) override;
    bool uses_quality_of_reads() override { return false; }

    void set_device(int device);  // before the first solve; default 0
    // devices for multi-contig callers of the C ABI's qmcp_hip_multi_* entry points; the reference's BamApi
    // holds ONE contig (libs/bam-api/src/bam_api.cpp:422), which is one independent problem, so solve()
    // below runs it on the first device of the list
    void set_devices(const std::vector<int>& devices) { if (!devices.empty()) { devices_ = devices; device_ = devices[0]; } }
    const std::vector<int>& devices() const { return devices_; }
    // complete mate pairs on the device before returning (what src/app.cpp:141 does on the
    // host with BamApi::find_pairs); off by default, like the reference solvers
    void set_complete_pairs(bool on) { complete_pairs_ = on; }
    // Depth before and after, for the reads of a per-reference BamApi against the kept set `kept` (ascending or not;
    // App::execute would pass find_pairs' result after write_paired_reads): qmcp_hip_depth_report_host with
    // M = required_cover, the BamApi's target regions and padding when it holds any, n_bins histogram bins.
    // std::terminate on a device failure, like solve()
    void depth_report(std::uint32_t required_cover, bam_api::BamApi& bam_api, const std::vector<bam_api::ReadIndex>& kept,
                      std::uint32_t n_bins, DepthReport& out);
    // The per-base form of depth_report, for the same reads and kept set: qmcp_hip_depth_track_host with
    // M = required_cover, the BamApi's target regions and padding when it holds any, `flags` (QMCP_TRACK_*) and
    // depth_cap; counted first, then fetched at the exact size.  std::terminate on a device failure, like solve()
    void depth_track(std::uint32_t required_cover, bam_api::BamApi& bam_api, const std::vector<bam_api::ReadIndex>& kept,
                     std::uint32_t flags, std::uint32_t depth_cap, DepthTrack& out);
    // Coverage ladder for the reads of a per-reference BamApi: the solve at required_cover, then at each of `levels`
    // (strictly below required_cover, strictly decreasing, >= 1; std::invalid_argument otherwise) on the reads the
    // level above kept, in one qmcp_hip_solve_ladder_host call.  One ascending Solution per level, required_cover's
    // first; each is a subset of the one before.  Mate completion is left to the caller (BamApi::find_pairs is
    // monotone, so completed levels stay nested).  std::terminate on a device failure, like solve()
    std::vector<std::unique_ptr<Solution>> solve_ladder(std::uint32_t required_cover, bam_api::BamApi& bam_api,
                                                        const std::vector<std::uint32_t>& levels);
    const qmcp_hip_ladder_stats& last_ladder_stats() const { return lstats_; }
    // Stratified reads (BamApiConfig::stratify_by): solve() caps every stratum on its own through
    // qmcp_hip_solve_stratified_host -- STRAND at ceil(M / 2) and floor(M / 2), READ_GROUP at M for every stratum.
    // The caps and the rows of the last such solve, one per stratum of the reads' stratum_names
    static std::vector<std::uint32_t> stratum_caps(std::uint32_t required_cover, bam_api::Stratify by, std::size_t n_strata);
    const std::vector<std::uint32_t>& last_stratum_caps() const { return stratum_caps_; }
    const std::vector<qmcp_hip_stratum_row>& last_stratum_rows() const { return stratum_rows_; }
    // Duplicate-aware downsampling for the reads of a BamApi built with BamApiConfig::dedup: qmcp_hip_solve_dedup_host
    // in pair mode with mate completion, tag = the reads' strand bit, quality = MAPQ; hist_bins bins of family sizes.
    // Duplicate pairs are not in the Solution.  std::invalid_argument for reads without contig ids or strand column;
    // std::terminate on a device failure, like solve()
    std::unique_ptr<Solution> solve_dedup(std::uint32_t required_cover, bam_api::BamApi& bam_api, std::uint32_t hist_bins);
    const qmcp_hip_dedup_stats& last_dedup_stats() const { return dstats_; }
    const std::vector<std::uint64_t>& last_dedup_hist() const { return dedup_hist_; }
    // Start cap for the reads of a BamApi built with BamApiConfig::start_cap: qmcp_hip_solve_start_cap_host with
    // QMCP_START_CAP_SHORTFALL, group = the reads' strand bit under start_cap_by_strand (else one group), priority = MAPQ;
    // hist_bins bins of cell sizes.  The Solution is the solve's own kept set: find_pairs completes it.
    // std::invalid_argument for reads without contig ids (or without the strand column it asks for); std::terminate on a
    // device failure, like solve()
    std::unique_ptr<Solution> solve_start_cap(std::uint32_t required_cover, bam_api::BamApi& bam_api, std::uint32_t hist_bins);
    const qmcp_hip_start_cap_stats& last_start_cap_stats() const { return scstats_; }
    const std::vector<std::uint64_t>& last_start_cap_hist() const { return start_cap_hist_; }
    // Amplicon-aware downsampling for the reads of a BamApi built with BamApiConfig::primer_clip, per_amplicon or
    // amplicon_report_filepath: qmcp_hip_solve_amplicons_host on the pairs with QMCP_AMPLICONS_COMPLETE_PAIRS, the table
    // and (under primer_clip) the inserts of the BamApi's reference amplicons, per amplicon or pooled.  The Solution holds
    // whole pairs; last_amplicon_labels() has one label per pair, last_amplicon_rows() one row per amplicon over the
    // insert the solve used.  Throws std::invalid_argument for a BamApi configured otherwise.
    std::unique_ptr<Solution> solve_amplicons(std::uint32_t required_cover, bam_api::BamApi& bam_api);
    const qmcp_hip_amplicons_stats& last_amplicons_stats() const { return astats_; }
    const std::vector<std::uint32_t>& last_amplicon_labels() const { return amplicon_labels_; }
    const std::vector<qmcp_hip_depth_row>& last_amplicon_rows() const { return amplicon_rows_; }
    // Coverage profile for the reads of a per-reference BamApi: qmcp_hip_solve_profile_host with the regions in CSR form
    // per reference (offsets: one more entry than the file has references; inclusive bounds, disjoint per reference)
    // and required_cover as the default cap.  std::invalid_argument for reads without contig ids or a table of other
    // references, and for what the library refuses in the table (overlap, start > end, a cap of 2^31 or more);
    // std::terminate on a device failure, like solve()
    std::unique_ptr<Solution> solve_profile(std::uint32_t required_cover, bam_api::BamApi& bam_api,
                                            const std::vector<std::uint32_t>& offsets, const std::vector<std::uint32_t>& starts,
                                            const std::vector<std::uint32_t>& ends, const std::vector<std::uint32_t>& caps);
    const qmcp_hip_profile_stats& last_profile_stats() const { return pstats_; }
    // Pair-aware downsampling for the reads of a BamApi built with BamApiConfig::pair_aware: qmcp_hip_solve_pairs_host
    // under its pair_stages (empty: the default schedule).  The Solution holds whole pairs already -- the caller writes it
    // without find_pairs.  std::invalid_argument for reads without contig ids, an odd number of reads and a refused
    // stage list (the library's message)
    std::unique_ptr<Solution> solve_pairs(std::uint32_t required_cover, bam_api::BamApi& bam_api);
    const qmcp_hip_pair_stats& last_pair_stats() const { return prstats_; }
    // Ceiling downsampling for the reads of a BamApi built with BamApiConfig::ceiling: qmcp_hip_solve_ceiling_host with
    // QMCP_CEILING_WHOLE_PAIRS, the regions as solve_profile takes them (all empty: none) and required_cover as the cap
    // elsewhere.  The Solution holds whole pairs already -- the caller writes it without find_pairs.
    // std::invalid_argument as solve_profile, and for an odd number of reads
    std::unique_ptr<Solution> solve_ceiling(std::uint32_t required_cover, bam_api::BamApi& bam_api,
                                            const std::vector<std::uint32_t>& offsets, const std::vector<std::uint32_t>& starts,
                                            const std::vector<std::uint32_t>& ends, const std::vector<std::uint32_t>& caps);
    const qmcp_hip_ceiling_stats& last_ceiling_stats() const { return clstats_; }
    // Proportional downsampling for the reads of a BamApi built with BamApiConfig::proportion: one
    // qmcp_hip_solve_proportional_host call with its num / den and floor, and required_cover as the hard upper end of the
    // demand (2^31 - 1: none).  The caller completes pairs with find_pairs, as after solve_profile.
    // std::invalid_argument for a BamApi without a proportion and for what the library refuses
    std::unique_ptr<Solution> solve_proportional(std::uint32_t required_cover, bam_api::BamApi& bam_api);
    const qmcp_hip_proportional_stats& last_proportional_stats() const { return ppstats_; }
    // Tiered downsampling for the reads of a BamApi built with BamApiConfig::mapq_tiers: every read's tier from its MAPQ
    // (the band it falls in; below the last threshold: QMCP_NO_TIER), then one qmcp_hip_solve_tiers_host call at
    // required_cover.  The caller completes pairs with find_pairs.  last_tier_rows has one row per threshold.
    // std::invalid_argument for a BamApi without mapq_tiers and for what the library refuses
    std::unique_ptr<Solution> solve_tiers(std::uint32_t required_cover, bam_api::BamApi& bam_api);
    const std::vector<qmcp_hip_tier_row>& last_tier_rows() const { return tier_rows_; }
    const qmcp_hip_tiers_stats& last_tiers_stats() const { return trstats_; }
    // Budget downsampling for the reads of a BamApi built with BamApiConfig::budget_reads or budget_fraction: one
    // qmcp_hip_solve_budget_host call with QMCP_BUDGET_WHOLE_PAIRS, required_cover as the upper end of the search and
    // BamApi::budget_for(placed reads) as the budget.  The Solution holds whole pairs already -- the caller writes it
    // without find_pairs.  std::invalid_argument for a BamApi without a budget and for what the library refuses
    std::unique_ptr<Solution> solve_budget(std::uint32_t required_cover, bam_api::BamApi& bam_api);
    const qmcp_hip_budget_stats& last_budget_stats() const { return bgstats_; }
    // S(M) = the bases any answer at coverage M must hold, M = 0 .. last_budget_stats().curve_entries - 1
    const std::vector<std::uint64_t>& last_budget_curve() const { return budget_curve_; }
    // Coverage thresholds for the reads of a BamApi built with BamApiConfig::thresholds_hi: one
    // qmcp_hip_solve_thresholds_host call with QMCP_THRESHOLDS_WHOLE_PAIRS over thresholds_lo .. thresholds_hi.  The
    // Solution holds the reads with a threshold (whole pairs already -- the caller writes them without find_pairs),
    // last_thresholds() one threshold per read of the BamApi, last_threshold_counts() the reads at every coverage of
    // the range.  std::invalid_argument for a BamApi without thresholds and for what the library refuses
    std::unique_ptr<Solution> solve_thresholds(bam_api::BamApi& bam_api);
    const qmcp_hip_thresholds_stats& last_thresholds_stats() const { return thstats_; }
    const std::vector<std::uint16_t>& last_thresholds() const { return thresholds_; }
    const std::vector<std::uint64_t>& last_threshold_counts() const { return threshold_counts_; }
    // Mean-depth downsampling for the reads of a BamApi built with BamApiConfig::mean_depth or budget_bases: one
    // qmcp_hip_solve_mean_depth_host call with QMCP_MEAN_DEPTH_WHOLE_PAIRS, required_cover as the upper end of the search,
    // the BamApi's mean-depth regions (none: every position) and BamApi::base_budget_for(their positions) as the budget.
    // The Solution holds whole pairs already -- the caller writes it without find_pairs.  std::invalid_argument for a
    // BamApi without a mean depth and for what the library refuses
    std::unique_ptr<Solution> solve_mean_depth(std::uint32_t required_cover, bam_api::BamApi& bam_api);
    const qmcp_hip_mean_depth_stats& last_mean_depth_stats() const { return mdstats_; }
    // S_R(M) = the bases inside the regions any answer at coverage M must hold, M = 0 .. curve_entries - 1
    const std::vector<std::uint64_t>& last_mean_depth_curve() const { return mean_depth_curve_; }
    // Disjoint replicates for the reads of a BamApi built with BamApiConfig::replicates: one
    // qmcp_hip_solve_replicates_host call with QMCP_REPLICATES_WHOLE_PAIRS | QMCP_REPLICATES_SHORTFALL at required_cover,
    // then the BamApi's further coverages.  Returns one byte per read, the replicate that holds it (1-based, 0: none);
    // a replicate holds whole pairs already -- the caller writes it without find_pairs.  std::invalid_argument for a
    // BamApi without replicates and for what the library refuses
    std::vector<std::uint8_t> solve_replicates(std::uint32_t required_cover, bam_api::BamApi& bam_api);
    const qmcp_hip_replicates_stats& last_replicates_stats() const { return rpstats_; }
    // Template-aware downsampling for a BamApi built with BamApiConfig::template_aware: qmcp_hip_solve_templates_host on
    // its segments under its template_stages (empty: the default schedule).  Returns the ids of the records whose
    // template is kept (ascending) -- the caller writes them with BamApi::write_records, without find_pairs.
    // std::invalid_argument for a BamApi without template_aware and a refused stage list (the library's message)
    std::vector<bam_api::BAMReadId> solve_templates(std::uint32_t required_cover, bam_api::BamApi& bam_api);
    const qmcp_hip_template_stats& last_template_stats() const { return tpstats_; }
    // solve_templates under a cap per region: qmcp_hip_solve_templates_profile_host with the regions in CSR form per
    // reference (as solve_profile takes them), default_cap outside them, and required_cover as the scale of the
    // BamApi's template_stages.  Returns the ids of the records whose template is kept, as solve_templates does.
    // std::invalid_argument in addition for a table of other references and for what the library refuses in the table
    std::vector<bam_api::BAMReadId> solve_templates_profile(std::uint32_t required_cover, bam_api::BamApi& bam_api,
                                                            const std::vector<std::uint32_t>& offsets,
                                                            const std::vector<std::uint32_t>& starts,
                                                            const std::vector<std::uint32_t>& ends,
                                                            const std::vector<std::uint32_t>& caps,
                                                            std::uint32_t default_cap);
    const qmcp_hip_template_profile_stats& last_template_profile_stats() const { return tqstats_; }
    // With BamApiConfig::fragment_depth both count a template once where its segments overlap: solve_templates calls
    // qmcp_hip_solve_fragments_host, solve_templates_profile calls qmcp_hip_clip_templates_host and runs the profile entry
    // on the clipped columns.  What the clip did (zeros without fragment_depth):
    const qmcp_hip_fragment_stats& last_fragment_stats() const { return frstats_; }
    const qmcp_hip_stats& last_stats() const { return stats_; }
    const qmcp_hip_target_stats& last_target_stats() const { return tstats_; }
    // host wall-clock of the last solve(): the library's parts, the mask -> Solution expansion, the whole call
    const qmcp_hip_host_breakdown& last_breakdown() const { return breakdown_; }
    float last_expand_ms() const { return ms_expand_; }
    float last_solve_call_ms() const { return ms_solve_call_; }

   protected:  // (QuasiMcpHipQualitySolver shares the helpers and the state)
    // what solve() hands over to, by what the reads carry
    std::unique_ptr<Solution> solve_by_contig(std::uint32_t required_cover, const bam_api::SOAPairedReads& reads,
                                              std::chrono::steady_clock::time_point t0);
    // the BamApi holds target regions (BamApiConfig::targets_filepath): qmcp_hip_solve_targets_host, with the reads'
    // qualities when `with_qualities`
    std::unique_ptr<Solution> solve_targets(std::uint32_t required_cover, const bam_api::SOAPairedReads& reads,
                                            const bam_api::TargetRegions& targets, bool with_qualities,
                                            std::chrono::steady_clock::time_point t0);
    std::unique_ptr<Solution> solve_stratified(std::uint32_t required_cover, const bam_api::SOAPairedReads& reads,
                                               bam_api::Stratify by, std::chrono::steady_clock::time_point t0);

    // The steps every entry shares.  The reference's GPU solver has no error channel: a device failure ends in
    // std::terminate(), and so does die(), under the solver's name
    virtual const char* name() const { return "quasi-mcp-hip"; }
    [[noreturn]] void die(const char* what, int rc) const;
    // the two return-code policies: any failure ends the process; or QMCP_EINVAL / QMCP_ERANGE -- what the library
    // refuses in the arguments -- throw std::invalid_argument with its message and anything else ends the process
    void ok_or_die(const char* what, int rc) const;
    void ok_or_throw(const char* what, int rc) const;
    qmcp_hip_ctx* context();  // created on first use, reused across solves; die() on failure
    // the reads' 64-bit coordinates as the uint32 columns of the C ABI (narrow_columns, by the contig ids when the
    // reads have them) and the number of placed reads; die("narrowing a coordinate") on a coordinate above UINT32_MAX
    struct Columns {
        std::vector<std::uint32_t> starts, ends;
        std::uint64_t placed = 0;
    };
    Columns narrowed(const bam_api::SOAPairedReads& reads) const;
    static bool one_contig_id_each(const bam_api::SOAPairedReads& reads);
    // std::invalid_argument(message) unless the BamApi is `configured` for the entry and holds per-reference reads with
    // one contig id each
    static void need_per_reference(bool configured, const bam_api::SOAPairedReads& reads, const char* message);
    // a region table in CSR form against n_refs references: std::invalid_argument for a table of other references and
    // for arrays shorter than the offsets say
    static void check_regions(const std::vector<std::uint32_t>& offsets, const std::vector<std::uint32_t>& starts,
                              const std::vector<std::uint32_t>& ends, const std::vector<std::uint32_t>& caps,
                              std::size_t n_refs);
    // the context's keep mask of n reads as the ascending Solution, sized by `upper` kept reads at most; stamps
    // ms_expand_ and, from t0, ms_solve_call_
    std::unique_ptr<Solution> expand(std::uint64_t n, std::uint64_t upper, std::chrono::steady_clock::time_point t0);
    // ... with the upper bound of a solve that left stats_.n_kept: twice that under complete_pairs_
    std::unique_ptr<Solution> expand_kept(std::uint64_t n, std::chrono::steady_clock::time_point t0);
    // the end of an entry that solved into `mask`: no breakdown, mates completed if asked, expand_kept
    std::unique_ptr<Solution> finish(std::vector<std::uint64_t>& mask, std::uint64_t n,
                                     std::chrono::steady_clock::time_point t0);

    qmcp_hip_ctx* ctx_ = nullptr;
    int device_ = 0;
    std::vector<int> devices_{0};
    bool complete_pairs_ = false;
    qmcp_hip_stats stats_{};
    qmcp_hip_host_breakdown breakdown_{};
    float ms_expand_ = 0.f, ms_solve_call_ = 0.f;
    // what the last call of each entry left, in the order of the entries above
    qmcp_hip_ladder_stats lstats_{};
    std::vector<std::uint32_t> stratum_caps_;
    std::vector<qmcp_hip_stratum_row> stratum_rows_;
    qmcp_hip_dedup_stats dstats_{};
    std::vector<std::uint64_t> dedup_hist_;
    qmcp_hip_start_cap_stats scstats_{};
    std::vector<std::uint64_t> start_cap_hist_;
    qmcp_hip_amplicons_stats astats_{};
    std::vector<std::uint32_t> amplicon_labels_;
    std::vector<qmcp_hip_depth_row> amplicon_rows_;
    qmcp_hip_profile_stats pstats_{};
    qmcp_hip_pair_stats prstats_{};
    qmcp_hip_ceiling_stats clstats_{};
    qmcp_hip_proportional_stats ppstats_{};
    std::vector<qmcp_hip_tier_row> tier_rows_;
    qmcp_hip_tiers_stats trstats_{};
    qmcp_hip_budget_stats bgstats_{};
    std::vector<std::uint64_t> budget_curve_;
    qmcp_hip_thresholds_stats thstats_{};
    std::vector<std::uint16_t> thresholds_;
    std::vector<std::uint64_t> threshold_counts_;
    qmcp_hip_mean_depth_stats mdstats_{};
    std::vector<std::uint64_t> mean_depth_curve_;
    qmcp_hip_replicates_stats rpstats_{};
    qmcp_hip_template_stats tpstats_{};
    qmcp_hip_template_profile_stats tqstats_{};
    qmcp_hip_fragment_stats frstats_{};
    qmcp_hip_target_stats tstats_{};
};

}  // namespace qmcp
#endif
