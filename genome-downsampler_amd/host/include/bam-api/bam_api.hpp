// In-memory BamApi: the part of the reference's BamApi the solver path and its tests use.
// Mirrors libs/bam-api/include/bam-api/bam_api.hpp:21-88 for
//   BamApi(const AOSPairedReads&) / BamApi(const SOAPairedReads&)   (bam_api.cpp:44-51)
//   get_paired_reads_aos / get_paired_reads_soa / get_paired_reads  (bam_api.cpp:189-233,303-309)
//   find_pairs                                                     (bam_api.cpp:239-273)
//   find_input_cover / find_filtered_cover                         (bam_api.cpp:275-301)
//   BamApi(path, BamApiConfig), read on first use, get_filtered_out_reads,
//   write_paired_reads, write_bam_api_filtered_out_reads            (bam_api.cpp:32-43,189-233,520-532)
// BAM files are read and written by bam-api/bam_io.hpp on zlib alone (HTSlib is not in this image).
#ifndef QMCP_AMD_BAM_API_BAM_API_HPP
#define QMCP_AMD_BAM_API_BAM_API_HPP

#include <cstdint>
#include <filesystem>
#include <optional>
#include <string>
#include <vector>

#include "bam-api/amplicon_set.hpp"
#include "bam-api/bam_io.hpp"
#include "bam-api/paired_reads.hpp"

namespace bam_api {

// bam_api_config.hpp:19-26
struct BamApiConfig {
    std::filesystem::path bed_filepath;
    std::filesystem::path tsv_filepath;
    std::uint32_t hts_thread_count = 1;  // kept for source compatibility; ingest here is single-threaded
    std::uint32_t min_seq_length = 0;
    std::uint32_t min_mapq = 0;
    AmpliconBehaviour amplicon_behaviour = AmpliconBehaviour::IGNORE;
    // Keep every read's reference (PairedReads::contig_ids / contig_lengths) instead of placing all reads on the first
    // one; the solver then solves one coverage problem per reference.  Amplicons (BED / TSV) only with
    // amplicons_by_reference below; without it the constructor throws std::invalid_argument.
    bool per_reference = false;
    // Match every BED line's chrom to a reference of the BAM header by name (exactly) and build the amplicons per
    // reference (build_reference_amplicon_set): FILTER keeps a pair only if both mates lie on one reference, inside
    // one of its amplicons; GRADE grades by the same predicate.  Needs per_reference (std::invalid_argument
    // otherwise); an unknown chrom or a TSV pair across references is a std::invalid_argument naming it.
    bool amplicons_by_reference = false;
    // On-target downsampling: a BED3+ file of target regions (0-based half-open; `track`, `browser` and `#` lines
    // skipped), every chrom matched exactly to a reference of the BAM header.  Coverage is capped inside the regions
    // (each widened by target_padding) only; reads that touch no region are dropped, or all kept with keep_off_target.
    // Needs per_reference (std::invalid_argument otherwise); an unknown chrom or a malformed line is a
    // std::invalid_argument naming it.  Independent of the amplicon files: FILTER / GRADE act at ingest, the targets in
    // the solve (the hip solvers call qmcp_hip_solve_targets_host when the BamApi holds targets).
    std::filesystem::path targets_filepath;
    std::uint32_t target_padding = 0;
    bool keep_off_target = false;
    // Depth report: after the output has been written, the caller (App::execute's place) asks the hip solver for the
    // depth of the reads the solve saw against the final kept set, per reference and per target region, and writes it
    // here as TSV (QuasiMcpHipSolver::depth_report / write_depth_report_tsv); depth_report_bins > 0 adds histograms.
    // Needs per_reference (std::invalid_argument otherwise).  Empty: no report, nothing changes.
    std::filesystem::path depth_report_filepath;
    std::uint32_t depth_report_bins = 0;
    // Depth track: after the output has been written, the per-base depth of the reads the solve saw against the final
    // kept set goes here as bedGraph (QuasiMcpHipSolver::depth_track / write_depth_track_bedgraph): the channel "kept",
    // "in" or "both", depths clamped to depth_track_cap (0: no clamp), inside the targets with their padding when the
    // BamApi holds any.  Needs per_reference; not together with a coverage ladder, stratify_by or dedup
    // (std::invalid_argument otherwise, also for another channel).  Empty: no track, nothing changes.
    std::filesystem::path depth_track_filepath;
    std::string depth_track_channel = "kept";
    std::uint32_t depth_track_cap = 0;
    // Coverage ladder: further coverages below the solve's max_coverage, strictly decreasing, each solved on the reads
    // the level above kept (QuasiMcpHipSolver::solve_ladder / qmcp_hip_solve_ladder_host), so the outputs are nested.
    // Needs per_reference; not together with targets or a depth report (std::invalid_argument otherwise).  Empty: no
    // ladder, nothing changes.
    std::vector<std::uint32_t> coverage_ladder;
    // Stratified downsampling: every read gets a stratum at ingest (bam_io.hpp's Stratify: by strand, or by the read
    // group of its RG:Z field) and QuasiMcpHipSolver::solve caps every stratum on its own
    // (qmcp_hip_solve_stratified_host): STRAND at ceil(M / 2) forward and floor(M / 2) reverse, READ_GROUP at M for
    // every read group.  Needs per_reference; not together with targets, a coverage ladder or a depth report
    // (std::invalid_argument otherwise).  NONE: nothing changes.
    Stratify stratify_by = Stratify::NONE;
    // Duplicate-aware downsampling: duplicate pairs -- equal unordered pair of (reference, start, end, strand) cells --
    // are collapsed to the pair of highest summed MAPQ before the solve (QuasiMcpHipSolver::solve_dedup /
    // qmcp_hip_solve_dedup_host in pair mode with mate completion); the ingest keeps every record's reverse-strand bit as
    // the reads' strata column for it.  Needs per_reference; not together with targets, a depth report, a coverage
    // ladder, stratify_by or amplicon files (std::invalid_argument otherwise).  false: nothing changes.
    bool dedup = false;
    // Start cap: every start site -- (reference, start), with start_cap_by_strand (reference, start, strand) -- offers the
    // solve at most start_cap reads: those of highest MAPQ, then the longest, then the first in the file's pairing order
    // (QuasiMcpHipSolver::solve_start_cap / qmcp_hip_solve_start_cap_host).  find_pairs then completes mates as always: it
    // only adds reads, so every floor the solve reached still holds, but a written start may exceed the cap through a
    // mate -- the cap is on what the solve may choose from.  With start_cap_by_strand the ingest keeps every record's
    // reverse-strand bit as the reads' strata column, as it does for dedup.  Needs per_reference; not together with any
    // other mode or with amplicon files (std::invalid_argument otherwise).  0: nothing changes.
    std::uint32_t start_cap = 0;
    bool start_cap_by_strand = false;
    // Tiered downsampling by MAPQ band (QuasiMcpHipSolver::solve_tiers / qmcp_hip_solve_tiers_host): strictly falling
    // thresholds, e.g. {30, 10, 0} -- a read of MAPQ >= mapq_tiers[0] is of tier 0, one below it and >= mapq_tiers[1] of
    // tier 1, and so on.  The best tier is solved first, a lower tier only fills what the better ones leave short of
    // min(coverage, max_coverage).  The last threshold must equal min_mapq, so that every read the ingest lets through has
    // a tier; at most QMCP_TIERS_MAX thresholds.  find_pairs completes mates as always: it only adds reads, so the floor
    // still holds.  Needs per_reference; not together with any other mode or with amplicon files (std::invalid_argument
    // otherwise).  Empty: nothing changes.
    std::vector<std::uint32_t> mapq_tiers;
    // Amplicon-aware downsampling (QuasiMcpHipSolver::solve_amplicons / qmcp_hip_solve_amplicons_host): primer_clip counts
    // depth on the reads clipped to their amplicon's insert (the amplicon without its primers, from the BED), per_amplicon
    // solves every amplicon as a coverage problem of its own ("every amplicon to M x"), amplicon_report_filepath gets one
    // line per amplicon; the report alone runs the entry with clipping off and pooled.  Clipping decides what counts as
    // depth, NOT what is written: the output holds the original, unclipped records of the kept reads, completed by
    // find_pairs as always.  All three need per_reference, amplicons_by_reference and a BED; together with any other
    // mode (targets, ladder, stratify_by, dedup, start cap, ...) the constructor throws std::invalid_argument, and so it
    // does under primer_clip for a primer pair that leaves no insert, naming the pair.
    bool primer_clip = false;
    bool per_amplicon = false;
    std::filesystem::path amplicon_report_filepath;
    // Pair-aware downsampling: the solve runs in stages that credit the coverage of the mates already kept
    // (QuasiMcpHipSolver::solve_pairs / qmcp_hip_solve_pairs_host), so the output -- whole pairs, written without a
    // further find_pairs -- stays near max_coverage instead of near twice that.  pair_stages: the stages' rising targets,
    // the last one max_coverage; empty: ceil(M / 2), then M.  Needs per_reference; not together with targets, a depth
    // report or track, a coverage ladder, stratify_by, dedup or amplicon files (std::invalid_argument otherwise).
    // false: nothing changes.
    bool pair_aware = false;
    std::vector<std::uint32_t> pair_stages;
    // Template-aware downsampling: the ingest is read_bam_templates (bam_io.hpp) -- one segment per aligned block of every
    // record, a template = the accepted records of one QNAME -- and the solve QuasiMcpHipSolver::solve_templates /
    // qmcp_hip_solve_templates_host: single-end reads, split reads with their supplementary alignments and spliced reads
    // are kept or dropped as whole templates, and an intron gets no depth.  split_spliced: cut a record at every N of its
    // CIGAR; include_secondary: take records with flag 0x100 instead of skipping them; template_stages: as pair_stages.
    // A record is written when its template is kept; no find_pairs follows.  Needs per_reference; not together with
    // pair_aware or anything pair_aware refuses (std::invalid_argument otherwise).  false: nothing changes, and the
    // three other fields must be left at their defaults.
    bool template_aware = false;
    bool split_spliced = true;
    bool include_secondary = false;
    std::vector<std::uint32_t> template_stages;
    // Fragment depth (with template_aware): a template counts once where its segments overlap -- the two mates of a
    // short-insert pair -- as in mosdepth, samtools depth -s and GATK.  QuasiMcpHipSolver::solve_templates then calls
    // qmcp_hip_solve_fragments_host, and solve_templates_profile calls qmcp_hip_clip_templates_host followed by the
    // profile entry on the clipped columns.  Needs template_aware (std::invalid_argument otherwise).
    bool fragment_depth = false;
    // Ceiling downsampling: max_coverage (and the caps of a coverage profile) bound the written depth from ABOVE, and as
    // many reads as possible are kept (QuasiMcpHipSolver::solve_ceiling / qmcp_hip_solve_ceiling_host with
    // QMCP_CEILING_WHOLE_PAIRS).  The output -- whole pairs -- is written from the final mask WITHOUT find_pairs, which
    // would put depth back.  The depth may fall below min(coverage, cap) next to deeper positions; the ceiling report
    // counts where.  Needs per_reference; goes together with a coverage profile and with nothing else pair_aware refuses,
    // and not with pair_aware or template_aware (std::invalid_argument otherwise).  false: nothing changes.
    bool ceiling = false;
    // Budget downsampling: the deepest coverage in 0 .. min(max_coverage, largest depth) whose solve, completed to whole
    // pairs, writes at most budget_reads records -- or at most floor(budget_fraction * placed reads), the placed reads
    // being those that passed the ingest filters (QuasiMcpHipSolver::solve_budget / qmcp_hip_solve_budget_host with
    // QMCP_BUDGET_WHOLE_PAIRS).  The output is written from the final mask WITHOUT find_pairs, which would add reads.
    // Exactly one of the two; budget_fraction in 0 .. 1.  Needs per_reference and goes together with nothing that
    // ceiling refuses, nor with ceiling or a coverage profile (std::invalid_argument otherwise).  Neither: nothing changes.
    std::optional<std::uint64_t> budget_reads;
    std::optional<double> budget_fraction;
    // Mean-depth downsampling: the deepest coverage in 0 .. min(max_coverage, largest depth) whose solve, completed to
    // whole pairs, writes at most budget_bases bases inside the regions of mean_depth_targets_filepath (a BED3+ file as
    // targets_filepath, no padding; empty: every position of every reference) -- or at most floor(mean_depth * the
    // regions' positions), the mean people quote as "30 x" or MEAN_TARGET_COVERAGE (QuasiMcpHipSolver::solve_mean_depth /
    // qmcp_hip_solve_mean_depth_host with QMCP_MEAN_DEPTH_WHOLE_PAIRS).  The output is written from the final mask
    // WITHOUT find_pairs, which would add bases.  Exactly one of the two; mean_depth finite and >= 0.  Needs
    // per_reference and goes together with nothing that budget downsampling refuses, nor with a budget, replicates, a
    // proportion or a coverage profile (std::invalid_argument otherwise).  Neither: nothing changes.
    std::optional<double> mean_depth;
    std::optional<std::uint64_t> budget_bases;
    std::filesystem::path mean_depth_targets_filepath;
    // Disjoint replicates: the coverages of replicates 2 .. K (an empty list: one replicate); replicate 1 is solved at
    // the solve's max_coverage, replicate r + 1 on the reads the earlier ones left free
    // (QuasiMcpHipSolver::solve_replicates / qmcp_hip_solve_replicates_host with QMCP_REPLICATES_WHOLE_PAIRS |
    // QMCP_REPLICATES_SHORTFALL).  Every file is written from its label WITHOUT find_pairs, which would copy a record
    // into two files.  Each coverage in 1 .. 2^31 - 1, at most QMCP_REPLICATES_MAX - 1 of them.  Needs per_reference and
    // goes together with nothing that budget downsampling refuses, nor with a budget or a coverage profile
    // (std::invalid_argument otherwise).  Not set: nothing changes.
    std::optional<std::vector<std::uint32_t>> replicates;
    // Proportional downsampling: every position keeps at least ceil(cov * num / den) of its depth, positions at or below
    // `floor` whole, max_coverage a hard upper end of the demand (QuasiMcpHipSolver::solve_proportional /
    // qmcp_hip_solve_proportional_host).  find_pairs completes mates as always -- it only adds reads, so every floor
    // still holds.  0 <= num <= den, 1 <= den <= QMCP_PROPORTION_DEN_MAX.  Needs per_reference and goes together with
    // nothing that disjoint replicates refuse, nor with replicates or a coverage profile (std::invalid_argument
    // otherwise).  Not set: nothing changes.
    struct Proportion {
        std::uint32_t num = 0, den = 1, floor = 0;
    };
    std::optional<Proportion> proportion;
    // Coverage thresholds: every pair's smallest coverage in thresholds_lo .. thresholds_hi at which the by-contig solve,
    // completed to whole pairs, keeps it (QuasiMcpHipSolver::solve_thresholds / qmcp_hip_solve_thresholds_host with
    // QMCP_THRESHOLDS_WHOLE_PAIRS).  The records with a threshold are written WITHOUT find_pairs, each with the aux field
    // <thresholds_tag>:S:<threshold>, so that any downsample of the range is a filter on the tag.  thresholds_hi set asks
    // for it; 1 <= thresholds_lo <= thresholds_hi <= QMCP_THRESHOLDS_COVERAGE_MAX, the tag [A-Za-z][A-Za-z0-9].  Needs
    // per_reference and goes together with nothing that proportional downsampling refuses, nor with a proportion or a
    // mean depth (std::invalid_argument otherwise).  Not set: nothing changes.
    std::uint32_t thresholds_lo = 1;
    std::optional<std::uint32_t> thresholds_hi;
    std::string thresholds_tag = "XC";
};

// the parsed target BED of BamApiConfig::targets_filepath: reference c owns regions [offsets[c], offsets[c + 1]) of
// starts / ends (inclusive bounds, file order), as qmcp_hip_solve_targets_host takes them
struct TargetRegions {
    std::vector<std::uint32_t> offsets, starts, ends;
    std::uint32_t padding = 0;
    bool keep_off_target = false;
};

// false + *err: the file cannot be opened, a line is malformed, or a chrom names no reference
bool target_regions_from_bed(const std::filesystem::path& bed, const std::vector<std::string>& ref_names,
                             TargetRegions& out, std::string* err);

class BamApi {
   public:
    // reading and filtering happen on the first get_paired_reads_* call (bam_api.cpp:189-233)
    BamApi(const std::filesystem::path& input_filepath, const BamApiConfig& config);
    explicit BamApi(const AOSPairedReads& paired_reads);
    explicit BamApi(const SOAPairedReads& paired_reads);

    const AOSPairedReads& get_paired_reads_aos();
    const SOAPairedReads& get_paired_reads_soa();
    const PairedReads& get_paired_reads() const;
    void set_amplicon_behaviour(AmpliconBehaviour b) { amplicon_behaviour_ = b; }
    const std::vector<BAMReadId>& get_filtered_out_reads() const { return filtered_out_reads_; }
    // BamApiConfig::targets_filepath was given: the solve is capped inside these regions only
    bool has_targets() const { return has_targets_; }
    const TargetRegions& get_targets() const { return targets_; }
    // BamApiConfig::depth_report_filepath (empty: none) and depth_report_bins
    const std::filesystem::path& depth_report_filepath() const { return depth_report_filepath_; }
    std::uint32_t depth_report_bins() const { return depth_report_bins_; }
    // BamApiConfig::depth_track_filepath (empty: none), depth_track_channel and depth_track_cap
    const std::filesystem::path& depth_track_filepath() const { return depth_track_filepath_; }
    const std::string& depth_track_channel() const { return depth_track_channel_; }
    std::uint32_t depth_track_cap() const { return depth_track_cap_; }
    // BamApiConfig::coverage_ladder (empty: none)
    const std::vector<std::uint32_t>& coverage_ladder() const { return coverage_ladder_; }
    // BamApiConfig::stratify_by (NONE: the reads carry no strata)
    Stratify stratify_by() const { return stratify_by_; }
    // BamApiConfig::dedup (the reads' strata column then holds the reverse-strand bit)
    bool dedup() const { return dedup_; }
    // BamApiConfig::start_cap (0: none) and start_cap_by_strand (the reads' strata column then holds the strand bit)
    std::uint32_t start_cap() const { return start_cap_; }
    // BamApiConfig::mapq_tiers (empty: no tiered solve)
    const std::vector<std::uint32_t>& mapq_tiers() const { return mapq_tiers_; }
    bool start_cap_by_strand() const { return start_cap_by_strand_; }
    // BamApiConfig::primer_clip, per_amplicon and amplicon_report_filepath; the amplicons matched to the references
    bool primer_clip() const { return primer_clip_; }
    bool per_amplicon() const { return per_amplicon_; }
    const std::filesystem::path& amplicon_report_filepath() const { return amplicon_report_filepath_; }
    const ReferenceAmpliconSet& reference_amplicons() const { return reference_amplicon_set_; }
    // BamApiConfig::pair_aware and pair_stages (empty: the default schedule)
    bool pair_aware() const { return pair_aware_; }
    const std::vector<std::uint32_t>& pair_stages() const { return pair_stages_; }
    // BamApiConfig::ceiling
    bool ceiling() const { return ceiling_; }
    // BamApiConfig::budget_reads / budget_fraction: whether one is set, and the budget for a number of placed reads
    bool budget() const { return budget_reads_.has_value() || budget_fraction_.has_value(); }
    std::uint64_t budget_for(std::uint64_t placed_reads) const;
    // BamApiConfig::mean_depth / budget_bases: whether one is set, the regions of mean_depth_targets_filepath (none: every
    // position), their positions after clipping to the references and merging, and the budget in bases
    bool mean_depth() const { return mean_depth_.has_value() || budget_bases_.has_value(); }
    bool has_mean_depth_regions() const { return has_mean_depth_regions_; }
    const TargetRegions& mean_depth_regions() const { return mean_depth_regions_; }
    std::uint64_t mean_depth_positions(const std::vector<std::uint32_t>& contig_lengths) const;
    std::uint64_t base_budget_for(std::uint64_t positions) const;
    // BamApiConfig::replicates (not set: no replicate split)
    const std::optional<std::vector<std::uint32_t>>& replicates() const { return replicates_; }
    // BamApiConfig::proportion (not set: no proportional solve)
    const std::optional<BamApiConfig::Proportion>& proportion() const { return proportion_; }
    // BamApiConfig::thresholds_lo / thresholds_hi / thresholds_tag (thresholds_hi not set: no thresholds)
    bool thresholds() const { return thresholds_hi_.has_value(); }
    std::uint32_t thresholds_lo() const { return thresholds_lo_; }
    std::uint32_t thresholds_hi() const { return thresholds_hi_.value_or(0); }
    const std::string& thresholds_tag() const { return thresholds_tag_; }
    // BamApiConfig::template_aware and template_stages (empty: the default schedule); the segments are read on the first
    // get_template_segments call, which also fills get_filtered_out_reads
    bool template_aware() const { return template_aware_; }
    bool fragment_depth() const { return fragment_depth_; }
    const std::vector<std::uint32_t>& template_stages() const { return template_stages_; }
    const TemplateSegments& get_template_segments();
    // the records with these ids (sorted in place), copied from the input; number of records written
    std::uint32_t write_records(const std::filesystem::path& output_filepath, std::vector<BAMReadId>& bam_ids) const;
    // number of records written; the output is always BAM
    std::uint32_t write_paired_reads(const std::filesystem::path& output_filepath,
                                     std::vector<ReadIndex>& active_ids) const;
    // the reads active_ids, each record with the aux field <tag>:S:<values[k]> appended (values: one per active id);
    // std::invalid_argument, before anything is written, for a bad tag and for a record that carries the tag already
    std::uint32_t write_tagged_reads(const std::filesystem::path& output_filepath, const std::vector<ReadIndex>& active_ids,
                                     const std::vector<std::uint16_t>& values, const std::string& tag) const;
    std::uint32_t write_bam_api_filtered_out_reads(const std::filesystem::path& output_filepath);

    std::vector<ReadIndex> find_pairs(const std::vector<ReadIndex>& ids) const;

    // testing purposes (same role as in the reference)
    std::vector<std::uint32_t> find_input_cover();
    std::vector<std::uint32_t> find_filtered_cover(const std::vector<ReadIndex>& active_ids);

   private:
    SOAPairedReads soa_paired_reads_;
    bool is_soa_loaded_ = false;
    AOSPairedReads aos_paired_reads_;
    bool is_aos_loaded_ = false;
    AmpliconSet amplicon_set_;
    ReferenceAmpliconSet reference_amplicon_set_;
    AmpliconBehaviour amplicon_behaviour_ = AmpliconBehaviour::IGNORE;
    std::vector<BAMReadId> filtered_out_reads_;
    std::filesystem::path input_filepath_;
    std::uint32_t min_seq_length_ = 0, min_mapq_ = 0;
    bool per_reference_ = false, amplicons_by_reference_ = false;
    TargetRegions targets_;
    bool has_targets_ = false;
    std::filesystem::path depth_report_filepath_;
    std::uint32_t depth_report_bins_ = 0;
    std::filesystem::path depth_track_filepath_;
    std::string depth_track_channel_ = "kept";
    std::uint32_t depth_track_cap_ = 0;
    std::vector<std::uint32_t> coverage_ladder_;
    Stratify stratify_by_ = Stratify::NONE;
    bool dedup_ = false;
    std::uint32_t start_cap_ = 0;
    std::vector<std::uint32_t> mapq_tiers_;
    bool start_cap_by_strand_ = false;
    bool primer_clip_ = false, per_amplicon_ = false;
    std::filesystem::path amplicon_report_filepath_;
    bool pair_aware_ = false;
    bool ceiling_ = false;
    std::optional<std::uint64_t> budget_reads_;
    std::optional<double> budget_fraction_;
    std::optional<double> mean_depth_;
    std::optional<std::uint64_t> budget_bases_;
    TargetRegions mean_depth_regions_;
    bool has_mean_depth_regions_ = false;
    std::optional<std::vector<std::uint32_t>> replicates_;
    std::optional<BamApiConfig::Proportion> proportion_;
    std::uint32_t thresholds_lo_ = 1;
    std::optional<std::uint32_t> thresholds_hi_;
    std::string thresholds_tag_ = "XC";
    std::vector<std::uint32_t> pair_stages_;
    bool template_aware_ = false, split_spliced_ = true, include_secondary_ = false, fragment_depth_ = false;
    std::vector<std::uint32_t> template_stages_;
    TemplateSegments template_segments_;
    bool are_segments_loaded_ = false;
    void read_bam_into(PairedReads& reads);
};

}  // namespace bam_api
#endif
