// C entry points of libqmcp_host.so for ctypes callers (tests, bench.py): the reads-gen
// restatement and the C++ solver adapter driven exactly as the reference drives a solver
// (SolverManager::get(name).solve(M, BamApi)).
#include <chrono>
#include <new>
#include <cstdint>
#include <cstring>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>

#include "bam-api/amplicon_set.hpp"
#include "bam-api/bam_api.hpp"
#include "bam-api/bam_io.hpp"
#include "qmcp_host_request.h"
#include "qmcp-solver/quasi_mcp_hip_quality_solver.hpp"
#include "reads_gen.hpp"
#include "solver_manager.hpp"

namespace {

// Weight functions of the reference's CoverageTester (src/tests/coverage_tester.cpp:157-175).
double low_both_sides(double x) { return x - x * x; }
double with_hole(double x) {
    if (x > 0.3684 && x < 0.6316) return 1000.0 * (x * x - x + 0.25) * (x * x - x + 0.25) + 0.2;
    return 0.5;
}
double zero_both_sides(double x) { return -10.0 * (x - 0.5) * (x - 0.5) + 1.0; }

SolverManager& manager() {
    static SolverManager m;
    return m;
}

// The default manager's solvers, and "quasi-mcp-hip-quality" beside them: an opt-in solver (an embedding application
// registers it with SolverManager::add), so qmcp_host_solver_names keeps listing the default manager only.
constexpr const char* kQualitySolverName = "quasi-mcp-hip-quality";
qmcp::Solver* resolve(const char* name) {
    if (manager().contains(name)) return &manager().get(name);
    if (std::strcmp(name, kQualitySolverName) == 0) {
        static qmcp::QuasiMcpHipQualitySolver quality;
        return &quality;
    }
    return nullptr;
}

// amplicon_mode: 0 IGNORE, 1 FILTER, 2 GRADE
bam_api::AmpliconBehaviour amplicon_behaviour(int amplicon_mode) {
    return amplicon_mode == 1 ? bam_api::AmpliconBehaviour::FILTER
         : amplicon_mode == 2 ? bam_api::AmpliconBehaviour::GRADE : bam_api::AmpliconBehaviour::IGNORE;
}
// amplicon_mode -1: the solver decides, as App::execute does (src/app.cpp:120-128) -- GRADE for a solver that uses the
// reads' qualities, FILTER for every other
bam_api::AmpliconBehaviour amplicon_behaviour(int amplicon_mode, qmcp::Solver& solver) {
    return amplicon_behaviour(amplicon_mode >= 0 ? amplicon_mode : solver.uses_quality_of_reads() ? 2 : 1);
}

void copy_err(const std::string& msg, char* err, std::size_t cap) {
    if (err && cap) {
        std::strncpy(err, msg.c_str(), cap - 1);
        err[cap - 1] = 0;
    }
}

// Nothing is thrown through the C boundary: -3 out of memory, -4 with the message in err when BamApi or an entry refuses
template <class Body>
std::int64_t guarded(char* err, std::size_t err_cap, Body body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// "strand" / "read_group" -> BamApiConfig::stratify_by; anything else is refused
bam_api::Stratify stratify_from_name(const char* name) {
    const std::string s = name ? name : "";
    if (s == "strand") return bam_api::Stratify::STRAND;
    if (s == "read_group") return bam_api::Stratify::READ_GROUP;
    throw std::invalid_argument("stratify must be \"strand\" or \"read_group\", not \"" + s + "\"");
}

// ---- what the qmcp_host_read_bam* entries take and hand out
bool given(const char* s) { return s && s[0]; }

bam_api::BamApiConfig ingest_config(const char* bed, const char* tsv, int amplicon_mode, std::uint32_t min_len,
                                    std::uint32_t min_mapq) {
    bam_api::BamApiConfig cfg;
    if (given(bed)) cfg.bed_filepath = bed;
    if (given(tsv)) cfg.tsv_filepath = tsv;
    cfg.amplicon_behaviour = amplicon_behaviour(amplicon_mode);
    cfg.min_seq_length = min_len;
    cfg.min_mapq = min_mapq;
    return cfg;
}

// the ingest's by-products: the filtered-out ids (cap_f entries) and every reference's length (ref_cap entries;
// ref_lengths NULL: not wanted).  false when a capacity is too small.
struct IngestOut {
    std::uint64_t cap_f;
    std::uint64_t* filtered_out;
    std::uint64_t* n_filtered_out;
    std::uint64_t ref_cap;
    std::uint32_t* ref_lengths;
    std::uint64_t* n_refs;
};
bool copy_out_ingest(const std::vector<bam_api::BAMReadId>& filtered, const std::vector<std::uint32_t>& lengths,
                     const IngestOut& o) {
    if (filtered.size() > o.cap_f || (o.ref_lengths && lengths.size() > o.ref_cap)) return false;
    *o.n_filtered_out = filtered.size();
    for (std::size_t i = 0; i < filtered.size(); ++i) o.filtered_out[i] = filtered[i];
    if (o.ref_lengths) {
        *o.n_refs = lengths.size();
        for (std::size_t k = 0; k < lengths.size(); ++k) o.ref_lengths[k] = lengths[k];
    }
    return true;
}

// the SoA columns of get_paired_reads_soa() (cap entries each; contig_ids / strata NULL: not wanted -- reads without
// a contig column get contig 0) and the ingest's by-products.  Returns the number of reads, -2 when a capacity is too small.
struct ReadsOut {
    std::uint64_t cap;
    std::uint64_t* bam_ids;
    std::uint32_t *starts, *ends, *qualities, *seq_lengths;
    std::uint8_t* is_first;
    std::uint32_t *contig_ids, *strata;
};
std::int64_t copy_out_reads(bam_api::BamApi& api, const ReadsOut& c, const IngestOut& o) {
    const bam_api::SOAPairedReads& r = api.get_paired_reads_soa();
    const std::uint64_t n = r.ids.size();
    if (n > c.cap || !copy_out_ingest(api.get_filtered_out_reads(), r.contig_lengths, o)) return -2;
    for (std::uint64_t i = 0; i < n; ++i) {
        c.bam_ids[i] = r.ids[i]; c.starts[i] = (std::uint32_t)r.start_inds[i]; c.ends[i] = (std::uint32_t)r.end_inds[i];
        c.qualities[i] = r.qualities[i]; c.seq_lengths[i] = r.seq_lengths[i]; c.is_first[i] = r.is_first_reads[i] ? 1 : 0;
        if (c.contig_ids) c.contig_ids[i] = r.contig_ids.size() == n ? r.contig_ids[i] : 0u;
        if (c.strata) c.strata[i] = r.strata[i];
    }
    return (std::int64_t)n;
}

// ---- the file-to-file flow behind qmcp_host_downsample_bam

// The request as a BamApiConfig, every knob handed on as given so that BamApiConfig refuses the combinations it
// refuses.  The only place that knows the request's "not given": NULL or "" for a path, NULL for an array, a negative
// budget_fraction (a NaN is handed on, to be refused).
bam_api::BamApiConfig config_of(const qmcp_host_downsample_request& q, qmcp::Solver& solver) {
    bam_api::BamApiConfig cfg = ingest_config(q.bed, q.tsv, 0, q.min_len, q.min_mapq);
    cfg.amplicon_behaviour = amplicon_behaviour(q.amplicon_mode, solver);
    cfg.per_reference = q.per_reference != 0;
    cfg.amplicons_by_reference = q.amplicons_by_reference != 0;
    if (given(q.targets)) cfg.targets_filepath = q.targets;
    cfg.target_padding = q.target_padding;
    cfg.keep_off_target = q.keep_off_target != 0;
    if (given(q.report)) cfg.depth_report_filepath = q.report;
    cfg.depth_report_bins = q.report_bins;
    if (given(q.track)) cfg.depth_track_filepath = q.track;
    if (given(q.track_channel)) cfg.depth_track_channel = q.track_channel;
    cfg.depth_track_cap = q.track_cap;
    if (q.ladder_levels) cfg.coverage_ladder.assign(q.ladder_levels, q.ladder_levels + q.n_ladder_levels);
    if (given(q.stratify)) cfg.stratify_by = stratify_from_name(q.stratify);
    cfg.dedup = q.dedup != 0;
    cfg.start_cap = q.start_cap;
    cfg.start_cap_by_strand = q.start_cap_by_strand != 0;
    cfg.primer_clip = q.primer_clip != 0;
    cfg.per_amplicon = q.per_amplicon != 0;
    if (given(q.amplicon_report)) cfg.amplicon_report_filepath = q.amplicon_report;
    if (q.mapq_tiers) cfg.mapq_tiers.assign(q.mapq_tiers, q.mapq_tiers + q.n_mapq_tiers);
    cfg.pair_aware = q.pair_aware != 0;
    if (q.pair_stages) cfg.pair_stages.assign(q.pair_stages, q.pair_stages + q.n_pair_stages);
    cfg.template_aware = q.template_aware != 0;
    cfg.split_spliced = q.split_spliced != 0;
    cfg.include_secondary = q.include_secondary != 0;
    cfg.fragment_depth = q.fragment_depth != 0;
    if (q.template_stages) cfg.template_stages.assign(q.template_stages, q.template_stages + q.n_template_stages);
    cfg.ceiling = q.ceiling != 0;
    if (q.has_budget_reads) cfg.budget_reads = q.budget_reads;
    if (q.budget_fraction >= 0.0 || q.budget_fraction != q.budget_fraction) cfg.budget_fraction = q.budget_fraction;
    if (q.has_mean_depth) cfg.mean_depth = q.mean_depth;
    if (q.has_budget_bases) cfg.budget_bases = q.budget_bases;
    if (given(q.mean_depth_targets)) cfg.mean_depth_targets_filepath = q.mean_depth_targets;
    if (q.has_replicates) {
        cfg.replicates = std::vector<std::uint32_t>();
        if (q.replicates_further) cfg.replicates->assign(q.replicates_further, q.replicates_further + q.n_replicates_further);
    }
    if (q.has_thresholds) {
        cfg.thresholds_lo = q.thresholds_lo;
        cfg.thresholds_hi = q.thresholds_hi;
    }
    if (given(q.thresholds_tag)) cfg.thresholds_tag = q.thresholds_tag;
    if (q.has_proportion)
        cfg.proportion = bam_api::BamApiConfig::Proportion{q.proportion_num, q.proportion_den, q.proportion_floor};
    return cfg;
}

// Which solve a request asks for: the first of these that it switches on.  PLAIN is Solver::solve -- with targets,
// amplicons, a depth report or a depth track, which any solver takes; every other mode is a method of the hip solver.
enum class Mode { TIERS, AMPLICONS, START_CAP, THRESHOLDS, MEAN_DEPTH, PROPORTIONAL, REPLICATES, BUDGET, CEILING, TEMPLATES, PAIRS, PROFILE, DEDUP, STRATIFIED, LADDER, PLAIN };
Mode mode_of(const qmcp_host_downsample_request& q, const bam_api::BamApiConfig& cfg) {
    if (!cfg.mapq_tiers.empty() || given(q.tiers_report)) return Mode::TIERS;
    if (cfg.primer_clip || cfg.per_amplicon || !cfg.amplicon_report_filepath.empty()) return Mode::AMPLICONS;
    if (cfg.start_cap || cfg.start_cap_by_strand || given(q.start_cap_report)) return Mode::START_CAP;
    if (cfg.thresholds_hi || given(q.thresholds_tag) || given(q.thresholds_report)) return Mode::THRESHOLDS;
    if (cfg.mean_depth || cfg.budget_bases || given(q.mean_depth_targets) || given(q.mean_depth_report))
        return Mode::MEAN_DEPTH;
    if (cfg.proportion || given(q.proportional_report)) return Mode::PROPORTIONAL;
    if (cfg.replicates) return Mode::REPLICATES;
    if (cfg.budget_reads || cfg.budget_fraction || given(q.budget_report)) return Mode::BUDGET;
    if (cfg.ceiling) return Mode::CEILING;
    if (cfg.template_aware) return Mode::TEMPLATES;
    if (cfg.pair_aware) return Mode::PAIRS;
    if (q.has_regions) return Mode::PROFILE;
    if (cfg.dedup) return Mode::DEDUP;
    if (cfg.stratify_by != bam_api::Stratify::NONE) return Mode::STRATIFIED;
    if (!cfg.coverage_ladder.empty() || given(q.ladder_template)) return Mode::LADDER;
    return Mode::PLAIN;
}

// a mode's words in the refusals: "<refuses> take ..." / "<refuses> go together with ...", "this solver has no <noun>"
struct ModeWords {
    std::string refuses, noun;
};
ModeWords words_of(Mode mode) {
    switch (mode) {
        case Mode::TIERS: return {"tiered downsampling does not", "tiered downsampling"};
        case Mode::AMPLICONS: return {"amplicon-aware downsampling does not", "amplicon-aware downsampling"};
        case Mode::START_CAP: return {"a start cap does not", "start cap"};
        case Mode::THRESHOLDS: return {"coverage thresholds do not", "coverage thresholds"};
        case Mode::MEAN_DEPTH: return {"mean-depth downsampling does not", "mean-depth downsampling"};
        case Mode::PROPORTIONAL: return {"proportional downsampling does not", "proportional downsampling"};
        case Mode::REPLICATES: return {"disjoint replicates do not", "disjoint replicates"};
        case Mode::BUDGET: return {"budget downsampling does not", "budget downsampling"};
        case Mode::CEILING: return {"ceiling downsampling does not", "ceiling downsampling"};
        case Mode::TEMPLATES: return {"template-aware downsampling does not", "template-aware downsampling"};
        case Mode::PAIRS: return {"pair-aware downsampling does not", "pair-aware downsampling"};
        case Mode::PROFILE: return {"a coverage profile does not", "coverage profile"};
        case Mode::DEDUP: return {"duplicate-aware downsampling does not", "duplicate-aware downsampling"};
        case Mode::STRATIFIED: return {"stratified downsampling does not", "stratified downsampling"};
        case Mode::LADDER: return {"a coverage ladder does not", "coverage ladder"};
        case Mode::PLAIN: break;
    }
    return {};
}

// What an entry refuses from the request alone, before the ingest (BamApiConfig's own rules follow in BamApi's
// constructor).  hip: the solver as the hip solver, NULL for another.
void refuse_before_ingest(const qmcp_host_downsample_request& q, const bam_api::BamApiConfig& cfg, Mode mode,
                          qmcp::Solver& solver, const qmcp::QuasiMcpHipSolver* hip, std::uint64_t written_cap) {
    const auto refuse = [](const std::string& why) { throw std::invalid_argument(why); };
    const ModeWords words = words_of(mode);
    if (q.in_path == nullptr || q.out_path == nullptr) refuse("a request needs in_path and out_path");
    const std::string ladder_template = q.ladder_template ? q.ladder_template : "";
    const std::string replicates_template = q.replicates_template ? q.replicates_template : "";
    if (mode == Mode::BUDGET && !cfg.budget_reads && !cfg.budget_fraction)
        refuse("budget downsampling needs budget_reads or budget_fraction");
    if (mode == Mode::MEAN_DEPTH && !cfg.mean_depth && !cfg.budget_bases)
        refuse("mean-depth downsampling needs mean_depth or budget_bases");
    if (mode == Mode::TIERS && cfg.mapq_tiers.empty()) refuse("tiers_report needs mapq_tiers");
    if (mode == Mode::START_CAP && !cfg.start_cap) refuse("start_cap_by_strand and start_cap_report need start_cap");
    if (mode == Mode::START_CAP && q.has_regions) refuse("a start cap does not go together with a coverage profile");
    if (mode == Mode::THRESHOLDS && !cfg.thresholds_hi) refuse("thresholds_tag and thresholds_report need thresholds");
    if (mode == Mode::PROPORTIONAL && !cfg.proportion) refuse("proportional downsampling needs a proportion");
    if (mode == Mode::LADDER && cfg.coverage_ladder.empty()) refuse("a coverage ladder needs at least one level");
    if (mode == Mode::LADDER && ladder_template.find("{M}") == std::string::npos)
        refuse("the ladder's output template has no {M}");
    if (mode == Mode::REPLICATES && !cfg.replicates->empty() && replicates_template.find("{R}") == std::string::npos)
        refuse("the replicates' output template has no {R}");
    if (mode == Mode::PROFILE) {  // (BamApiConfig knows no coverage profile, so its rules stand here)
        if (!cfg.per_reference) refuse("a coverage profile needs per_reference");
        if (!cfg.targets_filepath.empty()) refuse("a coverage profile does not go together with targets");
        if (!cfg.depth_report_filepath.empty()) refuse("a coverage profile does not go together with a depth report");
        if (!cfg.coverage_ladder.empty()) refuse("a coverage profile does not go together with a coverage ladder");
        if (cfg.stratify_by != bam_api::Stratify::NONE) refuse("a coverage profile does not go together with stratify_by");
        if (cfg.dedup) refuse("a coverage profile does not go together with dedup");
        if (!cfg.depth_track_filepath.empty()) refuse("a coverage profile does not go together with a depth track");
        if (!cfg.bed_filepath.empty() || !cfg.tsv_filepath.empty() || cfg.amplicons_by_reference)
            refuse("a coverage profile does not take amplicon files");
    }
    if (given(q.fragment_report) && !cfg.fragment_depth) refuse("a fragment report needs fragment_depth");
    if (q.has_regions &&
        (mode == Mode::PAIRS || mode == Mode::BUDGET || mode == Mode::REPLICATES || mode == Mode::PROPORTIONAL ||
         mode == Mode::MEAN_DEPTH || mode == Mode::THRESHOLDS || mode == Mode::AMPLICONS || mode == Mode::TIERS))
        refuse(words.refuses + " go together with a coverage profile");
    if (mode != Mode::PLAIN && solver.uses_quality_of_reads()) refuse(words.refuses + " take a solver that grades by quality");
    if (mode != Mode::PLAIN && hip == nullptr) refuse("this solver has no " + words.noun);
    if (hip == nullptr && !cfg.depth_report_filepath.empty()) refuse("this solver has no depth report");
    if (hip == nullptr && !cfg.depth_track_filepath.empty()) refuse("this solver has no depth track");
    if (q.has_regions) {
        const std::string table = mode == Mode::TEMPLATES ? "a cap table" : "a coverage profile";
        if (q.region_offsets == nullptr) refuse(table + " needs its region offsets");
        if (q.region_offsets[q.n_refs] && (!q.region_starts || !q.region_ends || !q.region_caps))
            refuse(table + " with regions needs their starts, ends and caps");
    }
    const std::size_t files = mode == Mode::LADDER       ? 1 + cfg.coverage_ladder.size()
                              : mode == Mode::REPLICATES ? 1 + cfg.replicates->size() : 1;
    if (files > 1 && written_cap < files) refuse("written_out is too short for this request's output files");
}

// ---- the reports, each written after the output; false when the file cannot be written
// one line per stratum: name, cap, reads, kept, mean depth before and after (bases / the sum of the reference lengths)
// of the solve's own kept set (before mate completion)
bool write_strata_report(const char* path, const bam_api::SOAPairedReads& r, const qmcp::QuasiMcpHipSolver& hip) {
    double positions = 0;
    for (std::uint32_t l : r.contig_lengths) positions += l;
    std::FILE* f = std::fopen(path, "w");
    if (f == nullptr) return false;
    std::fprintf(f, "#stratum\tcap\treads\tkept\tmean_depth_in\tmean_depth_kept\n");
    for (std::size_t s = 0; s < r.stratum_names.size(); ++s) {
        const qmcp_hip_stratum_row& row = hip.last_stratum_rows()[s];
        std::fprintf(f, "%s\t%u\t%llu\t%llu\t%.6f\t%.6f\n", r.stratum_names[s].c_str(), hip.last_stratum_caps()[s],
                     (unsigned long long)row.n_reads, (unsigned long long)row.n_kept,
                     positions > 0 ? (double)row.bases_in / positions : 0.0,
                     positions > 0 ? (double)row.bases_kept / positions : 0.0);
    }
    return std::fclose(f) == 0;
}

// one line per tier: its MAPQ band, reads, kept, mean depth before and after (bases / the sum of the reference lengths) of
// the solve's own kept set, demand and asked positions; then the records written and how many of them find_pairs added
bool write_tiers_report(const char* path, const bam_api::SOAPairedReads& r, const std::vector<std::uint32_t>& bands,
                        const qmcp::QuasiMcpHipSolver& hip, std::int64_t written, std::uint64_t mates_added) {
    double positions = 0;
    for (std::uint32_t l : r.contig_lengths) positions += l;
    if (positions <= 0) positions = 1;
    std::FILE* f = std::fopen(path, "w");
    if (f == nullptr) return false;
    std::fprintf(f, "#tier\tband\treads\tkept\tmean_depth_in\tmean_depth_kept\tdemand\tasked_positions\n");
    for (std::size_t t = 0; t < bands.size(); ++t) {
        const qmcp_hip_tier_row& row = hip.last_tier_rows()[t];
        std::fprintf(f, "%zu\tmapq>=%u\t%llu\t%llu\t%.6f\t%.6f\t%llu\t%llu\n", t, bands[t], (unsigned long long)row.n_reads,
                     (unsigned long long)row.n_kept, (double)row.bases_in / positions, (double)row.bases_kept / positions,
                     (unsigned long long)row.demand, (unsigned long long)row.asked_positions);
    }
    std::fprintf(f, "records_written\t%lld\nmates_added\t%llu\n", (long long)written, (unsigned long long)mates_added);
    return std::fclose(f) == 0;
}

// the statistics, then one size<TAB>families line per bin of the family-size histogram
constexpr std::uint32_t kDedupBins = 64;
bool write_dedup_report(const char* path, const qmcp::QuasiMcpHipSolver& hip) {
    const qmcp_hip_dedup_stats& ds = hip.last_dedup_stats();
    std::FILE* f = std::fopen(path, "w");
    if (f == nullptr) return false;
    std::fprintf(f, "#stat\tvalue\n");
    std::fprintf(f, "units\t%llu\nfamilies\t%llu\nduplicate_units\t%llu\nlargest_family\t%llu\nreads_survived\t%llu\n",
                 (unsigned long long)ds.units, (unsigned long long)ds.families, (unsigned long long)ds.duplicate_units,
                 (unsigned long long)ds.largest_family, (unsigned long long)ds.reads_survived);
    std::fprintf(f, "#size\tfamilies\n");
    for (std::uint32_t b = 0; b < kDedupBins; ++b)
        std::fprintf(f, "%u\t%llu\n", b + 1, (unsigned long long)hip.last_dedup_hist()[b]);
    return std::fclose(f) == 0;
}

// the statistics and the records written, then one size<TAB>cells line per bin of the cell-size histogram
constexpr std::uint32_t kStartCapBins = 64;
bool write_start_cap_report(const char* path, const qmcp::QuasiMcpHipSolver& hip, std::int64_t written) {
    const qmcp_hip_start_cap_stats& cs = hip.last_start_cap_stats();
    std::FILE* f = std::fopen(path, "w");
    if (f == nullptr) return false;
    std::fprintf(f, "#stat\tvalue\n");
    std::fprintf(f, "cap\t%u\nreads_placed\t%llu\ncells\t%llu\ncells_over_cap\t%llu\nreads_capped\t%llu\n"
                    "largest_cell\t%llu\nreads_survived\t%llu\ncells_kept\t%llu\nlargest_kept_cell\t%llu\n"
                    "short_positions\t%llu\nshort_bases\t%llu\nrecords_written\t%lld\n",
                 cs.cap, (unsigned long long)cs.reads_placed, (unsigned long long)cs.cells,
                 (unsigned long long)cs.cells_over_cap, (unsigned long long)cs.reads_capped,
                 (unsigned long long)cs.largest_cell, (unsigned long long)cs.reads_survived,
                 (unsigned long long)cs.cells_kept, (unsigned long long)cs.largest_kept_cell,
                 (unsigned long long)cs.short_positions, (unsigned long long)cs.short_bases, (long long)written);
    std::fprintf(f, "#size\tcells\n");
    for (std::uint32_t b = 0; b < kStartCapBins; ++b)
        std::fprintf(f, "%u\t%llu\n", b + 1, (unsigned long long)hip.last_start_cap_hist()[b]);
    return std::fclose(f) == 0;
}

// One line per amplicon, in the order of the references and within a reference of the BED / TSV: chrom, amplicon start
// and end, the insert the solve used (the amplicon itself without primer_clip), left primer, units assigned, reads kept
// (of the written set), minimum and mean depth over the insert before and after, positions short of min(before, M)
bool write_amplicon_report(const std::filesystem::path& path, const bam_api::ReferenceAmpliconSet& set,
                           const std::vector<std::string>& names, const qmcp::QuasiMcpHipSolver& hip,
                           const std::vector<bam_api::ReadIndex>& kept) {
    const std::vector<std::uint32_t>& labels = hip.last_amplicon_labels();
    const std::vector<qmcp_hip_depth_row>& rows = hip.last_amplicon_rows();
    std::vector<std::uint64_t> units(rows.size(), 0), reads_kept(rows.size(), 0);
    for (std::uint32_t l : labels)
        if (l != QMCP_NO_AMPLICON) units[l]++;
    for (bam_api::ReadIndex i : kept)
        if (labels[i / 2] != QMCP_NO_AMPLICON) reads_kept[labels[i / 2]]++;
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (f == nullptr) return false;
    std::fprintf(f, "#chrom\tamplicon_start\tamplicon_end\tinsert_start\tinsert_end\tleft_primer\tunits\treads_kept\t"
                    "min_depth_in\tmean_depth_in\tmin_depth_kept\tmean_depth_kept\tdeficit_positions\n");
    for (std::size_t c = 0; c < set.n_references(); ++c)
        for (std::uint32_t k = set.offsets[c]; k < set.offsets[c + 1]; ++k) {
            const qmcp_hip_depth_row& r = rows[k];
            const double positions = (double)r.positions;
            std::fprintf(f, "%s\t%llu\t%llu\t%u\t%u\t%s\t%llu\t%llu\t%u\t%.6f\t%u\t%.6f\t%llu\n", names[c].c_str(),
                         (unsigned long long)set.starts[k], (unsigned long long)set.ends[k], r.start, r.end,
                         set.left_names[k].c_str(), (unsigned long long)units[k], (unsigned long long)reads_kept[k],
                         r.min_in, (double)r.sum_in / positions, r.min_kept, (double)r.sum_kept / positions,
                         (unsigned long long)r.deficit_positions);
        }
    return std::fclose(f) == 0;
}

// stat<TAB>value: the qmcp_hip_ceiling_stats and the records written
bool write_ceiling_report(const char* path, const qmcp_hip_ceiling_stats& cs, std::int64_t written) {
    std::FILE* f = std::fopen(path, "w");
    if (f == nullptr) return false;
    std::fprintf(f, "#stat\tvalue\n");
    std::fprintf(f, "reads_placed\t%llu\nreads_dropped\t%llu\nmates_dropped\t%llu\nover_positions\t%llu\n"
                    "over_bases\t%llu\nshort_positions\t%llu\nshort_bases\t%llu\nexcess_positions\t%llu\n",
                 (unsigned long long)cs.reads_placed, (unsigned long long)cs.reads_dropped,
                 (unsigned long long)cs.mates_dropped, (unsigned long long)cs.over_positions,
                 (unsigned long long)cs.over_bases, (unsigned long long)cs.short_positions,
                 (unsigned long long)cs.short_bases, (unsigned long long)cs.excess_positions);
    std::fprintf(f, "max_kept_depth\t%u\nregions_in\t%u\nregions_used\t%u\nrecords_written\t%u\n", cs.max_kept_depth,
                 cs.regions_in, cs.regions_used, (unsigned)written);
    return std::fclose(f) == 0;
}

// stat<TAB>value: the qmcp_hip_fragment_stats and the records written
bool write_fragment_report(const char* path, const qmcp_hip_fragment_stats& fs, std::int64_t written) {
    std::FILE* f = std::fopen(path, "w");
    if (f == nullptr) return false;
    std::fprintf(f, "#stat\tvalue\n");
    std::fprintf(f, "segments_placed\t%llu\nsegments_clipped\t%llu\nsegments_emptied\t%llu\nbases_in\t%llu\n"
                    "bases_removed\t%llu\ntemplates_overlapping\t%llu\n",
                 (unsigned long long)fs.n_placed, (unsigned long long)fs.n_clipped, (unsigned long long)fs.n_emptied,
                 (unsigned long long)fs.bases_in, (unsigned long long)fs.bases_removed,
                 (unsigned long long)fs.n_templates_overlapping);
    std::fprintf(f, "max_group\t%u\nms_clip\t%.6g\nrecords_written\t%u\n", fs.max_group, (double)fs.ms_clip,
                 (unsigned)written);
    return std::fclose(f) == 0;
}

// stat<TAB>value: the qmcp_hip_proportional_stats and the records written
bool write_proportional_report(const char* path, const qmcp_hip_proportional_stats& ps, std::int64_t written) {
    std::FILE* f = std::fopen(path, "w");
    if (f == nullptr) return false;
    std::fprintf(f, "#stat\tvalue\n");
    std::fprintf(f, "reads_placed\t%llu\nbases_in\t%llu\nbases_kept\t%llu\ndemand\t%llu\nwhole_positions\t%llu\n"
                    "floor_positions\t%llu\ncapped_positions\t%llu\n",
                 (unsigned long long)ps.reads_placed, (unsigned long long)ps.bases_in, (unsigned long long)ps.bases_kept,
                 (unsigned long long)ps.demand, (unsigned long long)ps.whole_positions,
                 (unsigned long long)ps.floor_positions, (unsigned long long)ps.capped_positions);
    std::fprintf(f, "max_depth\t%u\nmax_need\t%u\nnum\t%u\nden\t%u\nfloor\t%u\nplain_route\t%u\nrecords_written\t%u\n",
                 ps.max_depth, ps.max_need, ps.num, ps.den, ps.floor, ps.plain_route, (unsigned)written);
    return std::fclose(f) == 0;
}

// stat<TAB>value: the qmcp_hip_thresholds_stats and the records written, then one M<TAB>reads line per coverage of the range
bool write_thresholds_report(const char* path, const qmcp_hip_thresholds_stats& ts, const std::vector<std::uint64_t>& counts,
                             std::int64_t written) {
    std::FILE* f = std::fopen(path, "w");
    if (f == nullptr) return false;
    std::fprintf(f, "#stat\tvalue\n");
    std::fprintf(f, "reads_placed\t%llu\nn_kept\t%llu\nnesting_violations\t%llu\n", (unsigned long long)ts.reads_placed,
                 (unsigned long long)ts.n_kept, (unsigned long long)ts.nesting_violations);
    std::fprintf(f, "coverage_lo\t%u\ncoverage_hi\t%u\ntop\t%u\nsolves\t%u\nsaturated\t%u\ncount_entries\t%u\n"
                    "ms_thresholds\t%.6g\nms_solves\t%.6g\nrecords_written\t%u\n",
                 ts.coverage_lo, ts.coverage_hi, ts.top, ts.solves, ts.saturated, ts.count_entries, (double)ts.ms_thresholds,
                 (double)ts.ms_solves, (unsigned)written);
    std::fprintf(f, "#M\treads\n");
    for (std::size_t k = 0; k < counts.size(); ++k)
        std::fprintf(f, "%zu\t%llu\n", (std::size_t)ts.coverage_lo + k, (unsigned long long)counts[k]);
    return std::fclose(f) == 0;
}

// stat<TAB>value: the qmcp_hip_budget_stats and the records written, then one M<TAB>bases line per entry of the curve
bool write_budget_report(const char* path, const qmcp_hip_budget_stats& bs, const std::vector<std::uint64_t>& curve,
                         std::int64_t written) {
    std::FILE* f = std::fopen(path, "w");
    if (f == nullptr) return false;
    std::fprintf(f, "#stat\tvalue\n");
    std::fprintf(f, "budget\t%llu\nreads_placed\t%llu\nn_kept\t%llu\nkept_above\t%llu\nbound_above\t%llu\n"
                    "total_bases\t%llu\n",
                 (unsigned long long)bs.budget, (unsigned long long)bs.reads_placed, (unsigned long long)bs.n_kept,
                 (unsigned long long)bs.kept_above, (unsigned long long)bs.bound_above, (unsigned long long)bs.total_bases);
    std::fprintf(f, "coverage\t%u\nmax_depth\t%u\ntop\t%u\nprobes\t%u\ncurve_entries\t%u\nsaturated\t%u\n"
                    "ms_budget\t%.6g\nms_solves\t%.6g\nrecords_written\t%u\n",
                 bs.coverage, bs.max_depth, bs.top, bs.probes, bs.curve_entries, bs.saturated, (double)bs.ms_budget,
                 (double)bs.ms_solves, (unsigned)written);
    std::fprintf(f, "#M\tbases\n");
    for (std::size_t m = 0; m < curve.size(); ++m) std::fprintf(f, "%zu\t%llu\n", m, (unsigned long long)curve[m]);
    return std::fclose(f) == 0;
}

// stat<TAB>value: the qmcp_hip_mean_depth_stats, the records written and the two means over the regions' positions, then
// one M<TAB>bases line per entry of the curve S_R
bool write_mean_depth_report(const char* path, const qmcp_hip_mean_depth_stats& ms, const std::vector<std::uint64_t>& curve,
                             std::int64_t written) {
    std::FILE* f = std::fopen(path, "w");
    if (f == nullptr) return false;
    std::fprintf(f, "#stat\tvalue\n");
    std::fprintf(f, "budget\t%llu\npositions\t%llu\nreads_placed\t%llu\nn_kept\t%llu\nkept_bases\t%llu\n"
                    "bases_above\t%llu\nbound_above\t%llu\ntotal_bases\t%llu\n",
                 (unsigned long long)ms.budget, (unsigned long long)ms.positions, (unsigned long long)ms.reads_placed,
                 (unsigned long long)ms.n_kept, (unsigned long long)ms.kept_bases, (unsigned long long)ms.bases_above,
                 (unsigned long long)ms.bound_above, (unsigned long long)ms.total_bases);
    std::fprintf(f, "coverage\t%u\nmax_depth\t%u\ntop\t%u\nprobes\t%u\ncurve_entries\t%u\nsaturated\t%u\n"
                    "regions_in\t%u\nregions_used\t%u\nms_mean_depth\t%.6g\nms_solves\t%.6g\nrecords_written\t%u\n",
                 ms.coverage, ms.max_depth, ms.top, ms.probes, ms.curve_entries, ms.saturated, ms.regions_in,
                 ms.regions_used, (double)ms.ms_mean_depth, (double)ms.ms_solves, (unsigned)written);
    const double positions = (double)ms.positions;
    std::fprintf(f, "mean_depth_in\t%.6f\nmean_depth_kept\t%.6f\n", positions > 0 ? (double)ms.total_bases / positions : 0.0,
                 positions > 0 ? (double)ms.kept_bases / positions : 0.0);
    std::fprintf(f, "#M\tbases\n");
    for (std::size_t m = 0; m < curve.size(); ++m) std::fprintf(f, "%zu\t%llu\n", m, (unsigned long long)curve[m]);
    return std::fclose(f) == 0;
}

// one line per replicate -- coverage, offered, kept, mates, short_positions, short_bases, records_written -- and n_full
bool write_replicates_report(const char* path, const qmcp_hip_replicates_stats& rs, std::uint32_t max_coverage,
                             const std::vector<std::uint32_t>& further, const std::vector<std::int64_t>& written) {
    std::FILE* f = std::fopen(path, "w");
    if (f == nullptr) return false;
    std::fprintf(f, "#replicate\tcoverage\toffered\tkept\tmates\tshort_positions\tshort_bases\trecords_written\n");
    for (std::size_t r = 0; r < written.size(); ++r)
        std::fprintf(f, "%zu\t%u\t%llu\t%llu\t%llu\t%llu\t%llu\t%u\n", r + 1, r == 0 ? max_coverage : further[r - 1],
                     (unsigned long long)rs.n_offered[r], (unsigned long long)rs.n_kept[r], (unsigned long long)rs.n_mates[r],
                     (unsigned long long)rs.short_positions[r], (unsigned long long)rs.short_bases[r], (unsigned)written[r]);
    std::fprintf(f, "n_full\t%u\n", rs.n_full);
    return std::fclose(f) == 0;
}

// The depth report and the depth track of BamApiConfig: the reads the solve saw against the final kept set (after
// find_pairs), with M = max_coverage and the call's targets and padding -- the report as TSV, the track as bedGraph with
// both depths compared and zero positions kept.  false with the reason in *why.
bool write_depth_report(qmcp::QuasiMcpHipSolver& hip, std::uint32_t max_coverage, bam_api::BamApi& api,
                        const std::vector<bam_api::ReadIndex>& kept, const std::vector<std::string>& names, std::string* why) {
    qmcp::DepthReport report;
    hip.depth_report(max_coverage, api, kept, api.depth_report_bins(), report);
    if (qmcp::write_depth_report_tsv(api.depth_report_filepath(), report, names)) return true;
    *why = "could not write " + api.depth_report_filepath().string();
    return false;
}
bool write_depth_track(qmcp::QuasiMcpHipSolver& hip, std::uint32_t max_coverage, bam_api::BamApi& api,
                       const std::vector<bam_api::ReadIndex>& kept, const std::vector<std::string>& names, std::string* why) {
    qmcp::DepthTrack track;
    hip.depth_track(max_coverage, api, kept, QMCP_TRACK_IN | QMCP_TRACK_KEPT, api.depth_track_cap(), track);
    if (qmcp::write_depth_track_bedgraph(api.depth_track_filepath(), track, names, api.depth_track_channel())) return true;
    *why = "could not write " + api.depth_track_filepath().string();
    return false;
}

// Everything qmcp_host_downsample_bam does (include/qmcp_host_request.h) but the exception mapping, in the order:
// solver, configuration, refusals, ingest, solve, output file(s), filtered-out file, stats, reports.
std::int64_t downsample(const qmcp_host_downsample_request& q, std::int64_t* written_out, std::uint64_t written_cap,
                        qmcp_hip_ceiling_stats* ceiling_stats, qmcp_hip_budget_stats* budget_stats,
                        qmcp_hip_replicates_stats* replicates_stats, qmcp_hip_template_stats* template_stats,
                        qmcp_hip_template_profile_stats* template_profile_stats, char* err, std::size_t err_cap) {
    if (q.struct_size != sizeof(q)) throw std::invalid_argument("the request has another struct_size than this library's");
    qmcp::Solver* solver = q.solver_name ? resolve(q.solver_name) : nullptr;
    if (solver == nullptr) return -1;
    bam_api::BamApiConfig cfg = config_of(q, *solver);
    const Mode mode = mode_of(q, cfg);
    auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(solver);
    refuse_before_ingest(q, cfg, mode, *solver, hip, written_out ? written_cap : UINT64_MAX);
    const std::uint32_t M = q.max_coverage;
    std::vector<std::uint32_t> offsets, starts, ends, caps;  // the region table; all empty: none
    if (q.has_regions) {
        const std::uint32_t n_regions = q.region_offsets[q.n_refs];
        offsets.assign(q.region_offsets, q.region_offsets + q.n_refs + 1);
        starts.assign(q.region_starts, q.region_starts + n_regions);
        ends.assign(q.region_ends, q.region_ends + n_regions);
        caps.assign(q.region_caps, q.region_caps + n_regions);
    }

    bam_api::BamApi api(q.in_path, cfg);

    // solve, and write every kept set: `written` gets one record count per output file, out_path's first.  Pairs are
    // completed by find_pairs where the solve does not leave whole pairs itself -- and never where that would put
    // depth, reads or bases back (ceiling, budget, mean depth) or copy a record into two files (replicates).
    std::vector<std::int64_t> written;
    std::vector<bam_api::ReadIndex> kept;  // the last kept set as written (the depth report and track describe it)
    const auto write_reads = [&](const qmcp::Solution& solution, bool complete_pairs, const std::string& path) {
        kept = complete_pairs ? api.find_pairs(solution) : solution;
        written.push_back(api.write_paired_reads(path, kept));
    };
    const auto path_from = [](const char* path_template, const char* token, std::uint64_t value) {
        std::string path = path_template;
        return path.replace(path.find(token), 3, std::to_string(value));
    };
    std::uint64_t mates_added = 0;  // tiered downsampling: the reads find_pairs put next to the solve's own
    switch (mode) {
        case Mode::TIERS: {
            const std::unique_ptr<qmcp::Solution> solution = hip->solve_tiers(M, api);
            write_reads(*solution, true, q.out_path);
            mates_added = kept.size() - solution->size();
            break;
        }
        case Mode::PLAIN:
        case Mode::STRATIFIED: write_reads(*solver->solve(M, api), true, q.out_path); break;
        case Mode::DEDUP: write_reads(*hip->solve_dedup(M, api, kDedupBins), true, q.out_path); break;
        case Mode::START_CAP: write_reads(*hip->solve_start_cap(M, api, kStartCapBins), true, q.out_path); break;
        case Mode::AMPLICONS: write_reads(*hip->solve_amplicons(M, api), true, q.out_path); break;
        case Mode::PROFILE: write_reads(*hip->solve_profile(M, api, offsets, starts, ends, caps), true, q.out_path); break;
        case Mode::PROPORTIONAL: write_reads(*hip->solve_proportional(M, api), true, q.out_path); break;
        case Mode::PAIRS: write_reads(*hip->solve_pairs(M, api), false, q.out_path); break;
        case Mode::CEILING: write_reads(*hip->solve_ceiling(M, api, offsets, starts, ends, caps), false, q.out_path); break;
        case Mode::BUDGET: write_reads(*hip->solve_budget(M, api), false, q.out_path); break;
        case Mode::MEAN_DEPTH: write_reads(*hip->solve_mean_depth(M, api), false, q.out_path); break;
        case Mode::THRESHOLDS: {  // the reads with a threshold, each record with its tag; no find_pairs
            kept = *hip->solve_thresholds(api);
            std::vector<std::uint16_t> values;
            values.reserve(kept.size());
            for (bam_api::ReadIndex i : kept) values.push_back(hip->last_thresholds()[i]);
            written.push_back(api.write_tagged_reads(q.out_path, kept, values, api.thresholds_tag()));
            break;
        }
        case Mode::LADDER: {
            const auto levels = hip->solve_ladder(M, api, api.coverage_ladder());
            for (std::size_t j = 0; j < levels.size(); ++j)
                write_reads(*levels[j], true, j == 0 ? q.out_path : path_from(q.ladder_template, "{M}", api.coverage_ladder()[j - 1]));
            break;
        }
        case Mode::REPLICATES: {
            const std::vector<std::uint8_t> labels = hip->solve_replicates(M, api);
            for (std::size_t r = 1; r <= api.replicates()->size() + 1; ++r) {
                qmcp::Solution labelled;
                for (std::size_t i = 0; i < labels.size(); ++i)
                    if (labels[i] == r) labelled.push_back(i);
                write_reads(labelled, false, r == 1 ? q.out_path : path_from(q.replicates_template, "{R}", r));
            }
            break;
        }
        case Mode::TEMPLATES: {  // whole templates: the kept RECORDS, written as they are
            std::vector<bam_api::BAMReadId> records = q.has_regions
                ? hip->solve_templates_profile(M, api, offsets, starts, ends, caps, q.default_cap)
                : hip->solve_templates(M, api);
            written.push_back(api.write_records(q.out_path, records));
            break;
        }
    }
    if (given(q.filtered_path)) api.write_bam_api_filtered_out_reads(q.filtered_path);

    for (std::size_t j = 0; written_out && j < written.size() && j < written_cap; ++j) written_out[j] = written[j];
    if (mode == Mode::CEILING && ceiling_stats) *ceiling_stats = hip->last_ceiling_stats();
    if (mode == Mode::BUDGET && budget_stats) *budget_stats = hip->last_budget_stats();
    if (mode == Mode::REPLICATES && replicates_stats) *replicates_stats = hip->last_replicates_stats();
    if (mode == Mode::TEMPLATES && template_stats) *template_stats = hip->last_template_stats();
    if (mode == Mode::TEMPLATES && q.has_regions && template_profile_stats)
        *template_profile_stats = hip->last_template_profile_stats();

    bool reported = true;
    if (mode == Mode::STRATIFIED && given(q.strata_report))
        reported = write_strata_report(q.strata_report, api.get_paired_reads_soa(), *hip);
    if (mode == Mode::TIERS && given(q.tiers_report))
        reported = write_tiers_report(q.tiers_report, api.get_paired_reads_soa(), api.mapq_tiers(), *hip, written[0], mates_added);
    if (mode == Mode::DEDUP && given(q.dedup_report)) reported = write_dedup_report(q.dedup_report, *hip);
    if (mode == Mode::START_CAP && given(q.start_cap_report))
        reported = write_start_cap_report(q.start_cap_report, *hip, written[0]);
    if (mode == Mode::AMPLICONS && given(q.amplicon_report)) {
        std::vector<std::string> names;
        std::vector<std::uint32_t> lengths;
        std::string why;
        reported = bam_api::read_bam_references(q.in_path, names, lengths, &why) &&
                   write_amplicon_report(q.amplicon_report, api.reference_amplicons(), names, *hip, kept);
    }
    if (mode == Mode::CEILING && given(q.ceiling_report))
        reported = write_ceiling_report(q.ceiling_report, hip->last_ceiling_stats(), written[0]);
    if (mode == Mode::TEMPLATES && given(q.fragment_report))
        reported = write_fragment_report(q.fragment_report, hip->last_fragment_stats(), written[0]);
    if (mode == Mode::PROPORTIONAL && given(q.proportional_report))
        reported = write_proportional_report(q.proportional_report, hip->last_proportional_stats(), written[0]);
    if (mode == Mode::BUDGET && given(q.budget_report))
        reported = write_budget_report(q.budget_report, hip->last_budget_stats(), hip->last_budget_curve(), written[0]);
    if (mode == Mode::THRESHOLDS && given(q.thresholds_report))
        reported = write_thresholds_report(q.thresholds_report, hip->last_thresholds_stats(), hip->last_threshold_counts(),
                                           written[0]);
    if (mode == Mode::MEAN_DEPTH && given(q.mean_depth_report))
        reported = write_mean_depth_report(q.mean_depth_report, hip->last_mean_depth_stats(), hip->last_mean_depth_curve(),
                                           written[0]);
    if (mode == Mode::REPLICATES && given(q.replicates_report))
        reported = write_replicates_report(q.replicates_report, hip->last_replicates_stats(), M, *api.replicates(), written);
    if (!api.depth_report_filepath().empty() || !api.depth_track_filepath().empty()) {
        std::vector<std::string> names;
        std::vector<std::uint32_t> lengths;
        std::string why;
        reported = bam_api::read_bam_references(q.in_path, names, lengths, &why);
        if (reported && !api.depth_report_filepath().empty()) reported = write_depth_report(*hip, M, api, kept, names, &why);
        if (reported && !api.depth_track_filepath().empty()) reported = write_depth_track(*hip, M, api, kept, names, &why);
        if (!reported) copy_err(why, err, err_cap);
    }
    if (!reported) return -5;
    return mode == Mode::LADDER || mode == Mode::REPLICATES ? (std::int64_t)written.size() : written[0];
}

}  // namespace

extern "C" {

// kind: 0 uniform, 1 x-x^2, 2 hole, 3 zero-on-both-sides.  Writes 2*pairs reads.
int qmcp_host_reads_gen(std::uint32_t seed, int kind, std::uint64_t pairs,
                        std::uint32_t genome_length, std::uint32_t read_length,
                        std::uint32_t* starts, std::uint32_t* ends, std::uint32_t* qualities) {
    if (genome_length < 2ull * read_length || read_length == 0) return -1;
    std::mt19937 gen(seed);
    switch (kind) {
        case 0:
            reads_gen::rand_reads_uniform_soa(gen, pairs, genome_length, read_length, starts, ends,
                                              qualities);
            return 0;
        case 1:
            reads_gen::rand_reads_soa(gen, pairs, genome_length, read_length, low_both_sides,
                                      starts, ends, qualities);
            return 0;
        case 2:
            reads_gen::rand_reads_soa(gen, pairs, genome_length, read_length, with_hole, starts,
                                      ends, qualities);
            return 0;
        case 3:
            reads_gen::rand_reads_soa(gen, pairs, genome_length, read_length, zero_both_sides,
                                      starts, ends, qualities);
            return 0;
        default:
            return -1;
    }
}

// AoS path of the generator (what the reference's tests call), copied out column-wise;
// lets a test check that the lean SoA variant and the AoS variant agree.
int qmcp_host_reads_gen_aos(std::uint32_t seed, int kind, std::uint64_t pairs,
                            std::uint32_t genome_length, std::uint32_t read_length,
                            std::uint32_t* starts, std::uint32_t* ends, std::uint32_t* qualities) {
    std::mt19937 gen(seed);
    bam_api::AOSPairedReads r;
    if (kind == 0) r = reads_gen::rand_reads_uniform(gen, pairs, genome_length, read_length);
    else if (kind == 1) r = reads_gen::rand_reads(gen, pairs, genome_length, read_length, low_both_sides);
    else if (kind == 2) r = reads_gen::rand_reads(gen, pairs, genome_length, read_length, with_hole);
    else if (kind == 3) r = reads_gen::rand_reads(gen, pairs, genome_length, read_length, zero_both_sides);
    else return -1;
    for (std::size_t i = 0; i < r.reads.size(); ++i) {
        starts[i] = static_cast<std::uint32_t>(r.reads[i].start_ind);
        ends[i] = static_cast<std::uint32_t>(r.reads[i].end_ind);
        if (qualities) qualities[i] = r.reads[i].quality;
        if (r.reads[i].bam_id != i || r.reads[i].is_first_read != (i % 2 == 0)) return -2;
    }
    return 0;
}

// BED (+ optional TSV, may be NULL or "") -> amplicon intervals, as BamApi::set_amplicon_filter
// builds them.  Returns the number of amplicons, -1 if a file cannot be opened, -2 if cap is
// too small.
int qmcp_host_amplicons_from_files(const char* bed_path, const char* tsv_path,
                                   std::uint32_t* starts, std::uint32_t* ends, std::size_t cap) {
    bam_api::AmpliconSet set;
    if (!bam_api::amplicon_set_from_files(bed_path, tsv_path ? tsv_path : "", set)) return -1;
    if (set.amplicons.size() > cap) return -2;
    for (std::size_t i = 0; i < set.amplicons.size(); ++i) {
        starts[i] = static_cast<std::uint32_t>(set.amplicons[i].start);
        ends[i] = static_cast<std::uint32_t>(set.amplicons[i].end);
    }
    return static_cast<int>(set.amplicons.size());
}

// In-memory BamApi helpers as the reference's tests use them (src/tests/coverage_tester.cpp:
// find_input_cover / find_filtered_cover; src/app.cpp:141: find_pairs).  `layout` 0 builds the
// BamApi from an AoS container, 1 from an SoA one (both constructors exist in the reference).
// cover_in / cover_out have ref_genome_length entries; paired_out capacity n; returns the
// number of paired ids.
std::int64_t qmcp_host_bamapi_probe(const std::uint32_t* starts, const std::uint32_t* ends,
                                    std::uint64_t n, std::uint32_t ref_genome_length, int layout,
                                    const std::uint64_t* ids, std::uint64_t n_ids,
                                    std::uint32_t* cover_in, std::uint32_t* cover_out,
                                    std::uint64_t* paired_out) {
    bam_api::AOSPairedReads aos;
    aos.ref_genome_length = ref_genome_length;
    for (std::uint64_t i = 0; i < n; ++i)
        aos.push_back(bam_api::Read(i, starts[i], ends[i], 0, ends[i] - starts[i] + 1, i % 2 == 0));
    bam_api::SOAPairedReads soa;
    soa.from(aos);
    bam_api::BamApi api = layout == 0 ? bam_api::BamApi(aos) : bam_api::BamApi(soa);
    // exercise the lazy layout conversion both ways
    if (api.get_paired_reads_aos().reads.size() != n || api.get_paired_reads_soa().ids.size() != n)
        return -1;
    const std::vector<bam_api::ReadIndex> idv(ids, ids + n_ids);
    const auto in = api.find_input_cover();
    const auto out = api.find_filtered_cover(idv);
    for (std::size_t p = 0; p < in.size(); ++p) { cover_in[p] = in[p]; cover_out[p] = out[p]; }
    const auto paired = api.find_pairs(idv);
    for (std::size_t i = 0; i < paired.size(); ++i) paired_out[i] = paired[i];
    return static_cast<std::int64_t>(paired.size());
}

// Names registered in the SolverManager, '\n'-separated, into buf.
int qmcp_host_solver_names(char* buf, std::size_t cap) {
    std::string all;
    for (const std::string& n : manager().get_names()) { all += n; all += '\n'; }
    if (all.size() + 1 > cap) return -1;
    std::memcpy(buf, all.c_str(), all.size() + 1);
    return static_cast<int>(manager().get_names().size());
}

// 1 if the solver of that name (the default manager's, or "quasi-mcp-hip-quality") uses the reads' qualities -- the
// app then grades amplicon pairs instead of filtering them --, 0 if not, -1 for an unknown name.  Builds nothing on the
// device: solvers touch it on their first solve only.
int qmcp_host_solver_uses_quality(const char* solver_name) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    return found->uses_quality_of_reads() ? 1 : 0;
}

// qmcp_host_solve with each read's quality (qmcp_host_solve builds reads of quality 0): kept_out (capacity n) gets the
// ascending ReadIndex, with_pairs != 0 applies BamApi::find_pairs.  adapter_pairs != 0: the solver itself completes
// pairs on the device for this call (QuasiMcpHipSolver::set_complete_pairs; -2 for a solver without that setter).
// Negative on an unknown solver.
std::int64_t qmcp_host_solve_with_qualities(const char* solver_name, const std::uint32_t* starts,
                                            const std::uint32_t* ends, const std::uint32_t* qualities, std::uint64_t n,
                                            std::uint32_t ref_genome_length, std::uint32_t max_coverage,
                                            int with_pairs, int adapter_pairs, std::uint64_t* kept_out) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::AOSPairedReads aos;
    aos.ref_genome_length = ref_genome_length;
    aos.reserve(n);
    for (std::uint64_t i = 0; i < n; ++i)
        aos.push_back(bam_api::Read(i, starts[i], ends[i], qualities[i], ends[i] - starts[i] + 1, i % 2 == 0));
    bam_api::BamApi api(aos);
    auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
    if (adapter_pairs && hip == nullptr) return -2;
    if (adapter_pairs) hip->set_complete_pairs(true);
    auto solution = found->solve(max_coverage, api);
    if (adapter_pairs) hip->set_complete_pairs(false);
    std::vector<bam_api::ReadIndex> ids = with_pairs ? api.find_pairs(*solution) : *solution;
    for (std::size_t i = 0; i < ids.size(); ++i) kept_out[i] = ids[i];
    return static_cast<std::int64_t>(ids.size());
}

// Runs SolverManager::get(name).solve(M, BamApi(aos)) the way src/app.cpp:134-135 and
// src/tests/coverage_tester.cpp:109-118 do; returns the number of kept reads, fills
// kept_out (capacity n) with ascending ReadIndex; with_pairs != 0 additionally applies
// BamApi::find_pairs (src/app.cpp:141).  Negative on unknown solver.
std::int64_t qmcp_host_solve(const char* solver_name, const std::uint32_t* starts,
                             const std::uint32_t* ends, std::uint64_t n,
                             std::uint32_t ref_genome_length, std::uint32_t max_coverage,
                             int with_pairs, std::uint64_t* kept_out) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::AOSPairedReads aos;
    aos.ref_genome_length = ref_genome_length;
    aos.reserve(n);
    for (std::uint64_t i = 0; i < n; ++i)
        aos.push_back(bam_api::Read(i, starts[i], ends[i], 0, ends[i] - starts[i] + 1, i % 2 == 0));
    bam_api::BamApi api(aos);
    qmcp::Solver& solver = *found;
    auto solution = solver.solve(max_coverage, api);
    std::vector<bam_api::ReadIndex> ids = with_pairs ? api.find_pairs(*solution) : *solution;
    for (std::size_t i = 0; i < ids.size(); ++i) kept_out[i] = ids[i];
    return static_cast<std::int64_t>(ids.size());
}

// ---- BAM ingest / emit (bam-api/bam_io.hpp) for ctypes callers
// Writes a synthetic single-reference BAM: record i = {qname "q<names[i]>", flags[i], pos[i], mapq[i], CIGAR
// "<clip_front[i]>S<match[i]>M<del[i]>D<match2[i]>M" with zero-length parts left out, l_seq = sum of S and M}.
int qmcp_host_write_synthetic_bam(const char* path, std::uint32_t ref_length, std::uint64_t n,
                                  const std::uint32_t* names, const std::uint16_t* flags,
                                  const std::uint32_t* pos, const std::uint8_t* mapq,
                                  const std::uint32_t* clip_front, const std::uint32_t* match,
                                  const std::uint32_t* del, const std::uint32_t* match2) {
    std::vector<bam_api::BamRecordSpec> recs(n);
    for (std::uint64_t i = 0; i < n; ++i) {
        bam_api::BamRecordSpec& r = recs[i];
        r.qname = "q" + std::to_string(names[i]);
        r.flag = flags[i];
        r.pos = (std::int32_t)pos[i];
        r.mapq = mapq[i];
        if (clip_front[i]) r.cigar.push_back({clip_front[i], 'S'});
        if (match[i]) r.cigar.push_back({match[i], 'M'});
        if (del[i]) r.cigar.push_back({del[i], 'D'});
        if (match2[i]) r.cigar.push_back({match2[i], 'M'});
        r.l_seq = clip_front[i] + match[i] + match2[i];
    }
    std::string err;
    return bam_api::write_synthetic_bam(path, "ref1", ref_length, recs, &err) ? 0 : -1;
}

// BamApi(path, config) -> get_paired_reads_soa(): columns out (capacity cap reads); returns the number of
// imported reads, *n_filtered_out = size of get_filtered_out_reads() (ids into filtered_out, capacity cap_f),
// *ref_len = ref_genome_length.  amplicon_mode: 0 IGNORE, 1 FILTER, 2 GRADE (bed/tsv may be NULL or "").  -2 when a
// capacity is too small, -3 out of memory, -4 when BamApi refuses the configuration.
std::int64_t qmcp_host_read_bam(const char* path, const char* bed, const char* tsv, int amplicon_mode,
                                std::uint32_t min_len, std::uint32_t min_mapq, std::uint64_t cap,
                                std::uint64_t* bam_ids, std::uint32_t* starts, std::uint32_t* ends,
                                std::uint32_t* qualities, std::uint32_t* seq_lengths, std::uint8_t* is_first,
                                std::uint64_t cap_f, std::uint64_t* filtered_out, std::uint64_t* n_filtered_out,
                                std::uint32_t* ref_len) {
    return guarded(nullptr, 0, [&]() -> std::int64_t {
        bam_api::BamApi api(path, ingest_config(bed, tsv, amplicon_mode, min_len, min_mapq));
        const std::int64_t n = copy_out_reads(api, {cap, bam_ids, starts, ends, qualities, seq_lengths, is_first, nullptr, nullptr},
                                              {cap_f, filtered_out, n_filtered_out, 0, nullptr, nullptr});
        if (n >= 0) *ref_len = (std::uint32_t)api.get_paired_reads_soa().ref_genome_length;
        return n;
    });
}

// qmcp_host_read_bam with amplicon_mode (0 IGNORE, 1 FILTER, 2 GRADE) and the two flags of BamApiConfig (per_reference,
// amplicons_by_reference): the same columns, plus each read's contig id (contig_ids, cap entries; QMCP_NO_CONTIG for an
// unmapped read, 0 without per_reference) and every reference's length (ref_lengths, ref_cap entries; *n_refs receives
// the count).  -2 when a capacity is too small, -3 out of memory, -4 when BamApi refuses the configuration or the
// amplicon files (message in err).
std::int64_t qmcp_host_read_bam_by_reference(const char* path, const char* bed, const char* tsv, int amplicon_mode,
                                             int per_reference, int amplicons_by_reference, std::uint32_t min_len,
                                             std::uint32_t min_mapq, std::uint64_t cap, std::uint64_t* bam_ids,
                                             std::uint32_t* starts, std::uint32_t* ends, std::uint32_t* qualities,
                                             std::uint32_t* seq_lengths, std::uint8_t* is_first,
                                             std::uint32_t* contig_ids, std::uint64_t cap_f,
                                             std::uint64_t* filtered_out, std::uint64_t* n_filtered_out,
                                             std::uint64_t ref_cap, std::uint32_t* ref_lengths, std::uint64_t* n_refs,
                                             char* err, std::size_t err_cap) {
    return guarded(err, err_cap, [&]() -> std::int64_t {
        bam_api::BamApiConfig cfg = ingest_config(bed, tsv, amplicon_mode, min_len, min_mapq);
        cfg.per_reference = per_reference != 0;
        cfg.amplicons_by_reference = amplicons_by_reference != 0;
        bam_api::BamApi api(path, cfg);
        return copy_out_reads(api, {cap, bam_ids, starts, ends, qualities, seq_lengths, is_first, contig_ids, nullptr},
                              {cap_f, filtered_out, n_filtered_out, ref_cap, ref_lengths, n_refs});
    });
}

// qmcp_host_read_bam_by_reference with its two flags fixed: per_reference on, amplicons_by_reference off (amplicon
// files are then refused, -4), amplicons ignored
std::int64_t qmcp_host_read_bam_per_reference(const char* path, const char* bed, const char* tsv,
                                              std::uint32_t min_len, std::uint32_t min_mapq, std::uint64_t cap,
                                              std::uint64_t* bam_ids, std::uint32_t* starts, std::uint32_t* ends,
                                              std::uint32_t* qualities, std::uint32_t* seq_lengths,
                                              std::uint8_t* is_first, std::uint32_t* contig_ids, std::uint64_t cap_f,
                                              std::uint64_t* filtered_out, std::uint64_t* n_filtered_out,
                                              std::uint64_t ref_cap, std::uint32_t* ref_lengths, std::uint64_t* n_refs,
                                              char* err, std::size_t err_cap) {
    return qmcp_host_read_bam_by_reference(path, bed, tsv, /*amplicon_mode=*/0, /*per_reference=*/1,
                                           /*amplicons_by_reference=*/0, min_len, min_mapq, cap, bam_ids, starts, ends,
                                           qualities, seq_lengths, is_first, contig_ids, cap_f, filtered_out, n_filtered_out,
                                           ref_cap, ref_lengths, n_refs, err, err_cap);
}

// qmcp_host_read_bam_by_reference with BamApiConfig::stratify_by ("strand" / "read_group") in place of amplicons: the
// same columns, plus each read's stratum (strata, cap entries) and the strata's names, one per line, in names_out
// (names_cap bytes; *n_strata receives the count).  -2 when a capacity is too small, -3 out of memory, -4 with the
// message in err.
std::int64_t qmcp_host_read_bam_stratified(const char* path, const char* stratify, std::uint32_t min_len,
                                           std::uint32_t min_mapq, std::uint64_t cap, std::uint64_t* bam_ids,
                                           std::uint32_t* starts, std::uint32_t* ends, std::uint32_t* qualities,
                                           std::uint32_t* seq_lengths, std::uint8_t* is_first, std::uint32_t* contig_ids,
                                           std::uint32_t* strata, std::uint64_t cap_f, std::uint64_t* filtered_out,
                                           std::uint64_t* n_filtered_out, std::uint64_t ref_cap,
                                           std::uint32_t* ref_lengths, std::uint64_t* n_refs, char* names_out,
                                           std::size_t names_cap, std::uint64_t* n_strata, int per_reference, char* err,
                                           std::size_t err_cap) {
    return guarded(err, err_cap, [&]() -> std::int64_t {
        bam_api::BamApiConfig cfg = ingest_config(nullptr, nullptr, 0, min_len, min_mapq);
        cfg.per_reference = per_reference != 0;
        cfg.stratify_by = stratify_from_name(stratify);
        bam_api::BamApi api(path, cfg);
        const bam_api::SOAPairedReads& r = api.get_paired_reads_soa();
        std::string names;
        for (const std::string& s : r.stratum_names) names += s + "\n";
        if (names.size() + 1 > names_cap) return -2;
        const std::int64_t n = copy_out_reads(api, {cap, bam_ids, starts, ends, qualities, seq_lengths, is_first, contig_ids, strata},
                                              {cap_f, filtered_out, n_filtered_out, ref_cap, ref_lengths, n_refs});
        if (n < 0) return n;
        std::memcpy(names_out, names.c_str(), names.size() + 1);
        *n_strata = r.stratum_names.size();
        return n;
    });
}

// Template-aware ingest alone (BamApiConfig::template_aware; bam_api::read_bam_templates): the segments' columns (cap
// entries each; segment_records: each segment's BAM record id), the skipped and dropped records (filtered_out, cap_f
// entries), every reference's length and the number of templates.  Returns the number of segments; -2 when a capacity is
// too small, -3 out of memory, -1 with the reader's message in err on a malformed or unreadable file.
std::int64_t qmcp_host_read_bam_templates(const char* path, std::uint32_t min_len, std::uint32_t min_mapq,
                                          int split_spliced, int include_secondary, std::uint64_t cap,
                                          std::uint32_t* starts, std::uint32_t* ends, std::uint32_t* contig_ids,
                                          std::uint32_t* template_ids, std::uint32_t* qualities,
                                          std::uint32_t* seq_lengths, std::uint64_t* segment_records, std::uint64_t cap_f,
                                          std::uint64_t* filtered_out, std::uint64_t* n_filtered_out, std::uint64_t ref_cap,
                                          std::uint32_t* ref_lengths, std::uint64_t* n_refs, std::uint64_t* n_templates,
                                          char* err, std::size_t err_cap) {
    return guarded(err, err_cap, [&]() -> std::int64_t {
        bam_api::TemplateIngest cfg;
        cfg.min_seq_length = min_len;
        cfg.min_mapq = min_mapq;
        cfg.split_spliced = split_spliced != 0;
        cfg.include_secondary = include_secondary != 0;
        bam_api::TemplateSegments seg;
        std::vector<bam_api::BAMReadId> filtered;
        std::string msg;
        if (!bam_api::read_bam_templates(path, cfg, seg, filtered, &msg)) {
            copy_err(msg, err, err_cap);
            return -1;
        }
        const std::uint64_t n = seg.starts.size();
        if (n > cap || !copy_out_ingest(filtered, seg.contig_lengths, {cap_f, filtered_out, n_filtered_out, ref_cap, ref_lengths, n_refs}))
            return -2;
        for (std::uint64_t i = 0; i < n; ++i) {
            starts[i] = seg.starts[i]; ends[i] = seg.ends[i]; contig_ids[i] = seg.contig_ids[i];
            template_ids[i] = seg.template_ids[i]; qualities[i] = seg.qualities[i]; seq_lengths[i] = seg.seq_lengths[i];
            segment_records[i] = seg.segment_records[i];
        }
        *n_templates = seg.n_templates;
        return (std::int64_t)n;
    });
}

// BED (+ optional TSV, may be NULL or "") against the references ref_names[0..n_refs) -> the amplicons of every
// reference in CSR form (build_reference_amplicon_set): offsets_out (n_refs + 1 entries), starts_out / ends_out (cap
// entries).  Returns the number of amplicons, -2 if cap is too small, -4 with the message in err (a file that cannot
// be opened, an unknown chrom, a TSV pair across references).
std::int64_t qmcp_host_amplicons_by_reference(const char* bed_path, const char* tsv_path, const char* const* ref_names,
                                              std::uint64_t n_refs, std::uint32_t* offsets_out, std::uint32_t* starts_out,
                                              std::uint32_t* ends_out, std::uint64_t cap, char* err, std::size_t err_cap) {
    try {
        std::vector<std::string> names;
        for (std::uint64_t r = 0; r < n_refs; ++r) names.emplace_back(ref_names[r]);
        bam_api::ReferenceAmpliconSet set;
        std::string msg;
        if (!bam_api::reference_amplicon_set_from_files(bed_path, tsv_path ? tsv_path : "", names, set, &msg)) {
            copy_err(msg, err, err_cap);
            return -4;
        }
        if (set.starts.size() > cap) return -2;
        for (std::size_t k = 0; k < set.offsets.size(); ++k) offsets_out[k] = set.offsets[k];
        for (std::size_t i = 0; i < set.starts.size(); ++i) {
            starts_out[i] = static_cast<std::uint32_t>(set.starts[i]);
            ends_out[i] = static_cast<std::uint32_t>(set.ends[i]);
        }
        return static_cast<std::int64_t>(set.starts.size());
    } catch (const std::bad_alloc&) {
        return -3;
    }
}

// The same set's inserts and left primer names, parallel to qmcp_host_amplicons_by_reference's starts / ends:
// insert_starts_out / insert_ends_out (cap entries, inclusive: from BED primers [ls, le) and [rs, re) the insert is
// [le, rs - 1]) and the names '\n'-separated in names_out (capacity names_cap).  Returns the number of amplicons, -2 if
// a capacity is too small, -4 with the message in err -- also for a primer pair that leaves no insert, naming it.
std::int64_t qmcp_host_amplicon_inserts_by_reference(const char* bed_path, const char* tsv_path,
                                                     const char* const* ref_names, std::uint64_t n_refs,
                                                     std::uint32_t* insert_starts_out, std::uint32_t* insert_ends_out,
                                                     std::uint64_t cap, char* names_out, std::size_t names_cap, char* err,
                                                     std::size_t err_cap) {
    try {
        std::vector<std::string> names;
        for (std::uint64_t r = 0; r < n_refs; ++r) names.emplace_back(ref_names[r]);
        bam_api::ReferenceAmpliconSet set;
        std::string msg;
        if (!bam_api::reference_amplicon_set_from_files(bed_path, tsv_path ? tsv_path : "", names, set, &msg)) {
            copy_err(msg, err, err_cap);
            return -4;
        }
        if (!set.empty_insert.empty()) {
            copy_err(set.empty_insert, err, err_cap);
            return -4;
        }
        std::string all;
        for (const std::string& n : set.left_names) { all += n; all += '\n'; }
        if (set.starts.size() > cap || all.size() + 1 > names_cap) return -2;
        for (std::size_t i = 0; i < set.starts.size(); ++i) {
            insert_starts_out[i] = static_cast<std::uint32_t>(set.insert_starts[i]);
            insert_ends_out[i] = static_cast<std::uint32_t>(set.insert_ends[i]);
        }
        std::memcpy(names_out, all.c_str(), all.size() + 1);
        return static_cast<std::int64_t>(set.starts.size());
    } catch (const std::bad_alloc&) {
        return -3;
    }
}

// The header's reference names, '\n'-separated, into buf (capacity cap) and their lengths (lengths_cap entries).
// Returns the number of references, -2 if a capacity is too small, -1 with the reader's message in buf.
std::int64_t qmcp_host_reference_names(const char* path, char* buf, std::size_t cap, std::uint32_t* lengths,
                                       std::uint64_t lengths_cap) {
    std::vector<std::string> names;
    std::vector<std::uint32_t> lens;
    std::string msg;
    if (!bam_api::read_bam_references(path, names, lens, &msg)) {
        copy_err(msg, buf, cap);
        return -1;
    }
    std::string all;
    for (const std::string& n : names) { all += n; all += '\n'; }
    if (all.size() + 1 > cap || lens.size() > lengths_cap) return -2;
    std::memcpy(buf, all.c_str(), all.size() + 1);
    for (std::size_t k = 0; k < lens.size(); ++k) lengths[k] = lens[k];
    return static_cast<std::int64_t>(names.size());
}


// read_bam's own verdict on a file, without BamApi's exit-on-error (the reference exits the process on an
// unreadable input; a caller that wants to look first -- and the tests of corrupt files -- use this): 0 and the
// number of imported reads in *n_reads, or -1 and the reader's message in err (capacity cap).  Allocation
// failures on absurd sizes are reported the same way, never thrown through the C boundary.
int qmcp_host_check_bam(const char* path, std::uint64_t* n_reads, char* err, std::size_t cap) {
    std::string msg;
    int rc = -1;
    try {
        bam_api::SOAPairedReads reads;
        std::vector<bam_api::BAMReadId> filtered;
        bam_api::BamFilters f;
        if (bam_api::read_bam(path, f, reads, filtered, nullptr, &msg)) {
            if (n_reads) *n_reads = reads.ids.size();
            rc = 0;
        }
    } catch (const std::bad_alloc&) {
        msg = "out of memory while reading the BAM file";
    } catch (const std::exception& e) {
        msg = e.what();
    }
    if (err && cap) {
        std::strncpy(err, msg.c_str(), cap - 1);
        err[cap - 1] = 0;
    }
    return rc;
}

// BamApi::write_bam alone (bam_api.cpp:534-656): the header and the records whose running id is in `ids` (n of them;
// sorted here, as the reference sorts them) copied to `out_path` -- BAM if it ends in ".bam", SAM text otherwise.
// Returns the number of records written, -1 on failure (message in err, capacity cap).
std::int64_t qmcp_host_copy_records(const char* in_path, const char* out_path, const std::uint64_t* ids, std::uint64_t n,
                                    char* err, std::size_t cap) {
    std::string msg;
    std::int64_t rc = -1;
    try {
        std::vector<bam_api::BAMReadId> v(ids, ids + n);
        const std::uint32_t written = bam_api::write_bam(in_path, out_path, v, &msg);
        if (written != UINT32_MAX) rc = (std::int64_t)written;
    } catch (const std::exception& e) {
        msg = e.what();
    }
    if (err && cap) {
        std::strncpy(err, msg.c_str(), cap - 1);
        err[cap - 1] = 0;
    }
    return rc;
}

// qmcp_host_copy_records with the aux field <tag>:S:<values[k]> appended to the record ids[k] (bam_api::write_bam_tagged):
// -1 with the reason in err -- before anything is written -- for a tag that is not [A-Za-z][A-Za-z0-9] and for a record
// that carries the tag already.
std::int64_t qmcp_host_copy_records_tagged(const char* in_path, const char* out_path, const std::uint64_t* ids,
                                           const std::uint16_t* values, std::uint64_t n, const char* tag, char* err,
                                           std::size_t cap) {
    std::string msg;
    std::int64_t rc = -1;
    try {
        std::vector<std::pair<bam_api::BAMReadId, std::uint16_t>> tagged;
        for (std::uint64_t k = 0; k < n; ++k) tagged.emplace_back(ids[k], values[k]);
        const std::uint32_t written = bam_api::write_bam_tagged(in_path, out_path, tagged, tag ? tag : "", &msg);
        if (written != UINT32_MAX) rc = (std::int64_t)written;
    } catch (const std::exception& e) {
        msg = e.what();
    }
    if (err && cap) {
        std::strncpy(err, msg.c_str(), cap - 1);
        err[cap - 1] = 0;
    }
    return rc;
}

// The file-to-file flow of App::execute (src/app.cpp:113-151), one entry for every mode: see
// include/qmcp_host_request.h and downsample() above.
std::int64_t qmcp_host_downsample_bam(const qmcp_host_downsample_request* request, std::int64_t* written_out,
                                      std::uint64_t written_cap, qmcp_hip_ceiling_stats* ceiling_stats,
                                      qmcp_hip_budget_stats* budget_stats, qmcp_hip_replicates_stats* replicates_stats,
                                      qmcp_hip_template_stats* template_stats,
                                      qmcp_hip_template_profile_stats* template_profile_stats, char* err, std::size_t err_cap) {
    return guarded(err, err_cap, [&]() -> std::int64_t {
        if (request == nullptr) throw std::invalid_argument("no request");
        return downsample(*request, written_out, written_cap, ceiling_stats, budget_stats, replicates_stats, template_stats,
                          template_profile_stats, err, err_cap);
    });
}

// BamApiConfig's rule for targets, without a solve: 0 when BamApi accepts {per_reference, targets, padding}, -4 with its
// message otherwise (targets without per_reference, an unknown chrom, a malformed line)
std::int64_t qmcp_host_check_targets_config(const char* in_path, const char* targets, int per_reference,
                                            std::uint32_t target_padding, std::uint64_t* n_regions, char* err,
                                            std::size_t err_cap) {
    return guarded(err, err_cap, [&]() -> std::int64_t {
        bam_api::BamApiConfig cfg;
        cfg.per_reference = per_reference != 0;
        if (given(targets)) cfg.targets_filepath = targets;
        cfg.target_padding = target_padding;
        bam_api::BamApi api(in_path, cfg);
        if (n_regions) *n_regions = api.has_targets() ? api.get_targets().starts.size() : 0;
        return 0;
    });
}

// The span the reference times as "solve took" (src/app.cpp:132-139) at the plugin boundary: a BamApi
// that already holds the reads as SOAPairedReads (size_t columns) -> solver.solve(M, api) -> Solution.
// Building the BamApi is outside the span, as parsing the BAM is in the reference.  `times` receives
// {wall of solve(), library total, narrow + H2D, device solve, D2H, mask expansion, threads, chunks,
// columns sent};
// returns the number of kept reads (kept_out may be NULL), negative on an unknown solver.
std::int64_t qmcp_host_plugin_solve_timed(const char* solver_name, const std::uint32_t* starts,
                                          const std::uint32_t* ends, std::uint64_t n,
                                          std::uint32_t ref_genome_length, std::uint32_t max_coverage,
                                          std::uint64_t* kept_out, float* times) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::SOAPairedReads soa;
    soa.ref_genome_length = ref_genome_length;
    soa.reserve(n);
    for (std::uint64_t i = 0; i < n; ++i)
        soa.push_back(bam_api::Read(i, starts[i], ends[i], 0, ends[i] - starts[i] + 1, i % 2 == 0));
    bam_api::BamApi api(soa);
    qmcp::Solver& solver = *found;
    const auto t0 = std::chrono::steady_clock::now();
    auto solution = solver.solve(max_coverage, api);
    const float wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (times) {
        for (int i = 0; i < 9; ++i) times[i] = 0.f;
        times[0] = wall;
        if (auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(&solver)) {
            const qmcp_hip_host_breakdown& b = hip->last_breakdown();
            times[1] = b.ms_total; times[2] = b.ms_narrow_h2d; times[3] = b.ms_solve; times[4] = b.ms_d2h;
            times[5] = hip->last_expand_ms(); times[6] = (float)b.host_threads; times[7] = (float)b.chunks;
            times[8] = (float)b.columns_sent;
        }
    }
    if (kept_out) for (std::size_t i = 0; i < solution->size(); ++i) kept_out[i] = (*solution)[i];
    return static_cast<std::int64_t>(solution->size());
}

}  // extern "C"
