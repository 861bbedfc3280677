// In-memory BamApi (see include/bam-api/bam_api.hpp for the reference lines mirrored).
#include "bam-api/bam_api.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>

#include "bam-api/bam_io.hpp"
#include "qmcp_hip.h"  // QMCP_TIERS_MAX

namespace bam_api {

bool target_regions_from_bed(const std::filesystem::path& bed, const std::vector<std::string>& ref_names,
                             TargetRegions& out, std::string* err) {
    auto fail = [err](const std::string& msg) {
        if (err) *err = msg;
        return false;
    };
    std::ifstream file(bed);
    if (!file.is_open()) return fail("could not open " + bed.string());
    std::map<std::string, std::uint32_t> ref_of;
    for (std::size_t r = 0; r < ref_names.size(); ++r) ref_of.emplace(ref_names[r], (std::uint32_t)r);
    std::vector<std::vector<std::pair<std::uint32_t, std::uint32_t>>> per(ref_names.size());
    std::string line;
    std::size_t lineno = 0;
    while (std::getline(file, line)) {
        ++lineno;
        const std::string where = bed.string() + ":" + std::to_string(lineno);
        std::istringstream fields(line);
        std::string chrom, start, end;
        if (!(fields >> chrom) || chrom[0] == '#' || chrom == "track" || chrom == "browser") continue;
        if (!(fields >> start >> end)) return fail(where + ": a BED line needs chrom, start and end");
        unsigned long long s = 0, e = 0;
        try {
            std::size_t used_s = 0, used_e = 0;
            s = std::stoull(start, &used_s);
            e = std::stoull(end, &used_e);
            if (used_s != start.size() || used_e != end.size() || start[0] == '-' || end[0] == '-')
                throw std::invalid_argument("");
        } catch (const std::exception&) {
            return fail(where + ": start and end must be integers");
        }
        if (e <= s || e > 0xFFFFFFFFull) return fail(where + ": region is empty or out of range");
        const auto ref = ref_of.find(chrom);
        if (ref == ref_of.end())
            return fail(where + ": BED chrom \"" + chrom + "\" names no reference of the BAM file (names must match exactly)");
        per[ref->second].emplace_back((std::uint32_t)s, (std::uint32_t)(e - 1));  // half-open -> inclusive
    }
    out.offsets.assign(1, 0);
    out.starts.clear();
    out.ends.clear();
    for (const auto& v : per) {
        for (const auto& r : v) {
            out.starts.push_back(r.first);
            out.ends.push_back(r.second);
        }
        out.offsets.push_back((std::uint32_t)out.starts.size());
    }
    return true;
}

// bam_api.cpp:32-43: filters from the config; amplicons only when a BED file is given
BamApi::BamApi(const std::filesystem::path& input_filepath, const BamApiConfig& config)
    : input_filepath_(input_filepath), min_seq_length_(config.min_seq_length), min_mapq_(config.min_mapq),
      per_reference_(config.per_reference), amplicons_by_reference_(config.amplicons_by_reference) {
    if (amplicons_by_reference_ && !per_reference_)
        throw std::invalid_argument("amplicons_by_reference needs per_reference: amplicons are matched to the "
                                    "references a per-reference ingest keeps");
    if (!config.mapq_tiers.empty()) {
        const auto no = [](const char* what) {
            throw std::invalid_argument(std::string("tiered downsampling does not go together with ") + what);
        };
        if (!per_reference_)
            throw std::invalid_argument("tiered downsampling needs per_reference: a tier is solved one reference at a time");
        if (config.mapq_tiers.size() > QMCP_TIERS_MAX)
            throw std::invalid_argument("mapq_tiers: at most " + std::to_string(QMCP_TIERS_MAX) + " thresholds");
        for (std::size_t k = 1; k < config.mapq_tiers.size(); ++k)
            if (config.mapq_tiers[k] >= config.mapq_tiers[k - 1])
                throw std::invalid_argument("mapq_tiers must fall strictly");
        if (config.mapq_tiers.back() != config.min_mapq)
            throw std::invalid_argument("the last threshold of mapq_tiers must equal min_mapq: every read the ingest lets "
                                        "through needs a tier");
        if (config.primer_clip || config.per_amplicon || !config.amplicon_report_filepath.empty())
            no("amplicon-aware downsampling");
        if (config.start_cap) no("a start cap");
        if (config.thresholds_hi.has_value()) no("coverage thresholds");
        if (config.mean_depth.has_value() || config.budget_bases.has_value()) no("a mean depth");
        if (config.proportion.has_value()) no("a proportion");
        if (config.replicates.has_value()) no("replicates");
        if (config.budget_reads.has_value() || config.budget_fraction.has_value()) no("a budget");
        if (config.ceiling) no("ceiling");
        if (config.pair_aware) no("pair_aware");
        if (config.template_aware) no("template_aware");
        if (!config.targets_filepath.empty()) no("targets");
        if (!config.depth_report_filepath.empty()) no("a depth report");
        if (!config.depth_track_filepath.empty()) no("a depth track");
        if (!config.coverage_ladder.empty()) no("a coverage ladder");
        if (config.stratify_by != Stratify::NONE) no("stratify_by");
        if (config.dedup) no("dedup");
        if (config.amplicons_by_reference || !config.bed_filepath.empty() || !config.tsv_filepath.empty())
            throw std::invalid_argument("tiered downsampling does not take amplicon files");
        mapq_tiers_ = config.mapq_tiers;
    }
    if (config.start_cap) {
        const auto no = [](const char* what) {
            throw std::invalid_argument(std::string("a start cap does not go together with ") + what);
        };
        if (!per_reference_)
            throw std::invalid_argument("a start cap needs per_reference: a start site includes its reference");
        if (config.thresholds_hi.has_value()) no("coverage thresholds");
        if (config.mean_depth.has_value() || config.budget_bases.has_value()) no("a mean depth");
        if (config.proportion.has_value()) no("a proportion");
        if (config.replicates.has_value()) no("replicates");
        if (config.budget_reads.has_value() || config.budget_fraction.has_value()) no("a budget");
        if (config.ceiling) no("ceiling");
        if (config.pair_aware) no("pair_aware");
        if (config.template_aware) no("template_aware");
        if (!config.targets_filepath.empty()) no("targets");
        if (!config.depth_report_filepath.empty()) no("a depth report");
        if (!config.depth_track_filepath.empty()) no("a depth track");
        if (!config.coverage_ladder.empty()) no("a coverage ladder");
        if (config.stratify_by != Stratify::NONE) no("stratify_by");
        if (config.dedup) no("dedup");
        if (config.amplicons_by_reference || !config.bed_filepath.empty() || !config.tsv_filepath.empty())
            throw std::invalid_argument("a start cap does not take amplicon files");
        start_cap_ = config.start_cap;
        start_cap_by_strand_ = config.start_cap_by_strand;
    } else if (config.start_cap_by_strand) {
        throw std::invalid_argument("start_cap_by_strand needs start_cap");
    }
    if (config.primer_clip || config.per_amplicon || !config.amplicon_report_filepath.empty()) {
        const auto no = [](const char* what) {
            throw std::invalid_argument(std::string("amplicon-aware downsampling does not go together with ") + what);
        };
        if (!per_reference_ || !amplicons_by_reference_ || config.bed_filepath.empty())
            throw std::invalid_argument("primer_clip, per_amplicon and amplicon_report need bed, per_reference and "
                                        "amplicons_by_reference: a read is clipped by an amplicon of its own reference");
        if (config.start_cap) no("a start cap");
        if (config.thresholds_hi.has_value()) no("coverage thresholds");
        if (config.mean_depth.has_value() || config.budget_bases.has_value()) no("a mean depth");
        if (config.proportion.has_value()) no("a proportion");
        if (config.replicates.has_value()) no("replicates");
        if (config.budget_reads.has_value() || config.budget_fraction.has_value()) no("a budget");
        if (config.ceiling) no("ceiling");
        if (config.pair_aware) no("pair_aware");
        if (config.template_aware) no("template_aware");
        if (!config.targets_filepath.empty()) no("targets");
        if (!config.depth_report_filepath.empty()) no("a depth report");
        if (!config.depth_track_filepath.empty()) no("a depth track");
        if (!config.coverage_ladder.empty()) no("a coverage ladder");
        if (config.stratify_by != Stratify::NONE) no("stratify_by");
        if (config.dedup) no("dedup");
        primer_clip_ = config.primer_clip;
        per_amplicon_ = config.per_amplicon;
        amplicon_report_filepath_ = config.amplicon_report_filepath;
    }
    if (!config.coverage_ladder.empty()) {
        if (!per_reference_)
            throw std::invalid_argument("a coverage ladder needs per_reference: its levels are solved one reference at "
                                        "a time");
        if (!config.targets_filepath.empty())
            throw std::invalid_argument("a coverage ladder does not take targets");
        if (!config.depth_report_filepath.empty())
            throw std::invalid_argument("a coverage ladder does not take a depth report");
        for (std::size_t j = 1; j < config.coverage_ladder.size(); ++j)
            if (config.coverage_ladder[j] >= config.coverage_ladder[j - 1])
                throw std::invalid_argument("the levels of a coverage ladder must be strictly decreasing");
        if (config.coverage_ladder.back() == 0) throw std::invalid_argument("a coverage ladder ends at a coverage >= 1");
        coverage_ladder_ = config.coverage_ladder;
    }
    if (config.stratify_by != Stratify::NONE) {
        if (!per_reference_)
            throw std::invalid_argument("stratified downsampling needs per_reference: every stratum is solved one "
                                        "reference at a time");
        if (!config.targets_filepath.empty())
            throw std::invalid_argument("stratified downsampling does not take targets");
        if (!config.coverage_ladder.empty())
            throw std::invalid_argument("stratified downsampling does not take a coverage ladder");
        if (!config.depth_report_filepath.empty())
            throw std::invalid_argument("stratified downsampling does not take a depth report");
        stratify_by_ = config.stratify_by;
    }
    if (config.dedup) {
        if (!per_reference_)
            throw std::invalid_argument("duplicate-aware downsampling needs per_reference: a duplicate's cell includes "
                                        "its reference");
        if (!config.targets_filepath.empty())
            throw std::invalid_argument("duplicate-aware downsampling does not take targets");
        if (!config.coverage_ladder.empty())
            throw std::invalid_argument("duplicate-aware downsampling does not take a coverage ladder");
        if (!config.depth_report_filepath.empty())
            throw std::invalid_argument("duplicate-aware downsampling does not take a depth report");
        if (config.stratify_by != Stratify::NONE)
            throw std::invalid_argument("duplicate-aware downsampling does not take stratify_by");
        if (config.amplicons_by_reference || !config.bed_filepath.empty() || !config.tsv_filepath.empty())
            throw std::invalid_argument("duplicate-aware downsampling does not take amplicon files");
        dedup_ = true;
    }
    if (config.pair_aware) {
        if (!per_reference_)
            throw std::invalid_argument("pair-aware downsampling needs per_reference: its stages are solved one "
                                        "reference at a time");
        if (!config.targets_filepath.empty()) throw std::invalid_argument("pair-aware downsampling does not take targets");
        if (!config.coverage_ladder.empty())
            throw std::invalid_argument("pair-aware downsampling does not take a coverage ladder");
        if (!config.depth_report_filepath.empty())
            throw std::invalid_argument("pair-aware downsampling does not take a depth report");
        if (!config.depth_track_filepath.empty())
            throw std::invalid_argument("pair-aware downsampling does not take a depth track");
        if (config.stratify_by != Stratify::NONE)
            throw std::invalid_argument("pair-aware downsampling does not take stratify_by");
        if (config.dedup) throw std::invalid_argument("pair-aware downsampling does not take dedup");
        if (config.amplicons_by_reference || !config.bed_filepath.empty() || !config.tsv_filepath.empty())
            throw std::invalid_argument("pair-aware downsampling does not take amplicon files");
        pair_aware_ = true;
        pair_stages_ = config.pair_stages;
    } else if (!config.pair_stages.empty()) {
        throw std::invalid_argument("pair_stages need pair_aware");
    }
    if (config.ceiling) {
        if (!per_reference_)
            throw std::invalid_argument("ceiling downsampling needs per_reference: its ceilings are solved one reference "
                                        "at a time");
        if (config.pair_aware) throw std::invalid_argument("ceiling downsampling does not take pair_aware");
        if (config.template_aware) throw std::invalid_argument("ceiling downsampling does not take template_aware");
        if (!config.targets_filepath.empty()) throw std::invalid_argument("ceiling downsampling does not take targets");
        if (!config.coverage_ladder.empty())
            throw std::invalid_argument("ceiling downsampling does not take a coverage ladder");
        if (!config.depth_report_filepath.empty())
            throw std::invalid_argument("ceiling downsampling does not take a depth report");
        if (!config.depth_track_filepath.empty())
            throw std::invalid_argument("ceiling downsampling does not take a depth track");
        if (config.stratify_by != Stratify::NONE)
            throw std::invalid_argument("ceiling downsampling does not take stratify_by");
        if (config.dedup) throw std::invalid_argument("ceiling downsampling does not take dedup");
        if (config.amplicons_by_reference || !config.bed_filepath.empty() || !config.tsv_filepath.empty())
            throw std::invalid_argument("ceiling downsampling does not take amplicon files");
        ceiling_ = true;
    }
    if (config.budget_reads.has_value() || config.budget_fraction.has_value()) {
        if (config.budget_reads.has_value() && config.budget_fraction.has_value())
            throw std::invalid_argument("budget downsampling takes budget_reads or budget_fraction, not both");
        if (config.budget_fraction.has_value() && !(*config.budget_fraction >= 0.0 && *config.budget_fraction <= 1.0))
            throw std::invalid_argument("budget_fraction must lie in 0 .. 1");
        if (!per_reference_)
            throw std::invalid_argument("budget downsampling needs per_reference: its probes are solved one reference at "
                                        "a time");
        if (config.ceiling) throw std::invalid_argument("budget downsampling does not take ceiling");
        if (config.pair_aware) throw std::invalid_argument("budget downsampling does not take pair_aware");
        if (config.template_aware) throw std::invalid_argument("budget downsampling does not take template_aware");
        if (!config.targets_filepath.empty()) throw std::invalid_argument("budget downsampling does not take targets");
        if (!config.coverage_ladder.empty())
            throw std::invalid_argument("budget downsampling does not take a coverage ladder");
        if (!config.depth_report_filepath.empty())
            throw std::invalid_argument("budget downsampling does not take a depth report");
        if (!config.depth_track_filepath.empty())
            throw std::invalid_argument("budget downsampling does not take a depth track");
        if (config.stratify_by != Stratify::NONE)
            throw std::invalid_argument("budget downsampling does not take stratify_by");
        if (config.dedup) throw std::invalid_argument("budget downsampling does not take dedup");
        if (config.amplicons_by_reference || !config.bed_filepath.empty() || !config.tsv_filepath.empty())
            throw std::invalid_argument("budget downsampling does not take amplicon files");
        budget_reads_ = config.budget_reads;
        budget_fraction_ = config.budget_fraction;
    }
    if (config.mean_depth.has_value() || config.budget_bases.has_value()) {
        if (config.mean_depth.has_value() && config.budget_bases.has_value())
            throw std::invalid_argument("mean-depth downsampling takes mean_depth or budget_bases, not both");
        if (config.mean_depth.has_value() && !(*config.mean_depth >= 0.0 && std::isfinite(*config.mean_depth)))
            throw std::invalid_argument("mean_depth must be a finite depth of at least 0");
        if (!per_reference_)
            throw std::invalid_argument("mean-depth downsampling needs per_reference: its probes are solved one reference "
                                        "at a time");
        if (config.proportion.has_value()) throw std::invalid_argument("mean-depth downsampling does not take a proportion");
        if (config.replicates.has_value()) throw std::invalid_argument("mean-depth downsampling does not take replicates");
        if (config.budget_reads.has_value() || config.budget_fraction.has_value())
            throw std::invalid_argument("mean-depth downsampling does not take a budget");
        if (config.ceiling) throw std::invalid_argument("mean-depth downsampling does not take ceiling");
        if (config.pair_aware) throw std::invalid_argument("mean-depth downsampling does not take pair_aware");
        if (config.template_aware) throw std::invalid_argument("mean-depth downsampling does not take template_aware");
        if (!config.targets_filepath.empty()) throw std::invalid_argument("mean-depth downsampling does not take targets");
        if (!config.coverage_ladder.empty())
            throw std::invalid_argument("mean-depth downsampling does not take a coverage ladder");
        if (!config.depth_report_filepath.empty())
            throw std::invalid_argument("mean-depth downsampling does not take a depth report");
        if (!config.depth_track_filepath.empty())
            throw std::invalid_argument("mean-depth downsampling does not take a depth track");
        if (config.stratify_by != Stratify::NONE)
            throw std::invalid_argument("mean-depth downsampling does not take stratify_by");
        if (config.dedup) throw std::invalid_argument("mean-depth downsampling does not take dedup");
        if (config.amplicons_by_reference || !config.bed_filepath.empty() || !config.tsv_filepath.empty())
            throw std::invalid_argument("mean-depth downsampling does not take amplicon files");
        mean_depth_ = config.mean_depth;
        budget_bases_ = config.budget_bases;
        if (!config.mean_depth_targets_filepath.empty()) {
            std::vector<std::string> names;
            std::vector<std::uint32_t> lengths;
            std::string err;
            if (!read_bam_references(input_filepath_, names, lengths, &err)) {
                std::fprintf(stderr, "[ERROR] %s\n", err.c_str());
                std::exit(EXIT_FAILURE);  // (as read_bam_into on an unreadable input)
            }
            if (!target_regions_from_bed(config.mean_depth_targets_filepath, names, mean_depth_regions_, &err))
                throw std::invalid_argument(err);
            has_mean_depth_regions_ = true;
        }
    } else if (!config.mean_depth_targets_filepath.empty()) {
        throw std::invalid_argument("mean_depth_targets need mean_depth or budget_bases");
    }
    if (config.replicates.has_value()) {
        if (!per_reference_)
            throw std::invalid_argument("disjoint replicates need per_reference: every replicate is solved one reference "
                                        "at a time");
        if (config.budget_reads.has_value() || config.budget_fraction.has_value())
            throw std::invalid_argument("disjoint replicates do not take a budget");
        if (config.ceiling) throw std::invalid_argument("disjoint replicates do not take ceiling");
        if (config.pair_aware) throw std::invalid_argument("disjoint replicates do not take pair_aware");
        if (config.template_aware) throw std::invalid_argument("disjoint replicates do not take template_aware");
        if (!config.targets_filepath.empty()) throw std::invalid_argument("disjoint replicates do not take targets");
        if (!config.coverage_ladder.empty()) throw std::invalid_argument("disjoint replicates do not take a coverage ladder");
        if (!config.depth_report_filepath.empty())
            throw std::invalid_argument("disjoint replicates do not take a depth report");
        if (!config.depth_track_filepath.empty()) throw std::invalid_argument("disjoint replicates do not take a depth track");
        if (config.stratify_by != Stratify::NONE) throw std::invalid_argument("disjoint replicates do not take stratify_by");
        if (config.dedup) throw std::invalid_argument("disjoint replicates do not take dedup");
        if (config.amplicons_by_reference || !config.bed_filepath.empty() || !config.tsv_filepath.empty())
            throw std::invalid_argument("disjoint replicates do not take amplicon files");
        if (config.replicates->size() > 15)
            throw std::invalid_argument("disjoint replicates: at most 16 replicates in one call");
        for (std::uint32_t cov : *config.replicates)
            if (cov == 0 || cov >= (1u << 31))
                throw std::invalid_argument("disjoint replicates: every coverage must lie in 1 .. 2^31 - 1");
        replicates_ = config.replicates;
    }
    if (config.proportion.has_value()) {
        const BamApiConfig::Proportion& f = *config.proportion;
        if (f.den == 0 || f.num > f.den) throw std::invalid_argument("proportion must lie in 0 .. 1");
        if (f.den > (1u << 20)) throw std::invalid_argument("proportion: the denominator must not exceed 2^20");
        if (!per_reference_)
            throw std::invalid_argument("proportional downsampling needs per_reference: its fractions are solved one "
                                        "reference at a time");
        if (config.replicates.has_value()) throw std::invalid_argument("proportional downsampling does not take replicates");
        if (config.budget_reads.has_value() || config.budget_fraction.has_value())
            throw std::invalid_argument("proportional downsampling does not take a budget");
        if (config.ceiling) throw std::invalid_argument("proportional downsampling does not take ceiling");
        if (config.pair_aware) throw std::invalid_argument("proportional downsampling does not take pair_aware");
        if (config.template_aware) throw std::invalid_argument("proportional downsampling does not take template_aware");
        if (!config.targets_filepath.empty()) throw std::invalid_argument("proportional downsampling does not take targets");
        if (!config.coverage_ladder.empty())
            throw std::invalid_argument("proportional downsampling does not take a coverage ladder");
        if (!config.depth_report_filepath.empty())
            throw std::invalid_argument("proportional downsampling does not take a depth report");
        if (!config.depth_track_filepath.empty())
            throw std::invalid_argument("proportional downsampling does not take a depth track");
        if (config.stratify_by != Stratify::NONE)
            throw std::invalid_argument("proportional downsampling does not take stratify_by");
        if (config.dedup) throw std::invalid_argument("proportional downsampling does not take dedup");
        if (config.amplicons_by_reference || !config.bed_filepath.empty() || !config.tsv_filepath.empty())
            throw std::invalid_argument("proportional downsampling does not take amplicon files");
        proportion_ = config.proportion;
    }
    if (config.thresholds_hi.has_value()) {
        const auto no = [](const char* what) { throw std::invalid_argument(std::string("coverage thresholds do not take ") + what); };
        if (config.thresholds_lo == 0 || config.thresholds_lo > *config.thresholds_hi || *config.thresholds_hi > 65534u)
            throw std::invalid_argument("coverage thresholds need 1 <= thresholds_lo <= thresholds_hi <= 65534");
        const std::string& tag = config.thresholds_tag;
        const auto alpha = [](char ch) { return (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z'); };
        if (tag.size() != 2 || !alpha(tag[0]) || !(alpha(tag[1]) || (tag[1] >= '0' && tag[1] <= '9')))
            throw std::invalid_argument("thresholds_tag must be [A-Za-z][A-Za-z0-9]");
        if (!per_reference_)
            throw std::invalid_argument("coverage thresholds need per_reference: every coverage is solved one reference at "
                                        "a time");
        if (config.proportion.has_value()) no("a proportion");
        if (config.mean_depth.has_value() || config.budget_bases.has_value()) no("a mean depth");
        if (config.replicates.has_value()) no("replicates");
        if (config.budget_reads.has_value() || config.budget_fraction.has_value()) no("a budget");
        if (config.ceiling) no("ceiling");
        if (config.pair_aware) no("pair_aware");
        if (config.template_aware) no("template_aware");
        if (!config.targets_filepath.empty()) no("targets");
        if (!config.coverage_ladder.empty()) no("a coverage ladder");
        if (!config.depth_report_filepath.empty()) no("a depth report");
        if (!config.depth_track_filepath.empty()) no("a depth track");
        if (config.stratify_by != Stratify::NONE) no("stratify_by");
        if (config.dedup) no("dedup");
        if (config.amplicons_by_reference || !config.bed_filepath.empty() || !config.tsv_filepath.empty()) no("amplicon files");
        thresholds_lo_ = config.thresholds_lo;
        thresholds_hi_ = config.thresholds_hi;
        thresholds_tag_ = config.thresholds_tag;
    }
    if (config.template_aware) {
        if (!per_reference_)
            throw std::invalid_argument("template-aware downsampling needs per_reference: its stages are solved one "
                                        "reference at a time");
        if (config.pair_aware) throw std::invalid_argument("template-aware downsampling does not take pair_aware");
        if (!config.targets_filepath.empty())
            throw std::invalid_argument("template-aware downsampling does not take targets");
        if (!config.coverage_ladder.empty())
            throw std::invalid_argument("template-aware downsampling does not take a coverage ladder");
        if (!config.depth_report_filepath.empty())
            throw std::invalid_argument("template-aware downsampling does not take a depth report");
        if (!config.depth_track_filepath.empty())
            throw std::invalid_argument("template-aware downsampling does not take a depth track");
        if (config.stratify_by != Stratify::NONE)
            throw std::invalid_argument("template-aware downsampling does not take stratify_by");
        if (config.dedup) throw std::invalid_argument("template-aware downsampling does not take dedup");
        if (config.amplicons_by_reference || !config.bed_filepath.empty() || !config.tsv_filepath.empty())
            throw std::invalid_argument("template-aware downsampling does not take amplicon files");
        template_aware_ = true;
        split_spliced_ = config.split_spliced;
        include_secondary_ = config.include_secondary;
        template_stages_ = config.template_stages;
        fragment_depth_ = config.fragment_depth;
    } else if (config.fragment_depth) {
        throw std::invalid_argument("fragment_depth needs template_aware");
    } else if (!config.template_stages.empty() || !config.split_spliced || config.include_secondary) {
        throw std::invalid_argument("template_stages, split_spliced and include_secondary need template_aware");
    }
    if (!config.depth_report_filepath.empty()) {
        if (!per_reference_)
            throw std::invalid_argument("a depth report needs per_reference: its rows are the references a per-reference "
                                        "ingest keeps");
        depth_report_filepath_ = config.depth_report_filepath;
        depth_report_bins_ = config.depth_report_bins;
    }
    if (!config.depth_track_filepath.empty()) {
        if (!per_reference_)
            throw std::invalid_argument("a depth track needs per_reference: its runs lie on the references a "
                                        "per-reference ingest keeps");
        if (!config.coverage_ladder.empty()) throw std::invalid_argument("a coverage ladder does not take a depth track");
        if (config.stratify_by != Stratify::NONE)
            throw std::invalid_argument("stratified downsampling does not take a depth track");
        if (config.dedup) throw std::invalid_argument("duplicate-aware downsampling does not take a depth track");
        if (config.depth_track_channel != "kept" && config.depth_track_channel != "in" &&
            config.depth_track_channel != "both")
            throw std::invalid_argument("the channel of a depth track is \"kept\", \"in\" or \"both\"");
        depth_track_filepath_ = config.depth_track_filepath;
        depth_track_channel_ = config.depth_track_channel;
        depth_track_cap_ = config.depth_track_cap;
    }
    if (!config.targets_filepath.empty()) {
        if (!per_reference_)
            throw std::invalid_argument("targets need per_reference: target regions are matched to the references a "
                                        "per-reference ingest keeps");
        std::vector<std::string> names;
        std::vector<std::uint32_t> lengths;
        std::string err;
        if (!read_bam_references(input_filepath_, names, lengths, &err)) {
            std::fprintf(stderr, "[ERROR] %s\n", err.c_str());
            std::exit(EXIT_FAILURE);  // (as read_bam_into on an unreadable input)
        }
        if (!target_regions_from_bed(config.targets_filepath, names, targets_, &err)) throw std::invalid_argument(err);
        targets_.padding = config.target_padding;
        targets_.keep_off_target = config.keep_off_target;
        has_targets_ = true;
    }
    if (per_reference_ && !amplicons_by_reference_ && (!config.bed_filepath.empty() || !config.tsv_filepath.empty()))
        throw std::invalid_argument("per-reference downsampling does not take amplicons (BED / TSV) yet: amplicons "
                                    "are not matched to references by name");
    if (amplicons_by_reference_) {
        if (!config.bed_filepath.empty()) {
            // the BED's chroms are matched to the header's reference names, so the header is read first
            std::vector<std::string> names;
            std::vector<std::uint32_t> lengths;
            std::string err;
            if (!read_bam_references(input_filepath_, names, lengths, &err)) {
                std::fprintf(stderr, "[ERROR] %s\n", err.c_str());
                std::exit(EXIT_FAILURE);  // (as read_bam_into on an unreadable input)
            }
            if (!reference_amplicon_set_from_files(config.bed_filepath, config.tsv_filepath, names,
                                                   reference_amplicon_set_, &err))
                throw std::invalid_argument(err);
            if (primer_clip_ && !reference_amplicon_set_.empty_insert.empty())
                throw std::invalid_argument(reference_amplicon_set_.empty_insert);
            amplicon_behaviour_ = config.amplicon_behaviour;
        }
        return;
    }
    if (!config.bed_filepath.empty()) {
        if (!amplicon_set_from_files(config.bed_filepath, config.tsv_filepath, amplicon_set_)) {
            std::fprintf(stderr, "[ERROR] could not open %s\n", config.bed_filepath.c_str());
            std::exit(EXIT_FAILURE);  // the reference exits the process on an unreadable input
        }
        amplicon_behaviour_ = config.amplicon_behaviour;
    }
}

void BamApi::read_bam_into(PairedReads& reads) {
    BamFilters f;
    f.min_seq_length = min_seq_length_;
    f.min_mapq = min_mapq_;
    f.amplicon_behaviour = amplicon_behaviour_;
    f.amplicons = &amplicon_set_;
    f.per_reference = per_reference_;
    // (dedup: the strand bit is the duplicate cell's tag; a start cap by strand: it is the start site's group)
    f.stratify = dedup_ || start_cap_by_strand_ ? Stratify::STRAND : stratify_by_;
    if (amplicons_by_reference_) f.reference_amplicons = &reference_amplicon_set_;
    std::string err;
    if (!read_bam(input_filepath_, f, reads, filtered_out_reads_, nullptr, &err)) {
        std::fprintf(stderr, "[ERROR] %s\n", err.c_str());
        std::exit(EXIT_FAILURE);
    }
}

const TemplateSegments& BamApi::get_template_segments() {
    if (!are_segments_loaded_) {
        if (!template_aware_) throw std::invalid_argument("segments need a BamApi built with BamApiConfig::template_aware");
        TemplateIngest cfg;
        cfg.min_seq_length = min_seq_length_;
        cfg.min_mapq = min_mapq_;
        cfg.split_spliced = split_spliced_;
        cfg.include_secondary = include_secondary_;
        std::string err;
        if (!read_bam_templates(input_filepath_, cfg, template_segments_, filtered_out_reads_, &err)) {
            std::fprintf(stderr, "[ERROR] %s\n", err.c_str());
            std::exit(EXIT_FAILURE);
        }
        are_segments_loaded_ = true;
    }
    return template_segments_;
}

std::uint32_t BamApi::write_records(const std::filesystem::path& output_filepath, std::vector<BAMReadId>& bam_ids) const {
    std::string err;
    const std::uint32_t n = write_bam(input_filepath_, output_filepath, bam_ids, &err);
    if (n == UINT32_MAX) { std::fprintf(stderr, "[ERROR] %s\n", err.c_str()); std::exit(EXIT_FAILURE); }
    return n;
}

std::uint32_t BamApi::write_paired_reads(const std::filesystem::path& output_filepath,
                                         std::vector<ReadIndex>& active_ids) const {
    const PairedReads& reads = get_paired_reads();
    std::vector<BAMReadId> bam_ids;
    bam_ids.reserve(active_ids.size());
    for (ReadIndex id : active_ids) bam_ids.push_back(reads.get_read_by_index(id).bam_id);
    std::string err;
    const std::uint32_t n = write_bam(input_filepath_, output_filepath, bam_ids, &err);
    if (n == UINT32_MAX) { std::fprintf(stderr, "[ERROR] %s\n", err.c_str()); std::exit(EXIT_FAILURE); }
    return n;
}

std::uint32_t BamApi::write_tagged_reads(const std::filesystem::path& output_filepath,
                                         const std::vector<ReadIndex>& active_ids, const std::vector<std::uint16_t>& values,
                                         const std::string& tag) const {
    if (values.size() != active_ids.size()) throw std::invalid_argument("write_tagged_reads needs one value per read");
    const PairedReads& reads = get_paired_reads();
    std::vector<std::pair<BAMReadId, std::uint16_t>> tagged;
    tagged.reserve(active_ids.size());
    for (std::size_t k = 0; k < active_ids.size(); ++k)
        tagged.emplace_back(reads.get_read_by_index(active_ids[k]).bam_id, values[k]);
    std::string err;
    const std::uint32_t n = write_bam_tagged(input_filepath_, output_filepath, tagged, tag, &err);
    if (n == UINT32_MAX) throw std::invalid_argument(err);
    return n;
}

std::uint32_t BamApi::write_bam_api_filtered_out_reads(const std::filesystem::path& output_filepath) {
    std::string err;
    const std::uint32_t n = write_bam(input_filepath_, output_filepath, filtered_out_reads_, &err);
    if (n == UINT32_MAX) { std::fprintf(stderr, "[ERROR] %s\n", err.c_str()); std::exit(EXIT_FAILURE); }
    return n;
}

BamApi::BamApi(const AOSPairedReads& paired_reads)
    : aos_paired_reads_(paired_reads), is_aos_loaded_(true) {}

BamApi::BamApi(const SOAPairedReads& paired_reads)
    : soa_paired_reads_(paired_reads), is_soa_loaded_(true) {}

// The reference converts lazily between layouts on first request of the other one
// (bam_api.cpp:189-233); same here.
const AOSPairedReads& BamApi::get_paired_reads_aos() {
    if (!is_aos_loaded_) {
        if (is_soa_loaded_ || input_filepath_.empty()) aos_paired_reads_.from(soa_paired_reads_);
        else read_bam_into(aos_paired_reads_);
        is_aos_loaded_ = true;
    }
    return aos_paired_reads_;
}

const SOAPairedReads& BamApi::get_paired_reads_soa() {
    if (!is_soa_loaded_) {
        if (is_aos_loaded_ || input_filepath_.empty()) soa_paired_reads_.from(aos_paired_reads_);
        else read_bam_into(soa_paired_reads_);
        is_soa_loaded_ = true;
    }
    return soa_paired_reads_;
}

const PairedReads& BamApi::get_paired_reads() const {
    if (is_soa_loaded_) return soa_paired_reads_;
    return aos_paired_reads_;
}

// bam_api.cpp:239-273: output keeps first-seen order: id, then its mate, de-duplicated.
std::vector<ReadIndex> BamApi::find_pairs(const std::vector<ReadIndex>& ids) const {
    const PairedReads& reads = get_paired_reads();
    const ReadIndex n = reads.get_reads_count();
    std::vector<ReadIndex> out;
    out.reserve(n);
    std::vector<bool> seen(n, false);
    for (ReadIndex id : ids) {
        if (!seen[id]) { seen[id] = true; out.push_back(id); }
        const ReadIndex mate = reads.get_read_by_index(id).is_first_read ? id + 1 : id - 1;
        if (!seen[mate]) { seen[mate] = true; out.push_back(mate); }
    }
    return out;
}

std::vector<std::uint32_t> BamApi::find_input_cover() {
    const PairedReads& reads = get_paired_reads();
    std::vector<std::uint32_t> cover(reads.ref_genome_length, 0);
    for (ReadIndex i = 0; i < reads.get_reads_count(); ++i) {
        const Read r = reads.get_read_by_index(i);
        for (Index p = r.start_ind; p <= r.end_ind; ++p) ++cover[p];
    }
    return cover;
}

std::vector<std::uint32_t> BamApi::find_filtered_cover(const std::vector<ReadIndex>& ids) {
    const PairedReads& reads = get_paired_reads();
    std::vector<std::uint32_t> cover(reads.ref_genome_length, 0);
    for (ReadIndex id : ids) {
        const Read r = reads.get_read_by_index(id);
        for (Index p = r.start_ind; p <= r.end_ind; ++p) ++cover[p];
    }
    return cover;
}

std::uint64_t BamApi::budget_for(std::uint64_t placed_reads) const {
    if (budget_reads_.has_value()) return *budget_reads_;
    if (!budget_fraction_.has_value()) throw std::invalid_argument("this BamApi was built without a budget");
    const double want = std::floor(*budget_fraction_ * static_cast<double>(placed_reads));
    return std::min(static_cast<std::uint64_t>(want), placed_reads);
}

// the regions clipped to their references (one that begins at or beyond the reference's length is dropped) and merged,
// as qmcp_hip_solve_mean_depth_host counts them
std::uint64_t BamApi::mean_depth_positions(const std::vector<std::uint32_t>& contig_lengths) const {
    std::uint64_t total = 0;
    if (!has_mean_depth_regions_) {
        for (std::uint32_t l : contig_lengths) total += l;
        return total;
    }
    const TargetRegions& t = mean_depth_regions_;
    std::vector<std::pair<std::uint64_t, std::uint64_t>> spans;
    for (std::size_t c = 0; c + 1 < t.offsets.size() && c < contig_lengths.size(); ++c) {
        const std::uint64_t len = contig_lengths[c];
        spans.clear();
        for (std::uint32_t k = t.offsets[c]; k < t.offsets[c + 1]; ++k)
            if (t.starts[k] < len) spans.emplace_back(t.starts[k], std::min<std::uint64_t>(t.ends[k], len - 1));
        std::sort(spans.begin(), spans.end());
        std::uint64_t next = 0;  // the first position not counted yet
        for (const auto& s : spans)
            if (s.second >= next) {
                total += s.second - std::max(s.first, next) + 1;
                next = s.second + 1;
            }
    }
    return total;
}

std::uint64_t BamApi::base_budget_for(std::uint64_t positions) const {
    if (budget_bases_.has_value()) return *budget_bases_;
    if (!mean_depth_.has_value()) throw std::invalid_argument("this BamApi was built without a mean depth");
    const double want = std::floor(*mean_depth_ * static_cast<double>(positions));
    if (want >= 18446744073709551616.0) throw std::invalid_argument("mean_depth * positions exceeds 64 bits");
    return static_cast<std::uint64_t>(want);
}

}  // namespace bam_api
