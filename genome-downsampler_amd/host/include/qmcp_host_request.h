/* The file-to-file downsample request of libqmcp_host.so: one plain struct that names every BamApiConfig knob of the
 * flow, and the one entry that takes it.  C99; the bridge is private to the package (the ctypes mirror is
 * DownsampleRequest in genome-downsampler_amd/__init__.py) -- integrations use BamApiConfig and QuasiMcpHipSolver.
 *
 * A zeroed request with struct_size, solver_name, in_path, out_path and max_coverage set is the reference's plain flow,
 * but for three fields whose "not given" is not zero: amplicon_mode (-1), split_spliced (1) and budget_fraction (< 0).
 * Every pointer may be NULL; a path that is NULL or "" is not given; an array is a pointer and a count. */
#ifndef QMCP_HOST_REQUEST_H
#define QMCP_HOST_REQUEST_H

#include <stddef.h>
#include <stdint.h>

#include "qmcp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qmcp_host_downsample_request {
    uint64_t struct_size; /* sizeof(qmcp_host_downsample_request); a request of another size is refused */
    const char* solver_name;
    const char* in_path;
    const char* out_path;
    const char* filtered_path; /* the records the ingest filters dropped */
    /* amplicons (BamApiConfig::bed_filepath, tsv_filepath, amplicon_behaviour, amplicons_by_reference) */
    const char* bed;
    const char* tsv;
    /* on-target downsampling (targets_filepath, target_padding, keep_off_target) */
    const char* targets;
    /* depth report and depth track, written after the output (depth_report_*, depth_track_*) */
    const char* report;
    const char* track;
    const char* track_channel; /* "kept" (also NULL), "in" or "both" */
    /* coverage ladder (coverage_ladder): level j to ladder_template with its "{M}" replaced by the coverage */
    const uint32_t* ladder_levels;
    const char* ladder_template;
    /* stratified downsampling (stratify_by): "strand" or "read_group" */
    const char* stratify;
    const char* strata_report;
    const char* dedup_report;
    /* a cap per region, CSR per reference of the file: n_refs + 1 offsets.  Alone it is a coverage profile with
     * max_coverage elsewhere; with ceiling the caps are ceilings; with template_aware it is the cap table of whole
     * templates, default_cap elsewhere.  has_regions says whether the table is given at all. */
    const uint32_t* region_offsets;
    const uint32_t* region_starts;
    const uint32_t* region_ends;
    const uint32_t* region_caps;
    uint64_t n_refs;
    /* the staged solves (pair_stages, template_stages); no stages: the default schedule */
    const uint32_t* pair_stages;
    const uint32_t* template_stages;
    /* fragment depth (fragment_depth, with template_aware): stat<TAB>value lines of the qmcp_hip_fragment_stats and
     * records_written, written by the host itself */
    const char* fragment_report;
    const char* ceiling_report;
    /* budget downsampling (budget_reads, budget_fraction): has_budget_reads != 0 and / or budget_fraction >= 0 ask for
     * it; budget_report alone is refused */
    const char* budget_report;
    uint64_t budget_reads;
    double budget_fraction;
    /* mean-depth downsampling (mean_depth, budget_bases, mean_depth_targets_filepath): has_mean_depth != 0 and / or
     * has_budget_bases != 0 ask for it; mean_depth_targets (a BED3+ file: the regions the bases are counted in) and
     * mean_depth_report (stat<TAB>value lines, then the curve S_R) alone are refused */
    const char* mean_depth_targets;
    const char* mean_depth_report;
    uint64_t budget_bases;
    double mean_depth;
    /* coverage thresholds (thresholds_lo, thresholds_hi, thresholds_tag): has_thresholds != 0 asks for them -- every
     * written record gets the aux field <thresholds_tag>:S:<the smallest coverage in thresholds_lo .. thresholds_hi that
     * keeps its pair>, and the records without one are not written; max_coverage is not used.  thresholds_tag NULL or
     * "": "XC".  thresholds_report: stat<TAB>value lines, then one M<TAB>reads line per coverage.  thresholds_tag or
     * thresholds_report alone are refused */
    const char* thresholds_tag;
    const char* thresholds_report;
    /* disjoint replicates (replicates): has_replicates != 0 asks for them, replicate r + 2 at replicates_further[r],
     * written to replicates_template with its "{R}" replaced */
    const uint32_t* replicates_further;
    const char* replicates_template;
    const char* replicates_report;

    uint32_t max_coverage;
    uint32_t min_len;
    uint32_t min_mapq;
    uint32_t target_padding;
    uint32_t report_bins;
    uint32_t track_cap;
    uint32_t n_ladder_levels;
    uint32_t default_cap;
    uint32_t n_pair_stages;
    uint32_t n_template_stages;
    uint32_t n_replicates_further;
    uint32_t thresholds_lo;
    uint32_t thresholds_hi;
    int32_t amplicon_mode; /* 0 IGNORE, 1 FILTER, 2 GRADE, -1: GRADE for a solver that grades by quality, else FILTER */
    int32_t per_reference;
    int32_t amplicons_by_reference;
    int32_t keep_off_target;
    int32_t dedup;
    int32_t has_regions;
    int32_t pair_aware;
    int32_t template_aware;
    int32_t split_spliced;
    int32_t include_secondary;
    int32_t fragment_depth;
    int32_t ceiling;
    int32_t has_budget_reads;
    int32_t has_budget_bases;
    int32_t has_mean_depth;
    int32_t has_replicates;
    int32_t has_thresholds;
    /* start cap (start_cap, start_cap_by_strand): start_cap != 0 asks for it -- every (reference, start) site, with
     * start_cap_by_strand every (reference, start, strand), offers the solve at most start_cap reads (highest MAPQ, then
     * longest, then first); start_cap_report: stat<TAB>value lines, then one size<TAB>cells line per bin of the cell-size
     * histogram.  start_cap_by_strand or start_cap_report alone are refused.  (The request ends with the proportion
     * fields: these three stand in front of them.) */
    int32_t start_cap_by_strand;
    uint32_t start_cap;
    const char* start_cap_report;
    /* amplicon-aware downsampling (primer_clip, per_amplicon, amplicon_report): primer_clip != 0 counts depth on the
     * reads clipped to their amplicon's insert, per_amplicon != 0 solves every amplicon as a coverage problem of its
     * own; amplicon_report: one line per amplicon (chrom, amplicon, insert, left primer, units, reads kept, minimum
     * and mean insert depth before and after, deficit positions); the report alone runs with clipping off, pooled.
     * They need bed, per_reference and amplicons_by_reference and go with no other mode.  (These three stand in front
     * of the proportion fields too.) */
    int32_t primer_clip;
    int32_t per_amplicon;
    const char* amplicon_report;
    /* tiered downsampling by MAPQ band (mapq_tiers): n_mapq_tiers strictly falling thresholds ask for it -- the best
     * band is solved first, a lower band only fills what the better ones leave short of min(coverage, max_coverage);
     * the last threshold must equal min_mapq.  tiers_report: one line per tier (band, reads, kept, mean depth before
     * and after, demand, asked positions), then records_written and mates_added; alone it is refused.  It needs
     * per_reference and goes with no other mode.  (These three stand in front of the proportion fields too.) */
    const uint32_t* mapq_tiers;
    uint32_t n_mapq_tiers;
    const char* tiers_report;
    /* proportional downsampling (proportion): has_proportion != 0 asks for it -- every position keeps
     * ceil(cov * proportion_num / proportion_den) of its depth, positions at or below proportion_floor whole,
     * max_coverage the hard upper end; proportional_report: stat<TAB>value lines */
    const char* proportional_report;
    uint32_t proportion_num;
    uint32_t proportion_den;
    uint32_t proportion_floor;
    int32_t has_proportion;
} qmcp_host_downsample_request;

/* BamApi(in_path, the request's BamApiConfig) -> the solve the configuration selects -> the output file(s) -> the
 * filtered-out file -> the stats -> the reports.  written_out (written_cap entries, may be NULL) receives each output
 * file's record count, out_path's first; the stats pointers may be NULL and are written only by the mode they belong
 * to.  Returns the records written -- for a ladder and for replicates the files written --, -1 for an unknown solver,
 * -3 out of memory, -4 when the request is refused (message in err), -5 when a report or track cannot be written. */
int64_t qmcp_host_downsample_bam(const qmcp_host_downsample_request* request, int64_t* written_out, uint64_t written_cap,
                                 qmcp_hip_ceiling_stats* ceiling_stats, qmcp_hip_budget_stats* budget_stats,
                                 qmcp_hip_replicates_stats* replicates_stats, qmcp_hip_template_stats* template_stats,
                                 qmcp_hip_template_profile_stats* template_profile_stats, char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif

#endif
