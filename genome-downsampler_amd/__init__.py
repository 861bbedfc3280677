"""ctypes binding of the MI355X quasi-MCP solver (C ABI: include/qmcp_hip.h).

The directory name has a hyphen, so import it with
``importlib.import_module("genome-downsampler_amd")`` (the repo root on sys.path) or through
``__graft_entry__.load_package()``.

There is no CPU fallback anywhere in this package: if the HIP library is missing it raises at
import, and without a GPU every solver call raises :class:`QmcpError`.
"""
import contextlib
import ctypes as C
import fractions
import heapq
import math
import numbers
import operator
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
# (QMCP_HIP_LIB: another build of the same library -- lab/variants/<name>/libqmcp_hip.so -- instead of the product's;
#  lab use only: the host mirror library still links the product's)
HIP_LIB_PATH = os.environ.get("QMCP_HIP_LIB") or os.path.join(LIB_DIR, "libqmcp_hip.so")
HOST_LIB_PATH = os.environ.get("QMCP_HOST_LIB") or os.path.join(LIB_DIR, "libqmcp_host.so")  # (e.g. a sanitizer build of the host mirror)

# every symbol include/qmcp_hip.h declares
ABI_SYMBOLS = (
    "qmcp_hip_abi_version", "qmcp_hip_last_error", "qmcp_hip_device_count", "qmcp_hip_create",
    "qmcp_hip_destroy", "qmcp_hip_solve_host", "qmcp_hip_solve_device", "qmcp_hip_coverage_host",
    "qmcp_hip_filtered_coverage_host", "qmcp_hip_complete_pairs_device",
    "qmcp_hip_complete_pairs_host", "qmcp_hip_amplicon_filter_host", "qmcp_hip_set_profiling",
    "qmcp_hip_kernel_times", "qmcp_hip_filter_solve_host", "qmcp_hip_solve_device_begin",
    "qmcp_hip_solve_end", "qmcp_hip_demand_host", "qmcp_hip_solve_host64", "qmcp_hip_multi_create",
    "qmcp_hip_multi_destroy", "qmcp_hip_multi_solve_host", "qmcp_hip_kept_indices_host",
    "qmcp_hip_default_options", "qmcp_hip_set_options", "qmcp_hip_get_options",
    "qmcp_hip_solve_by_contig_host", "qmcp_hip_solve_by_contig_device", "qmcp_hip_filter_solve_by_contig_host",
    "qmcp_hip_solve_quality_host", "qmcp_hip_solve_quality_device", "qmcp_hip_solve_quality_by_contig_host",
    "qmcp_hip_solve_targets_host", "qmcp_hip_solve_targets_device",
    "qmcp_hip_depth_report_host", "qmcp_hip_depth_report_device",
    "qmcp_hip_depth_track_host", "qmcp_hip_depth_track_device",
    "qmcp_hip_solve_ladder_host", "qmcp_hip_solve_ladder_device",
    "qmcp_hip_solve_stratified_host", "qmcp_hip_solve_stratified_device",
    "qmcp_hip_solve_dedup_host", "qmcp_hip_solve_dedup_device",
    "qmcp_hip_solve_profile_host", "qmcp_hip_solve_profile_device",
    "qmcp_hip_solve_pairs_host", "qmcp_hip_solve_pairs_device",
    "qmcp_hip_solve_templates_host", "qmcp_hip_solve_templates_device",
    "qmcp_hip_solve_templates_profile_host", "qmcp_hip_solve_templates_profile_device",
    "qmcp_hip_clip_templates_host", "qmcp_hip_clip_templates_device",
    "qmcp_hip_solve_fragments_host", "qmcp_hip_solve_fragments_device",
    "qmcp_hip_solve_ceiling_host", "qmcp_hip_solve_ceiling_device",
    "qmcp_hip_solve_budget_host", "qmcp_hip_solve_budget_device",
    "qmcp_hip_solve_mean_depth_host", "qmcp_hip_solve_mean_depth_device",
    "qmcp_hip_solve_thresholds_host", "qmcp_hip_solve_thresholds_device",
    "qmcp_hip_solve_replicates_host", "qmcp_hip_solve_replicates_device",
    "qmcp_hip_solve_proportional_host", "qmcp_hip_solve_proportional_device",
    "qmcp_hip_solve_start_cap_host", "qmcp_hip_solve_start_cap_device",
    "qmcp_hip_solve_amplicons_host", "qmcp_hip_solve_amplicons_device",
    "qmcp_hip_solve_tiers_host", "qmcp_hip_solve_tiers_device",
)

QMCP_OK = 0
PATH_UNIFORM, PATH_GENERAL, PATH_NEAR_UNIFORM = 1, 2, 3
KIND_UNIFORM, KIND_LOW_BOTH_SIDES, KIND_HOLE, KIND_ZERO_BOTH_SIDES = 0, 1, 2, 3
NO_CONTIG = 0xFFFFFFFF  # QMCP_NO_CONTIG: an unplaced read's contig id (never kept)
TARGETS_KEEP_OFF_TARGET = 1  # QMCP_TARGETS_KEEP_OFF_TARGET
LADDER_MAX_LEVELS = 16  # QMCP_LADDER_MAX_LEVELS
PAIR_MAX_STAGES = 16  # QMCP_PAIR_MAX_STAGES
CEILING_WHOLE_PAIRS = 1  # QMCP_CEILING_WHOLE_PAIRS
BUDGET_WHOLE_PAIRS = 1  # QMCP_BUDGET_WHOLE_PAIRS
BUDGET_CURVE_MAX = 8191  # QMCP_BUDGET_CURVE_MAX: the last coverage the curve of a budget solve reaches
MEAN_DEPTH_WHOLE_PAIRS = 1  # QMCP_MEAN_DEPTH_WHOLE_PAIRS
THRESHOLD_NEVER = 0xFFFF  # QMCP_THRESHOLD_NEVER: the threshold of a read that no coverage of the range keeps
THRESHOLDS_COVERAGE_MAX = 65534  # QMCP_THRESHOLDS_COVERAGE_MAX
THRESHOLDS_WHOLE_PAIRS = 1  # QMCP_THRESHOLDS_WHOLE_PAIRS
PROPORTION_DEN_MAX = 1 << 20  # QMCP_PROPORTION_DEN_MAX: the largest denominator of a proportional solve's fraction
REPLICATES_MAX = 16  # QMCP_REPLICATES_MAX
REPLICATES_WHOLE_PAIRS, REPLICATES_SHORTFALL = 1, 2  # QMCP_REPLICATES_*
NO_STRATUM = 0xFFFFFFFF  # QMCP_NO_STRATUM: the stratum id of a read that belongs to no stratum (never kept)
DEDUP_PAIRS, DEDUP_COMPLETE_PAIRS = 1, 2  # QMCP_DEDUP_PAIRS, QMCP_DEDUP_COMPLETE_PAIRS
DEDUP_REPORT_BINS = 64  # family-size bins of downsample_bam(dedup_report=)
START_CAP_SHORTFALL = 1  # QMCP_START_CAP_SHORTFALL
START_CAP_REPORT_BINS = 64  # cell-size bins of downsample_bam(start_cap_report=)
AMPLICONS_SINGLE_END, AMPLICONS_PER_AMPLICON, AMPLICONS_COMPLETE_PAIRS = 1, 2, 4  # QMCP_AMPLICONS_*
NO_AMPLICON = 0xFFFFFFFF  # QMCP_NO_AMPLICON: the label of a unit that no amplicon contains
AMPLICON_LDS_MAX = 2560  # qmcp::kAcLdsMax: the largest amplicon table the assign kernel stages in LDS
TRACK_IN, TRACK_KEPT, TRACK_SHORT_ONLY, TRACK_SKIP_ZERO = 1, 2, 4, 8  # QMCP_TRACK_*
TRACK_FIRST_CAPACITY = 1 << 22  # records Solver.depth_track offers first (96 MiB); beyond it, one more call at the exact count
NO_TIER = 0xFFFFFFFF  # QMCP_NO_TIER: the tier of a read that belongs to no tier (never kept)
TIERS_MAX = 16  # QMCP_TIERS_MAX
STRATUM_TALLY_TILE = 1024  # qmcp::kStratumTallyTile: the grouped records one workgroup of k_st_tally reduces


# status codes of include/qmcp_hip.h
QMCP_OK, QMCP_EINVAL, QMCP_EREAD, QMCP_ERANGE, QMCP_ENODEVICE, QMCP_EHIP, QMCP_ENOMEM = 0, -1, -2, -3, -4, -5, -6


class QmcpError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"qmcp_hip error {code}: {message}")
        self.code = code


class HostBreakdown(C.Structure):
    """qmcp_hip_host_breakdown (include/qmcp_hip.h)"""
    _fields_ = [("ms_total", C.c_float), ("ms_narrow_h2d", C.c_float), ("ms_solve", C.c_float),
                ("ms_d2h", C.c_float), ("host_threads", C.c_uint32), ("chunks", C.c_uint32),
                ("columns_sent", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [
        ("n_reads", C.c_uint64), ("n_kept", C.c_uint64), ("total_length", C.c_uint64),
        ("n_contigs", C.c_uint32), ("path", C.c_uint32), ("min_span", C.c_uint32),
        ("max_span", C.c_uint32), ("sort_passes", C.c_uint32), ("sweep_stretches", C.c_uint32),
        ("ms_total", C.c_float), ("ms_prepare", C.c_float), ("ms_scan", C.c_float),
        ("ms_sort", C.c_float), ("ms_sweep", C.c_float), ("ms_mark", C.c_float),
        ("ms_h2d", C.c_float), ("ms_d2h", C.c_float), ("columns_sent", C.c_uint32),
        ("spec_boundaries", C.c_uint32), ("spec_mismatches", C.c_uint32),
        ("spec_retry_mismatches", C.c_uint32), ("sweep_blocks_changed", C.c_uint32), ("sweep_blocks", C.c_uint32),
        ("arena_grown_mid_solve", C.c_uint32), ("near_uniform_exceptions", C.c_uint32),
        ("near_uniform_selected", C.c_uint32), ("near_uniform_rounds", C.c_uint32),
        ("near_uniform_giveup", C.c_uint32), ("pm_grid", C.c_int32), ("pm_heaviest_wave_slots", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class QualityStats(C.Structure):
    """qmcp_hip_quality_stats: what the quality pass after the plain solve did"""
    _fields_ = [("quality_min", C.c_uint32), ("quality_max", C.c_uint32), ("key_bits", C.c_uint32),
                ("sort_passes", C.c_uint32), ("cells_contested", C.c_uint64), ("reads_swapped", C.c_uint64),
                ("ms_quality", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TargetStats(C.Structure):
    """qmcp_hip_target_stats: what the projection, compaction and expansion around a target solve did"""
    _fields_ = [("reads_on_target", C.c_uint64), ("reads_off_target", C.c_uint64), ("target_positions", C.c_uint64),
                ("regions_in", C.c_uint32), ("regions_merged", C.c_uint32), ("ms_targets", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class ProfileStats(C.Structure):
    """qmcp_hip_profile_stats: the cap table of a profile solve and what the kernel that builds need(p) counted"""
    _fields_ = [("positions_in_regions", C.c_uint64), ("capped_positions", C.c_uint64), ("demand", C.c_uint64),
                ("regions_in", C.c_uint32), ("regions_used", C.c_uint32), ("ms_profile", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class CeilingStats(C.Structure):
    """qmcp_hip_ceiling_stats: what a ceiling solve dropped, where the data lies above its caps, and what the device-side
    check of the kept depth found (short_*, excess_positions and max_kept_depth: before mates are dropped)"""
    _fields_ = [("reads_placed", C.c_uint64), ("reads_dropped", C.c_uint64), ("mates_dropped", C.c_uint64),
                ("over_positions", C.c_uint64), ("over_bases", C.c_uint64), ("short_positions", C.c_uint64),
                ("short_bases", C.c_uint64), ("excess_positions", C.c_uint64), ("max_kept_depth", C.c_uint32),
                ("regions_in", C.c_uint32), ("regions_used", C.c_uint32), ("ms_ceiling", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class ProportionalStats(C.Structure):
    """qmcp_hip_proportional_stats: the bases a proportional solve saw and kept, what k_prop_need counted along the
    positions (zeros when plain_route == 1: the call was the plain by-contig solve), and the fraction as given"""
    _fields_ = [("reads_placed", C.c_uint64), ("bases_in", C.c_uint64), ("bases_kept", C.c_uint64),
                ("demand", C.c_uint64), ("whole_positions", C.c_uint64), ("floor_positions", C.c_uint64),
                ("capped_positions", C.c_uint64), ("max_depth", C.c_uint32), ("max_need", C.c_uint32),
                ("num", C.c_uint32), ("den", C.c_uint32), ("floor", C.c_uint32), ("plain_route", C.c_uint32),
                ("ms_need", C.c_float), ("ms_tally", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


def as_ratio(x):
    """a proportion as (num, den) with 0 <= num <= den: a (num, den) pair or a fractions.Fraction is taken as is (a
    denominator above PROPORTION_DEN_MAX is the library's to refuse: QMCP_ERANGE), any other number goes through
    Fraction(x).limit_denominator(PROPORTION_DEN_MAX); values outside 0 .. 1 raise ValueError"""
    if isinstance(x, (tuple, list)):
        if len(x) != 2:
            raise ValueError("a proportion given as a pair is (num, den)")
        num, den = operator.index(x[0]), operator.index(x[1])
    elif isinstance(x, fractions.Fraction):
        num, den = x.numerator, x.denominator
    else:
        if not isinstance(x, numbers.Rational):
            x = float(x)
            if not math.isfinite(x):
                raise ValueError(f"a proportion must lie in 0 .. 1, not {x!r}")
        if not 0 <= x <= 1:  # (before the rounding, which would take 1.0000001 to 1)
            raise ValueError(f"a proportion must lie in 0 .. 1, not {x!r}")
        f = fractions.Fraction(x).limit_denominator(PROPORTION_DEN_MAX)
        num, den = f.numerator, f.denominator
    if den < 1:
        raise ValueError("a proportion's denominator must be at least 1")
    if not 0 <= num <= den:
        raise ValueError(f"a proportion must lie in 0 .. 1, not {num} / {den}")
    return int(num), int(den)


class BudgetStats(C.Structure):
    """qmcp_hip_budget_stats: the coverage a budget solve ended on (coverage = M*), what it keeps there (n_kept) and
    what one coverage more would keep (kept_above where a probe measured it, else the lower bound bound_above that
    ruled it out), the data's depth (reads_placed, total_bases, max_depth, top) and the search's cost"""
    _fields_ = [("budget", C.c_uint64), ("reads_placed", C.c_uint64), ("n_kept", C.c_uint64), ("kept_above", C.c_uint64),
                ("bound_above", C.c_uint64), ("total_bases", C.c_uint64), ("coverage", C.c_uint32),
                ("max_depth", C.c_uint32), ("top", C.c_uint32), ("probes", C.c_uint32), ("curve_entries", C.c_uint32),
                ("saturated", C.c_uint32), ("ms_budget", C.c_float), ("ms_solves", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class MeanDepthStats(C.Structure):
    """qmcp_hip_mean_depth_stats: the coverage a mean-depth solve ended on (coverage = M*), the bases it keeps inside the
    regions there (kept_bases, in n_kept reads) and what one coverage more would keep (bases_above where a probe measured
    it, else the bound S_R(M* + 1) = bound_above that ruled it out), the regions (positions, regions_in, regions_used),
    the data's depth inside them (total_bases) and everywhere (max_depth, top) and the search's cost"""
    _fields_ = [("budget", C.c_uint64), ("positions", C.c_uint64), ("reads_placed", C.c_uint64), ("n_kept", C.c_uint64),
                ("kept_bases", C.c_uint64), ("bases_above", C.c_uint64), ("bound_above", C.c_uint64),
                ("total_bases", C.c_uint64), ("coverage", C.c_uint32), ("max_depth", C.c_uint32), ("top", C.c_uint32),
                ("probes", C.c_uint32), ("curve_entries", C.c_uint32), ("saturated", C.c_uint32),
                ("regions_in", C.c_uint32), ("regions_used", C.c_uint32), ("ms_mean_depth", C.c_float),
                ("ms_solves", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class ThresholdsStats(C.Structure):
    """qmcp_hip_thresholds_stats: the range of a thresholds solve (coverage_lo .. coverage_hi), the last coverage it had
    to solve (top, after `solves` whole solves; saturated: every placed read has a threshold), the reads with a
    threshold (n_kept), the (read, M) pairs in which a read with a threshold was not kept (nesting_violations: while it
    is 0, thresholds <= M is solve_by_contig's mask at M bit for bit) and the cost"""
    _fields_ = [("reads_placed", C.c_uint64), ("n_kept", C.c_uint64), ("nesting_violations", C.c_uint64),
                ("coverage_lo", C.c_uint32), ("coverage_hi", C.c_uint32), ("top", C.c_uint32), ("solves", C.c_uint32),
                ("saturated", C.c_uint32), ("count_entries", C.c_uint32), ("ms_thresholds", C.c_float),
                ("ms_solves", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


def region_positions(contig_lengths, region_offsets, region_starts, region_ends):
    """|R| as qmcp_hip_solve_mean_depth_* counts it: per contig the regions (inclusive bounds, any order, overlaps
    allowed) clipped to the contig -- one that begins at or beyond its length is dropped -- and merged; every position
    when region_offsets is None"""
    lengths = np.atleast_1d(np.asarray(contig_lengths, dtype=np.int64))
    if region_offsets is None:
        return int(lengths.sum())
    offs = np.asarray(region_offsets, dtype=np.int64)
    if offs.size != lengths.size + 1:
        raise ValueError("region_offsets needs n_contigs + 1 entries")
    r0, r1 = (np.zeros(0, np.int64) if a is None else np.asarray(a, dtype=np.int64) for a in (region_starts, region_ends))
    if min(r0.size, r1.size) < int(offs[-1]):
        raise ValueError("region_starts / region_ends are shorter than region_offsets says")
    total = 0
    for c, length in enumerate(lengths.tolist()):
        spans = sorted((int(s), min(int(e), length - 1)) for s, e in zip(r0[offs[c]:offs[c + 1]], r1[offs[c]:offs[c + 1]])
                       if s < length)
        reach = -1  # the last position counted so far
        for s, e in spans:
            if e > reach:
                total += e - max(s, reach + 1) + 1
                reach = e
    return total


class PairStats(C.Structure):
    """qmcp_hip_pair_stats: the stages of a pair-aware solve (the first n_stages entries of every array count)"""
    _fields_ = [("n_stages", C.c_uint32), ("reserved", C.c_uint32), ("n_selected", C.c_uint64 * PAIR_MAX_STAGES),
                ("n_kept", C.c_uint64 * PAIR_MAX_STAGES), ("capped_positions", C.c_uint64 * PAIR_MAX_STAGES),
                ("demand", C.c_uint64 * PAIR_MAX_STAGES), ("target", C.c_uint32 * PAIR_MAX_STAGES),
                ("sweeps", C.c_uint32 * PAIR_MAX_STAGES), ("ms_stage", C.c_float * PAIR_MAX_STAGES),
                ("ms_pairs", C.c_float), ("reserved2", C.c_uint32)]

    def as_dict(self):
        k = self.n_stages
        out = {name: list(getattr(self, name))[:k]
               for name in ("target", "n_selected", "n_kept", "capped_positions", "demand", "sweeps", "ms_stage")}
        out.update(n_stages=k, ms_pairs=self.ms_pairs)
        return out


class TemplateStats(C.Structure):
    """qmcp_hip_template_stats: the stages of a template-aware solve (the first n_stages entries of every per-stage array
    count) and the templates: how many have a segment, how many are kept, the largest, the histogram of their sizes
    (1 .. 7 segments, then 8 or more)"""
    _fields_ = [("n_stages", C.c_uint32), ("reserved", C.c_uint32), ("n_selected", C.c_uint64 * PAIR_MAX_STAGES),
                ("n_kept", C.c_uint64 * PAIR_MAX_STAGES), ("capped_positions", C.c_uint64 * PAIR_MAX_STAGES),
                ("demand", C.c_uint64 * PAIR_MAX_STAGES), ("target", C.c_uint32 * PAIR_MAX_STAGES),
                ("sweeps", C.c_uint32 * PAIR_MAX_STAGES), ("ms_stage", C.c_float * PAIR_MAX_STAGES),
                ("ms_templates", C.c_float), ("max_template_size", C.c_uint32), ("n_templates_used", C.c_uint64),
                ("n_templates_kept", C.c_uint64), ("size_hist", C.c_uint64 * 8)]

    def as_dict(self):
        k = self.n_stages
        out = {name: list(getattr(self, name))[:k]
               for name in ("target", "n_selected", "n_kept", "capped_positions", "demand", "sweeps", "ms_stage")}
        out.update(n_stages=k, ms_templates=self.ms_templates, max_template_size=self.max_template_size,
                   n_templates_used=self.n_templates_used, n_templates_kept=self.n_templates_kept,
                   size_hist=list(self.size_hist))
        return out


class TemplateProfileStats(C.Structure):
    """qmcp_hip_template_profile_stats: the cap table of a template-aware solve under caps, the placed segments that
    cover a position with a positive cap, the templates that own one, and the device time of the need kernels"""
    _fields_ = [("positions_in_regions", C.c_uint64), ("n_segments_on_cap", C.c_uint64), ("n_templates_on_cap", C.c_uint64),
                ("regions_in", C.c_uint32), ("regions_used", C.c_uint32), ("ms_need", C.c_float), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class FragmentStats(C.Structure):
    """qmcp_hip_fragment_stats: what the overlap clip of a template's segments did: placed segments and their bases going
    in, segments whose start moved, segments that became unplaced, the bases taken off (per-segment depth minus fragment
    depth, summed), the templates with such a segment, the largest (template, contig) group and the device time"""
    _fields_ = [("n_placed", C.c_uint64), ("n_clipped", C.c_uint64), ("n_emptied", C.c_uint64), ("bases_in", C.c_uint64),
                ("bases_removed", C.c_uint64), ("n_templates_overlapping", C.c_uint64), ("max_group", C.c_uint32),
                ("ms_clip", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class DepthRow(C.Structure):
    """qmcp_hip_depth_row: depth before (in) and after (kept) over the inclusive interval [start, end] of one contig"""
    _fields_ = [("contig", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("min_in", C.c_uint32),
                ("max_in", C.c_uint32), ("min_kept", C.c_uint32), ("max_kept", C.c_uint32), ("reserved", C.c_uint32),
                ("positions", C.c_uint64), ("sum_in", C.c_uint64), ("sum_kept", C.c_uint64),
                ("capped_positions", C.c_uint64), ("deficit_positions", C.c_uint64), ("deficit_sum", C.c_uint64)]


DEPTH_ROW_DTYPE = np.dtype([(name, np.uint32 if t is C.c_uint32 else np.uint64) for name, t in DepthRow._fields_])
assert DEPTH_ROW_DTYPE.itemsize == C.sizeof(DepthRow) == 80


class DepthStats(C.Structure):
    """qmcp_hip_depth_stats"""
    _fields_ = [("reads_placed", C.c_uint64), ("reads_kept", C.c_uint64), ("scope_positions", C.c_uint64),
                ("deficit_positions", C.c_uint64), ("regions_in", C.c_uint32), ("regions_merged", C.c_uint32),
                ("position_batches", C.c_uint32), ("ms_report", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrackRun(C.Structure):
    """qmcp_hip_track_run: a maximal run [start, end] (inclusive) of one contig with one (depth_in, depth_kept, short)"""
    _fields_ = [("contig", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("depth_in", C.c_uint32),
                ("depth_kept", C.c_uint32), ("flags", C.c_uint32)]


TRACK_RUN_DTYPE = np.dtype([(name, np.uint32) for name, _ in TrackRun._fields_])
assert TRACK_RUN_DTYPE.itemsize == C.sizeof(TrackRun) == 24


class TrackStats(C.Structure):
    """qmcp_hip_track_stats"""
    _fields_ = [("n_runs", C.c_uint64), ("positions_in_runs", C.c_uint64), ("scope_positions", C.c_uint64),
                ("short_positions", C.c_uint64), ("reads_placed", C.c_uint64), ("reads_kept", C.c_uint64),
                ("regions_in", C.c_uint32), ("regions_merged", C.c_uint32), ("position_batches", C.c_uint32),
                ("ms_track", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


assert C.sizeof(TrackStats) == 64


class LadderStats(C.Structure):
    """qmcp_hip_ladder_stats: the levels of a coverage ladder (n_kept / ms_level: the first n_levels entries count)"""
    _fields_ = [("n_levels", C.c_uint32), ("reserved", C.c_uint32), ("n_kept", C.c_uint64 * LADDER_MAX_LEVELS),
                ("ms_level", C.c_float * LADDER_MAX_LEVELS), ("ms_ladder", C.c_float)]

    def as_dict(self):
        k = self.n_levels
        return {"n_levels": k, "n_kept": list(self.n_kept[:k]), "ms_level": list(self.ms_level[:k]),
                "ms_ladder": self.ms_ladder}


class ReplicatesStats(C.Structure):
    """qmcp_hip_replicates_stats: the replicates of a split (the arrays' first n_replicates entries count)"""
    _fields_ = [("n_replicates", C.c_uint32), ("flags", C.c_uint32), ("n_full", C.c_uint32), ("reserved", C.c_uint32),
                ("n_offered", C.c_uint64 * REPLICATES_MAX), ("n_kept", C.c_uint64 * REPLICATES_MAX),
                ("n_mates", C.c_uint64 * REPLICATES_MAX), ("short_positions", C.c_uint64 * REPLICATES_MAX),
                ("short_bases", C.c_uint64 * REPLICATES_MAX), ("ms_replicate", C.c_float * REPLICATES_MAX),
                ("ms_split", C.c_float), ("reserved1", C.c_float)]

    def as_dict(self):
        k = self.n_replicates
        out = {"n_replicates": k, "flags": self.flags, "n_full": self.n_full, "ms_split": self.ms_split}
        for name in ("n_offered", "n_kept", "n_mates", "short_positions", "short_bases", "ms_replicate"):
            out[name] = list(getattr(self, name)[:k])
        return out


assert C.sizeof(ReplicatesStats) == 16 + 5 * 8 * REPLICATES_MAX + 4 * REPLICATES_MAX + 8


class StratumRow(C.Structure):
    """qmcp_hip_stratum_row: a stratum's placed reads, how many of them are kept, and the bases of both"""
    _fields_ = [("n_reads", C.c_uint64), ("n_kept", C.c_uint64), ("bases_in", C.c_uint64), ("bases_kept", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TierRow(C.Structure):
    """qmcp_hip_tier_row: a tier's placed reads, how many of them are kept, the bases of both; for a tier after the first
    the sum of need_t, the positions with need_t > 0 and those where its coverage exceeds max(0, M - credit_t); the solver
    calls that queued a sweep and their device time"""
    _fields_ = [("n_reads", C.c_uint64), ("n_kept", C.c_uint64), ("bases_in", C.c_uint64), ("bases_kept", C.c_uint64),
                ("demand", C.c_uint64), ("asked_positions", C.c_uint64), ("capped_positions", C.c_uint64),
                ("sweeps", C.c_uint32), ("ms_stage", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TiersStats(C.Structure):
    """qmcp_hip_tiers_stats: the tiers of the call, those that kept a read, the reads with NO_TIER, and the call's device
    time outside its solver calls"""
    _fields_ = [("n_tiers", C.c_uint32), ("tiers_used", C.c_uint32), ("reads_untiered", C.c_uint64),
                ("ms_tiers", C.c_float), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


assert C.sizeof(TierRow) == 64 and C.sizeof(TiersStats) == 24


class DedupStats(C.Structure):
    """qmcp_hip_dedup_stats: what the duplicate pass before the solve found (units: placed reads, or pairs with a placed
    mate; families: distinct cells / signatures; reads_survived: reads handed to the inner solve)"""
    _fields_ = [("units", C.c_uint64), ("families", C.c_uint64), ("duplicate_units", C.c_uint64),
                ("largest_family", C.c_uint64), ("reads_survived", C.c_uint64), ("key_bits", C.c_uint32),
                ("sort_passes", C.c_uint32), ("ms_dedup", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class StartCapStats(C.Structure):
    """qmcp_hip_start_cap_stats: what the start cap before the solve found (cells: distinct (contig, start, group);
    reads_survived: reads handed to the inner solve; cells_kept / largest_kept_cell: counted from the final mask;
    short_positions / short_bases: only under START_CAP_SHORTFALL)"""
    _fields_ = [("reads_placed", C.c_uint64), ("cells", C.c_uint64), ("cells_over_cap", C.c_uint64),
                ("reads_capped", C.c_uint64), ("largest_cell", C.c_uint64), ("reads_survived", C.c_uint64),
                ("cells_kept", C.c_uint64), ("largest_kept_cell", C.c_uint64), ("short_positions", C.c_uint64),
                ("short_bases", C.c_uint64), ("key_bits", C.c_uint32), ("sort_passes", C.c_uint32), ("cap", C.c_uint32),
                ("ms_cap", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


assert C.sizeof(StartCapStats) == 10 * 8 + 4 * 4


class AmpliconsStats(C.Structure):
    """qmcp_hip_amplicons_stats: what the assign step of an amplicon-aware solve did (units: pairs, or reads when
    single-end; units == units_assigned + units_filtered + units_no_amplicon; the reads_* and bases_clipped count the
    reads of assigned units only)"""
    _fields_ = [("units", C.c_uint64), ("units_assigned", C.c_uint64), ("units_filtered", C.c_uint64),
                ("units_no_amplicon", C.c_uint64), ("units_in_several", C.c_uint64), ("reads_shortened", C.c_uint64),
                ("reads_clipped_away", C.c_uint64), ("bases_clipped", C.c_uint64), ("amplicons", C.c_uint64),
                ("amplicons_unused", C.c_uint64), ("ms_assign", C.c_float), ("ms_report", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


assert C.sizeof(AmpliconsStats) == 10 * 8 + 2 * 4


class DepthReport:
    """what Solver.depth_report returns: contig_rows / region_rows (numpy structured arrays of DEPTH_ROW_DTYPE),
    hist_in / hist_kept (uint64, n_bins entries), stats (DepthStats); valid: no position in scope is short of
    min(coverage, max_coverage)"""

    def __init__(self, contig_rows, region_rows, hist_in, hist_kept, stats):
        self.contig_rows, self.region_rows = contig_rows, region_rows
        self.hist_in, self.hist_kept, self.stats = hist_in, hist_kept, stats

    @property
    def valid(self):
        return self.stats.deficit_positions == 0


class Options(C.Structure):
    """qmcp_hip_options (include/qmcp_hip.h): 0 = the library chooses"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("pass_major", C.c_int32), ("sweep", C.c_int32), ("cut_points", C.c_int32),
        ("speculation", C.c_int32), ("speculation_run_in", C.c_uint32), ("near_uniform", C.c_int32),
        ("near_uniform_rounds", C.c_uint32), ("near_uniform_min_depth", C.c_float), ("near_uniform_debug", C.c_int32),
        ("force_sort_route", C.c_int32), ("keep_expand", C.c_int32), ("mixed_sweep_in_lds", C.c_int32),
        ("rank_min_reads", C.c_uint32), ("host_threads", C.c_uint32), ("copy_streams", C.c_uint32),
        ("host_both_columns", C.c_int32), ("pm_grid", C.c_int32),
    ]


class DownsampleRequest(C.Structure):
    """qmcp_host_downsample_request (genome-downsampler_amd/host/include/qmcp_host_request.h): what
    qmcp_host_downsample_bam takes.  Build one with _downsample_request, which knows the fields whose "not given" is
    not zero"""
    _fields_ = (
        [("struct_size", C.c_uint64)]
        + [(name, C.c_char_p) for name in ("solver_name", "in_path", "out_path", "filtered_path", "bed", "tsv", "targets",
                                           "report", "track", "track_channel")]
        + [("ladder_levels", C.POINTER(C.c_uint32))]
        + [(name, C.c_char_p) for name in ("ladder_template", "stratify", "strata_report", "dedup_report")]
        + [(name, C.POINTER(C.c_uint32)) for name in ("region_offsets", "region_starts", "region_ends", "region_caps")]
        + [("n_refs", C.c_uint64), ("pair_stages", C.POINTER(C.c_uint32)), ("template_stages", C.POINTER(C.c_uint32)),
           ("fragment_report", C.c_char_p), ("ceiling_report", C.c_char_p), ("budget_report", C.c_char_p),
           ("budget_reads", C.c_uint64), ("budget_fraction", C.c_double), ("mean_depth_targets", C.c_char_p),
           ("mean_depth_report", C.c_char_p), ("budget_bases", C.c_uint64), ("mean_depth", C.c_double),
           ("thresholds_tag", C.c_char_p), ("thresholds_report", C.c_char_p),
           ("replicates_further", C.POINTER(C.c_uint32)),
           ("replicates_template", C.c_char_p), ("replicates_report", C.c_char_p)]
        + [(name, C.c_uint32) for name in ("max_coverage", "min_len", "min_mapq", "target_padding", "report_bins",
                                           "track_cap", "n_ladder_levels", "default_cap", "n_pair_stages",
                                           "n_template_stages", "n_replicates_further", "thresholds_lo",
                                           "thresholds_hi")]
        + [(name, C.c_int32) for name in ("amplicon_mode", "per_reference", "amplicons_by_reference", "keep_off_target",
                                          "dedup", "has_regions", "pair_aware", "template_aware", "split_spliced",
                                          "include_secondary", "fragment_depth", "ceiling", "has_budget_reads",
                                          "has_budget_bases", "has_mean_depth", "has_replicates", "has_thresholds",
                                          "start_cap_by_strand")]
        + [("start_cap", C.c_uint32), ("start_cap_report", C.c_char_p)]
        + [("primer_clip", C.c_int32), ("per_amplicon", C.c_int32), ("amplicon_report", C.c_char_p)]
        + [("mapq_tiers", C.POINTER(C.c_uint32)), ("n_mapq_tiers", C.c_uint32), ("tiers_report", C.c_char_p)]
        + [("proportional_report", C.c_char_p), ("proportion_num", C.c_uint32), ("proportion_den", C.c_uint32),
           ("proportion_floor", C.c_uint32), ("has_proportion", C.c_int32)])


SWEEP_AUTO, SWEEP_FAST, SWEEP_GENERAL, SWEEP_EVENTS = 0, 1, 2, 3
_SWEEP_NAMES = {None: 0, "auto": 0, "fast": 1, "gen": 2, "general": 2, "ev": 3, "events": 3}


if not os.path.exists(HIP_LIB_PATH):
    raise ImportError(
        f"{HIP_LIB_PATH} is missing: build it with `make lib` (or __graft_entry__.build()); "
        "this package has no CPU fallback")

_hip = C.CDLL(HIP_LIB_PATH, mode=C.RTLD_GLOBAL)
_host = C.CDLL(HOST_LIB_PATH) if os.path.exists(HOST_LIB_PATH) else None

_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_hip.qmcp_hip_last_error.restype = C.c_char_p
_hip.qmcp_hip_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
_hip.qmcp_hip_destroy.argtypes = [C.c_void_p]
_hip.qmcp_hip_destroy.restype = None
_hip.qmcp_hip_default_options.argtypes = [C.POINTER(Options)]
_hip.qmcp_hip_default_options.restype = None
_hip.qmcp_hip_set_options.argtypes = [C.c_void_p, C.POINTER(Options)]
_hip.qmcp_hip_get_options.argtypes = [C.c_void_p, C.POINTER(Options)]
_hip.qmcp_hip_solve_host.argtypes = [C.c_void_p, _u32p, _u32p, C.c_uint64, _u64p, _u32p,
                                     C.c_uint32, C.c_uint32, _u64p, C.POINTER(Stats)]
_hip.qmcp_hip_solve_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p, _u32p,
                                       C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.POINTER(Stats)]
_hip.qmcp_hip_solve_device_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p, _u32p,
                                             C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
_hip.qmcp_hip_solve_end.argtypes = [C.c_void_p, C.POINTER(Stats)]
_hip.qmcp_hip_solve_host64.argtypes = [C.c_void_p, _u64p, _u64p, C.c_uint64, _u64p, _u32p, C.c_uint32,
                                       C.c_uint32, _u64p, C.POINTER(Stats), C.POINTER(HostBreakdown)]
_hip.qmcp_hip_multi_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
_hip.qmcp_hip_multi_destroy.argtypes = [C.c_void_p]
_hip.qmcp_hip_multi_destroy.restype = None
_hip.qmcp_hip_multi_solve_host.argtypes = [C.c_void_p, _u32p, _u32p, C.c_uint64, _u64p, _u32p, C.c_uint32,
                                           C.c_uint32, _u64p, C.POINTER(Stats), C.POINTER(C.c_int)]
_hip.qmcp_hip_demand_host.argtypes = [C.c_void_p, _u32p, _u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
_hip.qmcp_hip_coverage_host.argtypes = [C.c_void_p, _u32p, _u32p, C.c_uint64, _u64p, _u32p,
                                        C.c_uint32, _u32p]
_hip.qmcp_hip_filtered_coverage_host.argtypes = [C.c_void_p, _u32p, _u32p, C.c_uint64, _u64p, _u32p,
                                                 C.c_uint32, _u64p, _u32p]
_hip.qmcp_hip_complete_pairs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
_hip.qmcp_hip_complete_pairs_host.argtypes = [C.c_void_p, _u64p, C.c_uint64]
_hip.qmcp_hip_amplicon_filter_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, C.c_uint64,
                                               _u32p, _u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                               _u64p]
_hip.qmcp_hip_filter_solve_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, C.c_uint64, _u32p,
                                            _u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_int, _u64p, _u64p, C.POINTER(Stats)]
_hip.qmcp_hip_solve_by_contig_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32,
                                                C.c_uint32, _u64p, C.POINTER(Stats)]
_hip.qmcp_hip_solve_by_contig_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p,
                                                  C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
_hip.qmcp_hip_filter_solve_by_contig_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, _u32p, C.c_uint64, _u32p,
                                                       C.c_uint32, _u32p, _u32p, _u32p, C.c_uint32, C.c_uint32,
                                                       C.c_uint32, C.c_int, _u64p, _u64p, C.POINTER(Stats)]
_hip.qmcp_hip_solve_quality_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u64p, _u32p, C.c_uint32,
                                             C.c_uint32, _u64p, C.POINTER(Stats), C.POINTER(QualityStats)]
_hip.qmcp_hip_solve_quality_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p, _u32p,
                                               C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats),
                                               C.POINTER(QualityStats)]
_hip.qmcp_hip_solve_quality_by_contig_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, C.c_uint64, _u32p,
                                                       C.c_uint32, C.c_uint32, _u64p, C.POINTER(Stats),
                                                       C.POINTER(QualityStats)]
_hip.qmcp_hip_solve_targets_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32,
                                             _u32p, _u32p, _u32p, C.c_uint32, C.c_uint32, C.c_uint32, _u64p,
                                             C.POINTER(Stats), C.POINTER(TargetStats)]
_hip.qmcp_hip_solve_targets_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                               _u32p, C.c_uint32, _u32p, _u32p, _u32p, C.c_uint32, C.c_uint32,
                                               C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats),
                                               C.POINTER(TargetStats)]
_depth_out = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, _u64p, _u64p, _u64p]
_hip.qmcp_hip_depth_report_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32, _u64p,
                                            C.c_uint32, _u32p, _u32p, _u32p, C.c_uint32] + _depth_out + \
                                           [C.POINTER(DepthStats)]
_hip.qmcp_hip_depth_report_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p,
                                              C.c_uint32, C.c_void_p, C.c_uint32, _u32p, _u32p, _u32p, C.c_uint32] + \
                                             _depth_out + [C.c_void_p, C.POINTER(DepthStats)]
_track_out = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, _u64p]
_hip.qmcp_hip_depth_track_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32, _u64p,
                                           C.c_uint32, _u32p, _u32p, _u32p, C.c_uint32] + _track_out + \
                                          [C.POINTER(TrackStats)]
_hip.qmcp_hip_depth_track_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p,
                                             C.c_uint32, C.c_void_p, C.c_uint32, _u32p, _u32p, _u32p, C.c_uint32] + \
                                            _track_out + [C.c_void_p, C.POINTER(TrackStats)]
_hip.qmcp_hip_solve_ladder_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32, _u32p,
                                            C.c_uint32, C.c_void_p, C.POINTER(Stats), C.POINTER(LadderStats)]
_hip.qmcp_hip_solve_replicates_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32, _u32p,
                                                C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(Stats), C.POINTER(Stats),
                                                C.POINTER(ReplicatesStats)]
_hip.qmcp_hip_solve_replicates_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p,
                                                  C.c_uint32, _u32p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                  C.POINTER(Stats), C.POINTER(Stats), C.POINTER(ReplicatesStats)]
_hip.qmcp_hip_solve_ladder_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p,
                                              C.c_uint32, _u32p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats),
                                              C.POINTER(LadderStats)]
_hip.qmcp_hip_solve_stratified_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32,
                                                _u32p, C.c_uint32, _u64p, C.POINTER(StratumRow), C.POINTER(Stats)]
_hip.qmcp_hip_solve_tiers_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32, C.c_uint32,
                                           C.c_uint32, _u64p, C.POINTER(TierRow), C.POINTER(Stats), C.POINTER(TiersStats)]
_hip.qmcp_hip_solve_tiers_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p,
                                             C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(TierRow), C.c_void_p,
                                             C.POINTER(Stats), C.POINTER(TiersStats)]
_hip.qmcp_hip_solve_stratified_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                  _u32p, C.c_uint32, _u32p, C.c_uint32, C.c_void_p,
                                                  C.POINTER(StratumRow), C.c_void_p, C.POINTER(Stats)]
_hip.qmcp_hip_solve_dedup_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32,
                                           C.c_uint32, C.c_uint32, _u64p, _u64p, _u64p, C.c_uint32, C.POINTER(Stats),
                                           C.POINTER(DedupStats)]
_hip.qmcp_hip_solve_dedup_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_uint64, _u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                             C.c_void_p, _u64p, C.c_uint32, C.c_void_p, C.POINTER(Stats),
                                             C.POINTER(DedupStats)]
_hip.qmcp_hip_solve_start_cap_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, _u32p, C.c_uint64, _u32p,
                                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u64p, _u64p, _u64p,
                                               C.c_uint32, C.POINTER(Stats), C.POINTER(StartCapStats)]
_hip.qmcp_hip_solve_start_cap_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_uint64, _u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                 C.c_void_p, C.c_void_p, _u64p, C.c_uint32, C.c_void_p, C.POINTER(Stats),
                                                 C.POINTER(StartCapStats)]
_amplicons_tail = [_u32p, C.c_uint32, _u32p, _u32p, _u32p, _u32p, _u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
_hip.qmcp_hip_solve_amplicons_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, _u32p, C.c_uint64] + \
                                              _amplicons_tail + [_u64p, _u32p, C.c_void_p, C.POINTER(Stats),
                                                                 C.POINTER(AmpliconsStats)]
_hip.qmcp_hip_solve_amplicons_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_uint64] + _amplicons_tail + \
                                                [C.c_void_p, _u32p, C.c_void_p, C.c_void_p, C.POINTER(Stats),
                                                 C.POINTER(AmpliconsStats)]
_hip.qmcp_hip_solve_profile_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32, _u32p, _u32p,
                                             _u32p, _u32p, C.c_uint32, C.c_uint32, _u64p, C.POINTER(Stats),
                                             C.POINTER(ProfileStats)]
_hip.qmcp_hip_solve_profile_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p,
                                               C.c_uint32, _u32p, _u32p, _u32p, _u32p, C.c_uint32, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.POINTER(Stats), C.POINTER(ProfileStats)]
_hip.qmcp_hip_solve_pairs_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32, C.c_uint32,
                                           _u32p, C.c_uint32, _u64p, C.POINTER(Stats), C.POINTER(PairStats)]
_hip.qmcp_hip_solve_pairs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p, C.c_uint32,
                                             C.c_uint32, _u32p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats),
                                             C.POINTER(PairStats)]
_hip.qmcp_hip_solve_templates_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, C.c_uint64, C.c_uint32, _u32p,
                                               C.c_uint32, C.c_uint32, _u32p, C.c_uint32, _u64p, C.POINTER(Stats),
                                               C.POINTER(TemplateStats)]
_hip.qmcp_hip_solve_templates_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                 C.c_uint32, _u32p, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, C.c_void_p,
                                                 C.c_void_p, C.POINTER(Stats), C.POINTER(TemplateStats)]
_hip.qmcp_hip_clip_templates_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, C.c_uint64, C.c_uint32, _u32p,
                                              C.c_uint32, _u32p, _u32p, C.POINTER(FragmentStats)]
_hip.qmcp_hip_clip_templates_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                C.c_uint32, _u32p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(FragmentStats)]
_hip.qmcp_hip_solve_fragments_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, _u32p, C.c_uint64, C.c_uint32, _u32p,
                                               C.c_uint32, C.c_uint32, _u32p, C.c_uint32, _u64p, C.POINTER(Stats),
                                               C.POINTER(TemplateStats), C.POINTER(FragmentStats)]
_hip.qmcp_hip_solve_fragments_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                 C.c_uint32, _u32p, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, C.c_void_p,
                                                 C.c_void_p, C.POINTER(Stats), C.POINTER(TemplateStats),
                                                 C.POINTER(FragmentStats)]
_hip.qmcp_hip_solve_templates_profile_host.argtypes = [
    C.c_void_p, _u32p, _u32p, _u32p, _u32p, C.c_uint64, C.c_uint32, _u32p, C.c_uint32, _u32p, _u32p, _u32p, _u32p,
    C.c_uint32, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, _u64p, C.POINTER(Stats), C.POINTER(TemplateStats),
    C.POINTER(TemplateProfileStats)]
_hip.qmcp_hip_solve_templates_profile_device.argtypes = [
    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, _u32p, C.c_uint32, _u32p, _u32p,
    _u32p, _u32p, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats),
    C.POINTER(TemplateStats), C.POINTER(TemplateProfileStats)]
_hip.qmcp_hip_solve_ceiling_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32, _u32p, _u32p,
                                             _u32p, _u32p, C.c_uint32, C.c_uint32, _u64p, C.POINTER(Stats),
                                             C.POINTER(CeilingStats)]
_hip.qmcp_hip_solve_ceiling_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p,
                                               C.c_uint32, _u32p, _u32p, _u32p, _u32p, C.c_uint32, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.POINTER(Stats), C.POINTER(CeilingStats)]
_hip.qmcp_hip_solve_budget_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32, C.c_uint32,
                                            C.c_uint64, C.c_uint32, _u64p, C.c_uint32, _u64p, C.POINTER(Stats),
                                            C.POINTER(BudgetStats)]
_hip.qmcp_hip_solve_mean_depth_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32, C.c_uint32,
                                                C.c_uint64, _u32p, _u32p, _u32p, C.c_uint32, _u64p, C.c_uint32, _u64p,
                                                C.POINTER(Stats), C.POINTER(MeanDepthStats)]
_hip.qmcp_hip_solve_mean_depth_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p,
                                                  C.c_uint32, C.c_uint32, C.c_uint64, _u32p, _u32p, _u32p, C.c_uint32,
                                                  _u64p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats),
                                                  C.POINTER(MeanDepthStats)]
_u16p = C.POINTER(C.c_uint16)
_hip.qmcp_hip_solve_thresholds_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.c_uint32, _u16p, _u64p, C.c_uint32, C.POINTER(Stats),
                                                C.POINTER(ThresholdsStats)]
_hip.qmcp_hip_solve_thresholds_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p,
                                                  C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _u64p,
                                                  C.c_uint32, C.c_void_p, C.POINTER(Stats), C.POINTER(ThresholdsStats)]
_hip.qmcp_hip_solve_budget_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p,
                                              C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _u64p, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.POINTER(Stats), C.POINTER(BudgetStats)]
_hip.qmcp_hip_solve_proportional_host.argtypes = [C.c_void_p, _u32p, _u32p, _u32p, C.c_uint64, _u32p, C.c_uint32,
                                                  C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u64p,
                                                  C.POINTER(Stats), C.POINTER(ProportionalStats)]
_hip.qmcp_hip_solve_proportional_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u32p,
                                                    C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.POINTER(Stats),
                                                    C.POINTER(ProportionalStats)]
_hip.qmcp_hip_set_profiling.argtypes = [C.c_void_p, C.c_int]
_hip.qmcp_hip_kernel_times.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
if _host is not None:
    _host.qmcp_host_reads_gen.argtypes = [C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32,
                                          _u32p, _u32p, _u32p]
    _host.qmcp_host_reads_gen_aos.argtypes = _host.qmcp_host_reads_gen.argtypes
    _host.qmcp_host_solver_names.argtypes = [C.c_char_p, C.c_size_t]
    _host.qmcp_host_solve.argtypes = [C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                                      C.c_int, _u64p]
    _host.qmcp_host_solve.restype = C.c_int64
    _host.qmcp_host_solve_with_qualities.argtypes = [C.c_char_p, _u32p, _u32p, _u32p, C.c_uint64, C.c_uint32,
                                                     C.c_uint32, C.c_int, C.c_int, _u64p]
    _host.qmcp_host_solve_with_qualities.restype = C.c_int64
    _host.qmcp_host_solver_uses_quality.argtypes = [C.c_char_p]
    _host.qmcp_host_plugin_solve_timed.argtypes = [C.c_char_p, _u32p, _u32p, C.c_uint64, C.c_uint32,
                                                   C.c_uint32, _u64p, C.POINTER(C.c_float)]
    _host.qmcp_host_plugin_solve_timed.restype = C.c_int64
    _u16p, _u8p = C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)
    _host.qmcp_host_write_synthetic_bam.argtypes = [C.c_char_p, C.c_uint32, C.c_uint64, _u32p, _u16p, _u32p,
                                                    _u8p, _u32p, _u32p, _u32p, _u32p]
    _host.qmcp_host_read_bam.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32,
                                         C.c_uint64, _u64p, _u32p, _u32p, _u32p, _u32p, _u8p, C.c_uint64, _u64p,
                                         _u64p, _u32p]
    _host.qmcp_host_read_bam.restype = C.c_int64
    _host.qmcp_host_downsample_bam.argtypes = [C.POINTER(DownsampleRequest), C.POINTER(C.c_int64), C.c_uint64,
                                               C.POINTER(CeilingStats), C.POINTER(BudgetStats),
                                               C.POINTER(ReplicatesStats), C.POINTER(TemplateStats),
                                               C.POINTER(TemplateProfileStats), C.c_char_p, C.c_size_t]
    _host.qmcp_host_downsample_bam.restype = C.c_int64
    _host.qmcp_host_read_bam_per_reference.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32,
                                                       C.c_uint64, _u64p, _u32p, _u32p, _u32p, _u32p,
                                                       C.POINTER(C.c_uint8), _u32p, C.c_uint64, _u64p,
                                                       C.POINTER(C.c_uint64), C.c_uint64, _u32p,
                                                       C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
    _host.qmcp_host_read_bam_per_reference.restype = C.c_int64
    _host.qmcp_host_read_bam_by_reference.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int,
                                                      C.c_uint32, C.c_uint32, C.c_uint64, _u64p, _u32p, _u32p, _u32p,
                                                      _u32p, C.POINTER(C.c_uint8), _u32p, C.c_uint64, _u64p,
                                                      C.POINTER(C.c_uint64), C.c_uint64, _u32p, C.POINTER(C.c_uint64),
                                                      C.c_char_p, C.c_size_t]
    _host.qmcp_host_read_bam_by_reference.restype = C.c_int64
    _host.qmcp_host_read_bam_stratified.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64, _u64p,
                                                    _u32p, _u32p, _u32p, _u32p, C.POINTER(C.c_uint8), _u32p, _u32p,
                                                    C.c_uint64, _u64p, C.POINTER(C.c_uint64), C.c_uint64, _u32p,
                                                    C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t,
                                                    C.POINTER(C.c_uint64), C.c_int, C.c_char_p, C.c_size_t]
    _host.qmcp_host_read_bam_stratified.restype = C.c_int64
    _host.qmcp_host_read_bam_templates.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint64, _u32p,
                                                   _u32p, _u32p, _u32p, _u32p, _u32p, _u64p, C.c_uint64, _u64p,
                                                   C.POINTER(C.c_uint64), C.c_uint64, _u32p, C.POINTER(C.c_uint64),
                                                   C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
    _host.qmcp_host_read_bam_templates.restype = C.c_int64
    _host.qmcp_host_check_targets_config.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, _u64p, C.c_char_p,
                                                     C.c_size_t]
    _host.qmcp_host_check_targets_config.restype = C.c_int64
    _host.qmcp_host_amplicons_by_reference.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_uint64,
                                                       _u32p, _u32p, _u32p, C.c_uint64, C.c_char_p, C.c_size_t]
    _host.qmcp_host_amplicons_by_reference.restype = C.c_int64
    _host.qmcp_host_reference_names.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, _u32p, C.c_uint64]
    _host.qmcp_host_reference_names.restype = C.c_int64
    _host.qmcp_host_check_bam.argtypes = [C.c_char_p, _u64p, C.c_char_p, C.c_size_t]
    _host.qmcp_host_bamapi_probe.argtypes = [_u32p, _u32p, C.c_uint64, C.c_uint32, C.c_int, _u64p,
                                             C.c_uint64, _u32p, _u32p, _u64p]
    _host.qmcp_host_bamapi_probe.restype = C.c_int64
    _host.qmcp_host_amplicons_from_files.argtypes = [C.c_char_p, C.c_char_p, _u32p, _u32p, C.c_size_t]


def _p32(a):
    return a.ctypes.data_as(_u32p) if a is not None else None


def _p64(a):
    return a.ctypes.data_as(_u64p) if a is not None else None


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _check(rc):
    if rc != QMCP_OK:
        raise QmcpError(rc, _hip.qmcp_hip_last_error().decode())


def abi_version():
    return _hip.qmcp_hip_abi_version()


def device_count():
    return _hip.qmcp_hip_device_count()


def exported_symbols():
    return [s for s in ABI_SYMBOLS if hasattr(_hip, s)]


def mask_words(n_reads):
    return (int(n_reads) + 63) // 64


def mask_to_indices(mask, n_reads):
    """ascending kept ReadIndex list == the reference's Solution vector"""
    bits = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[:n_reads]
    return np.flatnonzero(bits).astype(np.uint64)


def indices_to_mask(indices, n_reads):
    bits = np.zeros(mask_words(n_reads) * 64, dtype=np.uint8)
    bits[np.asarray(indices, dtype=np.int64)] = 1
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def ladder_mask(levels, j):
    """the packed keep mask (np.uint64 words, input order) of level j of a coverage ladder: K_j = {i : levels[i] > j}"""
    levels = np.ascontiguousarray(levels, dtype=np.uint8)
    bits = np.zeros(mask_words(levels.size) * 64, dtype=np.uint8)
    bits[:levels.size] = levels > int(j)
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def threshold_mask(thresholds, M):
    """the packed keep mask (np.uint64 words, input order) of coverage M from the thresholds of Solver.solve_thresholds:
    {i : thresholds[i] <= M}, for M inside the solved range"""
    thresholds = np.ascontiguousarray(thresholds, dtype=np.uint16)
    bits = np.zeros(mask_words(thresholds.size) * 64, dtype=np.uint8)
    bits[:thresholds.size] = thresholds <= min(int(M), THRESHOLD_NEVER - 1)
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def replicate_mask(labels, r):
    """the packed mask (np.uint64 words, input order) of replicate r (1-based) of a replicate split: R_r = {i : labels[i]
    == r}"""
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    bits = np.zeros(mask_words(labels.size) * 64, dtype=np.uint8)
    bits[:labels.size] = labels == int(r)
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def _contig_tables(n_reads, contig_read_offsets, contig_lengths):
    if contig_read_offsets is None:
        lengths = np.atleast_1d(np.asarray(contig_lengths, dtype=np.uint32))
        assert lengths.size == 1, "contig_read_offsets required for several contigs"
        offs = np.array([0, n_reads], dtype=np.uint64)
    else:
        offs = np.ascontiguousarray(contig_read_offsets, dtype=np.uint64)
        lengths = np.ascontiguousarray(contig_lengths, dtype=np.uint32)
    return offs, lengths


class Solver:
    """One solver context == one reference solver instance (created once, solved many times)."""

    def __init__(self, device=0):
        self._ctx = C.c_void_p()
        _check(_hip.qmcp_hip_create(int(device), C.byref(self._ctx)))
        self.device = device
        self.last_stats = None
        self.last_quality_stats = None
        self.last_target_stats = None
        self.last_ladder_stats = None
        self.last_stratum_rows = None
        self.last_tier_rows = None
        self.last_tiers_stats = None
        self.last_dedup_stats = None
        self.last_start_cap_stats = None
        self.last_amplicons_stats = None
        self.last_pair_stats = None
        self.last_template_stats = None
        self.last_template_profile_stats = None
        self.last_fragment_stats = None
        self.last_ceiling_stats = None
        self.last_proportional_stats = None
        self.last_budget_stats = None
        self.last_mean_depth_stats = None
        self.last_thresholds_stats = None
        self.last_replicates_stats = None
        self.last_replicate_solve_stats = None

    def close(self):
        if self._ctx:
            _hip.qmcp_hip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_profiling(self, enabled):
        """bracket kernel launches with HIP events on the solver stream (resets the totals):
        True / 1 every kernel, 2 only the selection sweep, False / 0 off"""
        _check(_hip.qmcp_hip_set_profiling(self._ctx, 2 if enabled == 2 else int(bool(enabled))))

    def kernel_times(self):
        """{kernel: (launches, total_ms)} accumulated since set_profiling(True)"""
        buf = C.create_string_buffer(8192)
        n = _hip.qmcp_hip_kernel_times(self._ctx, buf, len(buf))
        if n < 0:
            _check(n)
        out = {}
        for line in buf.value.decode().splitlines():
            name, launches, ms = line.split("\t")
            out[name] = (int(launches), float(ms))
        return out

    def solve(self, starts, ends, contig_lengths, max_coverage, contig_read_offsets=None):
        """host arrays in, host keep bitmask (np.uint64 words) out"""
        starts, ends = _u32(starts), _u32(ends)
        n = starts.size
        offs, lengths = _contig_tables(n, contig_read_offsets, contig_lengths)
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st = Stats()
        _check(_hip.qmcp_hip_solve_host(self._ctx, _p32(starts), _p32(ends), n, _p64(offs),
                                        _p32(lengths), lengths.size, int(max_coverage), _p64(mask),
                                        C.byref(st)))
        self.last_stats = st
        return mask[:mask_words(n)]

    def solve_quality(self, starts, ends, qualities, contig_lengths, max_coverage, contig_read_offsets=None):
        """solve()'s coverage and number of reads, with the best reads: in every (contig, start, end) cell the plain
        solve's count of reads, taken by quality descending, then read index; host keep bitmask out.  The plain solve's
        stats go to last_stats, the quality pass's to last_quality_stats"""
        starts, ends = _u32(starts), _u32(ends)
        q = None if qualities is None else _u32(qualities)
        n = starts.size
        assert q is None or q.size == n, "one quality per read"
        offs, lengths = _contig_tables(n, contig_read_offsets, contig_lengths)
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st, qs = Stats(), QualityStats()
        _check(_hip.qmcp_hip_solve_quality_host(self._ctx, _p32(starts), _p32(ends), _p32(q), n, _p64(offs),
                                                _p32(lengths), lengths.size, int(max_coverage), _p64(mask),
                                                C.byref(st), C.byref(qs)))
        self.last_stats, self.last_quality_stats = st, qs
        return mask[:mask_words(n)]

    def solve_quality_device(self, d_starts, d_ends, d_qualities, n_reads, contig_lengths, max_coverage, d_mask,
                             contig_read_offsets=None, stream=0):
        """solve_quality on device pointers (ints); the mask is written to d_mask.  Returns the quality stats"""
        offs, lengths = _contig_tables(n_reads, contig_read_offsets, contig_lengths)
        st, qs = Stats(), QualityStats()
        _check(_hip.qmcp_hip_solve_quality_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                  C.c_void_p(d_qualities), int(n_reads), _p64(offs), _p32(lengths),
                                                  lengths.size, int(max_coverage), C.c_void_p(d_mask),
                                                  C.c_void_p(stream), C.byref(st), C.byref(qs)))
        self.last_stats, self.last_quality_stats = st, qs
        return qs

    def solve_quality_by_contig(self, starts, ends, contig_ids, qualities, contig_lengths, max_coverage):
        """solve_by_contig, then the quality pass on its input-order mask (the contig is part of every cell)"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        q = None if qualities is None else _u32(qualities)
        n = starts.size
        assert ends.size == n and ids.size == n and (q is None or q.size == n), "one entry per read in every column"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st, qs = Stats(), QualityStats()
        _check(_hip.qmcp_hip_solve_quality_by_contig_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), _p32(q), n,
                                                          _p32(lengths), lengths.size, int(max_coverage), _p64(mask),
                                                          C.byref(st), C.byref(qs)))
        self.last_stats, self.last_quality_stats = st, qs
        return mask[:mask_words(n)]

    def solve_by_contig(self, starts, ends, contig_ids, contig_lengths, max_coverage):
        """reads of several contigs in any order, one contig id each (NO_CONTIG: unplaced, never kept) -- grouped on
        the device, solved per contig in batches within one call's limits; host keep bitmask in INPUT order out"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st = Stats()
        _check(_hip.qmcp_hip_solve_by_contig_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), n, _p32(lengths),
                                                  lengths.size, int(max_coverage), _p64(mask), C.byref(st)))
        self.last_stats = st
        return mask[:mask_words(n)]

    def solve_by_contig_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, max_coverage, d_mask,
                               stream=0):
        """the same on device pointers (ints); the input-order mask is written to d_mask"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        st = Stats()
        _check(_hip.qmcp_hip_solve_by_contig_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                    C.c_void_p(d_contig_ids), int(n_reads), _p32(lengths),
                                                    lengths.size, int(max_coverage), C.c_void_p(d_mask),
                                                    C.c_void_p(stream), C.byref(st)))
        self.last_stats = st
        return st

    def solve_ladder(self, starts, ends, contig_ids, contig_lengths, coverages):
        """solve_by_contig at several falling coverages in one call (qmcp_hip_solve_ladder_host): level 0 is
        solve_by_contig at coverages[0], every further level is solved on the reads the level above kept, so the levels
        are nested.  -> one uint8 per read in INPUT order, the number of levels that keep it (ladder_mask(levels, j) is
        level j's mask).  Level 0's stats go to last_stats, the levels' to last_ladder_stats"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        cov = np.atleast_1d(np.ascontiguousarray(coverages, dtype=np.uint32))
        levels = np.zeros(max(n, 1), dtype=np.uint8)
        st, ls = Stats(), LadderStats()
        _check(_hip.qmcp_hip_solve_ladder_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), n, _p32(lengths),
                                               lengths.size, _p32(cov), cov.size, C.c_void_p(levels.ctypes.data),
                                               C.byref(st), C.byref(ls)))
        self.last_stats, self.last_ladder_stats = st, ls
        return levels[:n]

    def solve_ladder_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, coverages, d_levels,
                            stream=0):
        """the same on device pointers (ints); the level bytes (n_reads of them, input order) are written to d_levels.
        Returns the ladder stats"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        cov = np.atleast_1d(np.ascontiguousarray(coverages, dtype=np.uint32))
        st, ls = Stats(), LadderStats()
        _check(_hip.qmcp_hip_solve_ladder_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                 C.c_void_p(d_contig_ids), int(n_reads), _p32(lengths), lengths.size,
                                                 _p32(cov), cov.size, C.c_void_p(d_levels), C.c_void_p(stream),
                                                 C.byref(st), C.byref(ls)))
        self.last_stats, self.last_ladder_stats = st, ls
        return ls

    def solve_replicates(self, starts, ends, contig_ids, contig_lengths, coverages, flags=0):
        """one read set split into disjoint downsamples in one call (qmcp_hip_solve_replicates_host): replicate 1 is
        solve_by_contig at coverages[0], replicate r + 1 is solve_by_contig at coverages[r] of the placed reads that no
        earlier replicate took.  flags: REPLICATES_WHOLE_PAIRS (reads (2q, 2q + 1) move together),
        REPLICATES_SHORTFALL (per replicate, how far it stays below min(cov, coverage)).  -> one uint8 per read in INPUT
        order, the replicate that holds it (1-based; 0: none; replicate_mask(labels, r) is replicate r's mask).
        Replicate 1's solve stats go to last_stats, the replicates' to last_replicates_stats, and the batch-summed
        stats of each replicate's solves to last_replicate_solve_stats (a list)"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        cov = np.atleast_1d(np.ascontiguousarray(coverages, dtype=np.uint32))
        labels = np.zeros(max(n, 1), dtype=np.uint8)
        st, rs = Stats(), ReplicatesStats()
        reps = (Stats * max(cov.size, 1))()
        _check(_hip.qmcp_hip_solve_replicates_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), n, _p32(lengths),
                                                   lengths.size, _p32(cov), cov.size, int(flags),
                                                   C.c_void_p(labels.ctypes.data), C.byref(st), reps, C.byref(rs)))
        self.last_stats, self.last_replicates_stats = st, rs
        self.last_replicate_solve_stats = list(reps)[:cov.size]
        return labels[:n]

    def solve_replicates_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, coverages, d_labels,
                                flags=0, stream=0):
        """the same on device pointers (ints); the label bytes (n_reads of them, input order) are written to d_labels.
        Returns the replicates' stats"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        cov = np.atleast_1d(np.ascontiguousarray(coverages, dtype=np.uint32))
        st, rs = Stats(), ReplicatesStats()
        reps = (Stats * max(cov.size, 1))()
        _check(_hip.qmcp_hip_solve_replicates_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                     C.c_void_p(d_contig_ids), int(n_reads), _p32(lengths), lengths.size,
                                                     _p32(cov), cov.size, int(flags), C.c_void_p(d_labels),
                                                     C.c_void_p(stream), C.byref(st), reps, C.byref(rs)))
        self.last_stats, self.last_replicates_stats = st, rs
        self.last_replicate_solve_stats = list(reps)[:cov.size]
        return rs

    def solve_stratified(self, starts, ends, contig_ids, strata, contig_lengths, max_coverages):
        """one coverage cap per stratum (qmcp_hip_solve_stratified_host): strata[i] < len(max_coverages) names read i's
        stratum (strand, read group, sample, ...), NO_STRATUM a read that belongs to none (never kept).  The mask is the
        OR over the strata of solve_by_contig on that stratum's reads alone at max_coverages[s]; a cap of 0 keeps
        nothing.  Every stratum keeps its own floor min(its coverage, its cap); a stratum with little data is NOT topped
        up from another.  -> host keep bitmask in INPUT order; last_stats, and last_stratum_rows (a list of StratumRow,
        one per stratum)"""
        starts, ends, ids, strata = _u32(starts), _u32(ends), _u32(contig_ids), _u32(strata)
        n = starts.size
        assert ends.size == n and ids.size == n and strata.size == n, \
            "starts, ends, contig_ids and strata must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        caps = np.atleast_1d(np.ascontiguousarray(max_coverages, dtype=np.uint32))
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        rows = (StratumRow * max(caps.size, 1))()
        st = Stats()
        _check(_hip.qmcp_hip_solve_stratified_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), _p32(strata), n,
                                                   _p32(lengths), lengths.size, _p32(caps), caps.size, _p64(mask), rows,
                                                   C.byref(st)))
        self.last_stats, self.last_stratum_rows = st, list(rows)[:caps.size]
        return mask[:mask_words(n)]

    def solve_stratified_device(self, d_starts, d_ends, d_contig_ids, d_strata, n_reads, contig_lengths, max_coverages,
                                d_mask, stream=0):
        """the same on device pointers (ints); the input-order mask is written to d_mask, the rows come back to the host
        (last_stratum_rows).  Returns the stats"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        caps = np.atleast_1d(np.ascontiguousarray(max_coverages, dtype=np.uint32))
        rows = (StratumRow * max(caps.size, 1))()
        st = Stats()
        _check(_hip.qmcp_hip_solve_stratified_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                     C.c_void_p(d_contig_ids), C.c_void_p(d_strata), int(n_reads),
                                                     _p32(lengths), lengths.size, _p32(caps), caps.size,
                                                     C.c_void_p(d_mask), rows, C.c_void_p(stream), C.byref(st)))
        self.last_stats, self.last_stratum_rows = st, list(rows)[:caps.size]
        return st

    def solve_tiers(self, starts, ends, contig_ids, tiers, contig_lengths, max_coverage, n_tiers):
        """the best tier first, worse tiers only where the better ones leave the depth short of min(coverage,
        max_coverage) (qmcp_hip_solve_tiers_host): tiers[i] < n_tiers names read i's tier, 0 the best, NO_TIER a read
        that is never kept.  Tier 0 is solve_by_contig of its reads alone; tier t is the canonical selection of its reads
        alone under need_t = min(its coverage, max(0, max_coverage - the depth of the earlier tiers' kept reads)).  The
        kept depth is >= min(coverage of all tiered reads, max_coverage) everywhere.  -> host keep bitmask in INPUT
        order; last_stats (tier 0's solves), last_tier_rows (a list of TierRow, one per tier), last_tiers_stats"""
        starts, ends, ids, tiers = _u32(starts), _u32(ends), _u32(contig_ids), _u32(tiers)
        n = starts.size
        assert ends.size == n and ids.size == n and tiers.size == n, \
            "starts, ends, contig_ids and tiers must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        rows = (TierRow * max(int(n_tiers), 1))()
        st, ts = Stats(), TiersStats()
        column = tiers if n else np.zeros(1, np.uint32)   # (tiers == NULL is refused, also without reads)
        _check(_hip.qmcp_hip_solve_tiers_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), _p32(column), n, _p32(lengths),
                                              lengths.size, int(max_coverage), int(n_tiers), _p64(mask), rows, C.byref(st),
                                              C.byref(ts)))
        self.last_stats, self.last_tier_rows, self.last_tiers_stats = st, list(rows)[:int(n_tiers)], ts
        return mask[:mask_words(n)]

    def solve_tiers_device(self, d_starts, d_ends, d_contig_ids, d_tiers, n_reads, contig_lengths, max_coverage, n_tiers,
                           d_mask, stream=0):
        """the same on device pointers (ints); the input-order mask is written to d_mask, the rows come back to the host
        (last_tier_rows, last_tiers_stats).  Returns the stats"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        rows = (TierRow * max(int(n_tiers), 1))()
        st, ts = Stats(), TiersStats()
        _check(_hip.qmcp_hip_solve_tiers_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends), C.c_void_p(d_contig_ids),
                                                C.c_void_p(d_tiers), int(n_reads), _p32(lengths), lengths.size,
                                                int(max_coverage), int(n_tiers), C.c_void_p(d_mask), rows,
                                                C.c_void_p(stream), C.byref(st), C.byref(ts)))
        self.last_stats, self.last_tier_rows, self.last_tiers_stats = st, list(rows)[:int(n_tiers)], ts
        return st

    def solve_dedup(self, starts, ends, contig_ids, contig_lengths, max_coverage, tags=None, qualities=None, pairs=False,
                    complete_pairs=False, hist_bins=0):
        """duplicate families collapsed to their representative before solve_by_contig (qmcp_hip_solve_dedup_host).
        A cell is (contig, start, end, tag).  Read mode: a family is the placed reads of one cell, its representative the
        read of highest quality, then lowest index.  pairs=True: unit q is the reads (2q, 2q + 1), a family the units
        with equal unordered pair of cells, the representative the unit of highest summed quality of its placed mates,
        then lowest q.  The mask is solve_by_contig's on the representatives' reads, in INPUT order; complete_pairs ORs
        inside each aligned bit pair afterwards.  tags / qualities: one uint32 per read or None (all 0).
        -> (mask, dup_mask, stats_dict, hist): dup_mask marks the reads of non-representative units, hist[k - 1] counts
        the families of size k (the last of the hist_bins bins: sizes >= hist_bins).  last_stats is the inner solve's,
        last_dedup_stats the DedupStats"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        t = None if tags is None else _u32(tags)
        q = None if qualities is None else _u32(qualities)
        n = starts.size
        assert ends.size == n and ids.size == n and (t is None or t.size == n) and (q is None or q.size == n), \
            "one entry per read in every column"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        flags = (DEDUP_PAIRS if pairs else 0) | (DEDUP_COMPLETE_PAIRS if complete_pairs else 0)
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        dup = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        hist = np.zeros(max(int(hist_bins), 1), dtype=np.uint64)
        st, ds = Stats(), DedupStats()
        _check(_hip.qmcp_hip_solve_dedup_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), _p32(t), _p32(q), n,
                                              _p32(lengths), lengths.size, int(max_coverage), flags, _p64(mask),
                                              _p64(dup), _p64(hist) if hist_bins else None, int(hist_bins),
                                              C.byref(st), C.byref(ds)))
        self.last_stats, self.last_dedup_stats = st, ds
        return mask[:mask_words(n)], dup[:mask_words(n)], ds.as_dict(), hist[:int(hist_bins)]

    def solve_dedup_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, max_coverage, d_mask,
                           d_tags=0, d_qualities=0, pairs=False, complete_pairs=False, d_dup_mask=0, hist_bins=0,
                           stream=0):
        """the same on device pointers (ints; 0: no tags / no qualities / no duplicate mask), columns at any 4-byte
        alignment; the masks are written to d_mask / d_dup_mask.  -> (stats_dict, hist)"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        flags = (DEDUP_PAIRS if pairs else 0) | (DEDUP_COMPLETE_PAIRS if complete_pairs else 0)
        hist = np.zeros(max(int(hist_bins), 1), dtype=np.uint64)
        st, ds = Stats(), DedupStats()
        _check(_hip.qmcp_hip_solve_dedup_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                C.c_void_p(d_contig_ids), C.c_void_p(d_tags or None),
                                                C.c_void_p(d_qualities or None), int(n_reads), _p32(lengths),
                                                lengths.size, int(max_coverage), flags, C.c_void_p(d_mask),
                                                C.c_void_p(d_dup_mask or None), _p64(hist) if hist_bins else None,
                                                int(hist_bins), C.c_void_p(stream), C.byref(st), C.byref(ds)))
        self.last_stats, self.last_dedup_stats = st, ds
        return ds.as_dict(), hist[:int(hist_bins)]

    def solve_start_cap(self, starts, ends, contig_ids, contig_lengths, max_coverage, cap, groups=None, priorities=None,
                        shortfall=False, hist_bins=0):
        """at most `cap` reads of every (contig, start, group) cell reach solve_by_contig
        (qmcp_hip_solve_start_cap_host): the survivors of a cell are its first `cap` reads by priority descending, span
        descending, index ascending; the other placed reads are capped.  The mask is solve_by_contig's on the survivors,
        in INPUT order.  groups / priorities: one uint32 per read or None (one group / all equal).  shortfall=True also
        counts the positions (and bases) where the kept depth is below min(coverage of ALL placed reads, max_coverage).
        -> (mask, capped, stats_dict, hist): capped marks the capped reads, hist[k - 1] counts the cells of size k (the
        last of the hist_bins bins: sizes >= hist_bins).  last_stats is the inner solve's, last_start_cap_stats the
        StartCapStats"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        g = None if groups is None else _u32(groups)
        q = None if priorities is None else _u32(priorities)
        n = starts.size
        assert ends.size == n and ids.size == n and (g is None or g.size == n) and (q is None or q.size == n), \
            "one entry per read in every column"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        capped = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        hist = np.zeros(max(int(hist_bins), 1), dtype=np.uint64)
        st, cs = Stats(), StartCapStats()
        _check(_hip.qmcp_hip_solve_start_cap_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), _p32(g), _p32(q), n,
                                                  _p32(lengths), lengths.size, int(max_coverage), int(cap),
                                                  START_CAP_SHORTFALL if shortfall else 0, _p64(mask), _p64(capped),
                                                  _p64(hist) if hist_bins else None, int(hist_bins), C.byref(st),
                                                  C.byref(cs)))
        self.last_stats, self.last_start_cap_stats = st, cs
        return mask[:mask_words(n)], capped[:mask_words(n)], cs.as_dict(), hist[:int(hist_bins)]

    def solve_start_cap_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, max_coverage, cap, d_mask,
                               d_groups=0, d_priorities=0, shortfall=False, d_capped_mask=0, hist_bins=0, stream=0):
        """the same on device pointers (ints; 0: no groups / no priorities / no capped mask), columns at any 4-byte
        alignment; the masks are written to d_mask / d_capped_mask.  -> (stats_dict, hist)"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        hist = np.zeros(max(int(hist_bins), 1), dtype=np.uint64)
        st, cs = Stats(), StartCapStats()
        _check(_hip.qmcp_hip_solve_start_cap_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                    C.c_void_p(d_contig_ids), C.c_void_p(d_groups or None),
                                                    C.c_void_p(d_priorities or None), int(n_reads), _p32(lengths),
                                                    lengths.size, int(max_coverage), int(cap),
                                                    START_CAP_SHORTFALL if shortfall else 0, C.c_void_p(d_mask),
                                                    C.c_void_p(d_capped_mask or None), _p64(hist) if hist_bins else None,
                                                    int(hist_bins), C.c_void_p(stream), C.byref(st), C.byref(cs)))
        self.last_stats, self.last_start_cap_stats = st, cs
        return cs.as_dict(), hist[:int(hist_bins)]

    @staticmethod
    def _amplicons_flags(single_end, per_amplicon, complete_pairs):
        return ((AMPLICONS_SINGLE_END if single_end else 0) | (AMPLICONS_PER_AMPLICON if per_amplicon else 0)
                | (AMPLICONS_COMPLETE_PAIRS if complete_pairs else 0))

    @staticmethod
    def _amplicons_tables(n_contigs, amp_offsets, amp_starts, amp_ends, insert_starts, insert_ends):
        offs = None if amp_offsets is None else _u32(amp_offsets)
        if offs is not None:
            assert offs.size == n_contigs + 1, "amp_offsets needs n_contigs + 1 entries"
        n_amp = 0 if offs is None else int(offs[-1])
        cols = [None if a is None else _u32(a) for a in (amp_starts, amp_ends, insert_starts, insert_ends)]
        for a in cols:
            assert a is None or a.size == n_amp, "one entry per amplicon in every table column"
        return offs, n_amp, cols

    def solve_amplicons(self, starts, ends, contig_ids, contig_lengths, max_coverage, amp_offsets, amp_starts, amp_ends,
                        insert_starts=None, insert_ends=None, seq_lengths=None, qualities=None, min_length=0, min_mapq=0,
                        single_end=False, per_amplicon=False, complete_pairs=False, labels=True, rows=True):
        """amplicon-aware downsampling (qmcp_hip_solve_amplicons_host): every unit -- the pair 2q, 2q + 1, or one read
        with single_end -- that passes the length / MAPQ filters is assigned to the amplicon of its contig that contains
        all of it (several: the greatest start, then the smallest end, then the smallest index), its reads are clipped
        to that amplicon's insert [insert_starts[k], insert_ends[k]] (None: the amplicon itself), and the clipped reads
        are solved: pooled per contig, or with per_amplicon one coverage problem per amplicon on its insert.  The
        amplicons of contig c are [amp_offsets[c], amp_offsets[c + 1]) of the table columns.
        -> (mask over the input reads, labels or None (uint32 per unit, NO_AMPLICON: none), rows or None (one
        DEPTH_ROW_DTYPE record per amplicon over its insert: depth of the clipped reads before, of the final mask
        after), stats_dict).  last_stats is the inner solve's, last_amplicons_stats the AmpliconsStats"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        sl = None if seq_lengths is None else _u32(seq_lengths)
        q = None if qualities is None else _u32(qualities)
        assert (sl is None or sl.size == n) and (q is None or q.size == n), "one entry per read in every column"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs, n_amp, (a0, a1, i0, i1) = self._amplicons_tables(lengths.size, amp_offsets, amp_starts, amp_ends,
                                                               insert_starts, insert_ends)
        n_units = n if single_end else n // 2
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        lab = np.full(max(n_units, 1), NO_AMPLICON, dtype=np.uint32) if labels else None
        rws = np.zeros(max(n_amp, 1), dtype=DEPTH_ROW_DTYPE) if rows else None
        st, ast = Stats(), AmpliconsStats()
        _check(_hip.qmcp_hip_solve_amplicons_host(
            self._ctx, _p32(starts), _p32(ends), _p32(ids), _p32(sl), _p32(q), n, _p32(lengths), lengths.size, _p32(offs),
            _p32(a0), _p32(a1), _p32(i0), _p32(i1), int(min_length), int(min_mapq), int(max_coverage),
            self._amplicons_flags(single_end, per_amplicon, complete_pairs), _p64(mask), _p32(lab),
            C.c_void_p(rws.ctypes.data) if rows else None, C.byref(st), C.byref(ast)))
        self.last_stats, self.last_amplicons_stats = st, ast
        return (mask[:mask_words(n)], lab[:n_units] if labels else None, rws[:n_amp] if rows else None, ast.as_dict())

    def solve_amplicons_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, max_coverage, d_mask,
                               amp_offsets, amp_starts, amp_ends, insert_starts=None, insert_ends=None, d_seq_lengths=0,
                               d_qualities=0, min_length=0, min_mapq=0, single_end=False, per_amplicon=False,
                               complete_pairs=False, labels=True, rows=True, stream=0):
        """the same on device pointers (ints; 0: no lengths / no qualities); the mask is written to d_mask, the tables,
        labels and rows stay on the host.  With pairs the columns must be 8-byte aligned (QMCP_EINVAL otherwise).
        -> (labels or None, rows or None, stats_dict)"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs, n_amp, (a0, a1, i0, i1) = self._amplicons_tables(lengths.size, amp_offsets, amp_starts, amp_ends,
                                                               insert_starts, insert_ends)
        n = int(n_reads)
        n_units = n if single_end else n // 2
        lab = np.full(max(n_units, 1), NO_AMPLICON, dtype=np.uint32) if labels else None
        rws = np.zeros(max(n_amp, 1), dtype=DEPTH_ROW_DTYPE) if rows else None
        st, ast = Stats(), AmpliconsStats()
        _check(_hip.qmcp_hip_solve_amplicons_device(
            self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends), C.c_void_p(d_contig_ids), C.c_void_p(d_seq_lengths or None),
            C.c_void_p(d_qualities or None), n, _p32(lengths), lengths.size, _p32(offs), _p32(a0), _p32(a1), _p32(i0),
            _p32(i1), int(min_length), int(min_mapq), int(max_coverage),
            self._amplicons_flags(single_end, per_amplicon, complete_pairs), C.c_void_p(d_mask), _p32(lab),
            C.c_void_p(rws.ctypes.data) if rows else None, C.c_void_p(stream), C.byref(st), C.byref(ast)))
        self.last_stats, self.last_amplicons_stats = st, ast
        return lab[:n_units] if labels else None, rws[:n_amp] if rows else None, ast.as_dict()

    @staticmethod
    def _target_tables(n_contigs, target_offsets, target_starts, target_ends):
        offs = None if target_offsets is None else _u32(target_offsets)
        t0 = None if target_starts is None else _u32(target_starts)
        t1 = None if target_ends is None else _u32(target_ends)
        if offs is not None:
            assert offs.size == n_contigs + 1, "target_offsets needs n_contigs + 1 entries"
            n_reg = int(offs[-1])
            assert (t0 is None or t0.size >= n_reg) and (t1 is None or t1.size >= n_reg), \
                "target_starts / target_ends are shorter than target_offsets says"
        return offs, t0, t1

    def solve_targets(self, starts, ends, contig_ids, contig_lengths, max_coverage, target_offsets, target_starts,
                      target_ends, padding=0, qualities=None, keep_off_target=False):
        """on-target downsampling (qmcp_hip_solve_targets_host): coverage capped at max_coverage inside the target
        regions only -- contig c owns regions [target_offsets[c], target_offsets[c + 1]) of target_starts / target_ends
        (inclusive, any order, overlaps allowed), each widened by `padding`.  Reads that touch no target are dropped, or
        all kept with keep_off_target=True.  qualities: the quality pass on the projected problem.  Host keep bitmask in
        INPUT order out; the projected solve's stats go to last_stats, the pass around it to last_target_stats"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        q = None if qualities is None else _u32(qualities)
        n = starts.size
        assert ends.size == n and ids.size == n and (q is None or q.size == n), "one entry per read in every column"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs, t0, t1 = self._target_tables(lengths.size, target_offsets, target_starts, target_ends)
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st, ts = Stats(), TargetStats()
        _check(_hip.qmcp_hip_solve_targets_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), _p32(q), n, _p32(lengths),
                                                lengths.size, _p32(offs), _p32(t0), _p32(t1), int(padding),
                                                int(max_coverage), TARGETS_KEEP_OFF_TARGET if keep_off_target else 0,
                                                _p64(mask), C.byref(st), C.byref(ts)))
        self.last_stats, self.last_target_stats = st, ts
        return mask[:mask_words(n)]

    def solve_targets_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, max_coverage, target_offsets,
                             target_starts, target_ends, d_mask, padding=0, d_qualities=0, keep_off_target=False,
                             stream=0):
        """solve_targets on device pointers (ints; d_qualities 0: none); the input-order mask is written to d_mask.
        Returns the target stats"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs, t0, t1 = self._target_tables(lengths.size, target_offsets, target_starts, target_ends)
        st, ts = Stats(), TargetStats()
        _check(_hip.qmcp_hip_solve_targets_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                  C.c_void_p(d_contig_ids), C.c_void_p(d_qualities or None), int(n_reads),
                                                  _p32(lengths), lengths.size, _p32(offs), _p32(t0), _p32(t1),
                                                  int(padding), int(max_coverage),
                                                  TARGETS_KEEP_OFF_TARGET if keep_off_target else 0, C.c_void_p(d_mask),
                                                  C.c_void_p(stream), C.byref(st), C.byref(ts)))
        self.last_stats, self.last_target_stats = st, ts
        return ts

    @staticmethod
    def _region_tables(n_contigs, region_offsets, region_starts, region_ends, region_caps):
        if region_offsets is None:
            return None, None, None, None
        offs = _u32(region_offsets)
        assert offs.size == n_contigs + 1, "region_offsets needs n_contigs + 1 entries"
        cols = [None if a is None else _u32(a) for a in (region_starts, region_ends, region_caps)]
        assert all(a is None or a.size >= int(offs[-1]) for a in cols), \
            "region_starts / region_ends / region_caps are shorter than region_offsets says"
        return (offs, *cols)

    def solve_profile(self, starts, ends, contig_ids, contig_lengths, default_cap, region_offsets=None, region_starts=None,
                      region_ends=None, region_caps=None, flags=0):
        """a cap that varies along the genome (qmcp_hip_solve_profile_host): contig c owns regions
        [region_offsets[c], region_offsets[c + 1]) of region_starts / region_ends (inclusive, any order, disjoint per
        contig after clipping) with region_caps; default_cap everywhere else.  The kept set covers every position p
        min(cov(p), cap(p)) times with the fewest reads (the canonical rule).  No regions: solve_by_contig at default_cap.
        Host keep bitmask in INPUT order out; last_stats, last_profile_stats"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs, r0, r1, caps = self._region_tables(lengths.size, region_offsets, region_starts, region_ends, region_caps)
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st, ps = Stats(), ProfileStats()
        _check(_hip.qmcp_hip_solve_profile_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), n, _p32(lengths),
                                                lengths.size, _p32(offs), _p32(r0), _p32(r1), _p32(caps), int(default_cap),
                                                int(flags), _p64(mask), C.byref(st), C.byref(ps)))
        self.last_stats, self.last_profile_stats = st, ps
        return mask[:mask_words(n)]

    def solve_profile_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, default_cap, d_mask,
                             region_offsets=None, region_starts=None, region_ends=None, region_caps=None, flags=0,
                             stream=0):
        """solve_profile on device pointers (ints); the input-order mask is written to d_mask.  Returns the profile stats"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs, r0, r1, caps = self._region_tables(lengths.size, region_offsets, region_starts, region_ends, region_caps)
        st, ps = Stats(), ProfileStats()
        _check(_hip.qmcp_hip_solve_profile_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                  C.c_void_p(d_contig_ids), int(n_reads), _p32(lengths), lengths.size,
                                                  _p32(offs), _p32(r0), _p32(r1), _p32(caps), int(default_cap), int(flags),
                                                  C.c_void_p(d_mask), C.c_void_p(stream), C.byref(st), C.byref(ps)))
        self.last_stats, self.last_profile_stats = st, ps
        return ps

    def solve_ceiling(self, starts, ends, contig_ids, contig_lengths, default_cap, region_offsets=None, region_starts=None,
                      region_ends=None, region_caps=None, flags=0):
        """ceiling downsampling (qmcp_hip_solve_ceiling_host): solve_profile's reads, regions and default_cap, but the
        caps are CEILINGS -- the kept depth is at most cap(p) at every position and as many reads as possible are kept
        (the dropped set is the canonical selection under max(0, cov - cap)).  The depth may fall below min(cov, cap):
        last_ceiling_stats.short_positions / short_bases say where.  flags: CEILING_WHOLE_PAIRS also drops the mate
        (reads 2q, 2q + 1) of every dropped read.  Host keep bitmask in INPUT order out; last_stats, last_ceiling_stats"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs, r0, r1, caps = self._region_tables(lengths.size, region_offsets, region_starts, region_ends, region_caps)
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st, cs = Stats(), CeilingStats()
        _check(_hip.qmcp_hip_solve_ceiling_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), n, _p32(lengths),
                                                lengths.size, _p32(offs), _p32(r0), _p32(r1), _p32(caps), int(default_cap),
                                                int(flags), _p64(mask), C.byref(st), C.byref(cs)))
        self.last_stats, self.last_ceiling_stats = st, cs
        return mask[:mask_words(n)]

    def solve_ceiling_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, default_cap, d_mask,
                             region_offsets=None, region_starts=None, region_ends=None, region_caps=None, flags=0,
                             stream=0):
        """solve_ceiling on device pointers (ints); the input-order mask is written to d_mask.  Returns the ceiling stats"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs, r0, r1, caps = self._region_tables(lengths.size, region_offsets, region_starts, region_ends, region_caps)
        st, cs = Stats(), CeilingStats()
        _check(_hip.qmcp_hip_solve_ceiling_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                  C.c_void_p(d_contig_ids), int(n_reads), _p32(lengths), lengths.size,
                                                  _p32(offs), _p32(r0), _p32(r1), _p32(caps), int(default_cap), int(flags),
                                                  C.c_void_p(d_mask), C.c_void_p(stream), C.byref(st), C.byref(cs)))
        self.last_stats, self.last_ceiling_stats = st, cs
        return cs

    def solve_proportional(self, starts, ends, contig_ids, contig_lengths, proportion, floor=0,
                           max_coverage=2**31 - 1):
        """keep a fraction of the depth everywhere (qmcp_hip_solve_proportional_host): with num / den =
        as_ratio(proportion), the kept set covers every position p at least
        min(cov(p), max_coverage, max(ceil(cov(p) * num / den), floor)) times with the fewest reads (the canonical
        rule): the fraction of the depth rounded up, positions at or below `floor` whole, max_coverage a hard upper
        end of the demand.  proportion 1 (or floor >= max_coverage) is solve_by_contig at max_coverage, proportion 0
        is solve_by_contig at min(floor, max_coverage).  Host keep bitmask in INPUT order out; last_stats,
        last_proportional_stats"""
        num, den = as_ratio(proportion)
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st, ps = Stats(), ProportionalStats()
        _check(_hip.qmcp_hip_solve_proportional_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), n, _p32(lengths),
                                                     lengths.size, num, den, int(floor), int(max_coverage), 0,
                                                     _p64(mask), C.byref(st), C.byref(ps)))
        self.last_stats, self.last_proportional_stats = st, ps
        return mask[:mask_words(n)]

    def solve_proportional_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, proportion, d_mask,
                                  floor=0, max_coverage=2**31 - 1, stream=0):
        """solve_proportional on device pointers (ints); the input-order mask is written to d_mask.  Returns the
        proportional stats"""
        num, den = as_ratio(proportion)
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        st, ps = Stats(), ProportionalStats()
        _check(_hip.qmcp_hip_solve_proportional_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                       C.c_void_p(d_contig_ids), int(n_reads), _p32(lengths), lengths.size,
                                                       num, den, int(floor), int(max_coverage), 0, C.c_void_p(d_mask),
                                                       C.c_void_p(stream), C.byref(st), C.byref(ps)))
        self.last_stats, self.last_proportional_stats = st, ps
        return ps

    @staticmethod
    def _budget_of(budget_reads, fraction, placed):
        """the read budget of a budget solve: budget_reads, or floor(fraction * placed reads)"""
        if (budget_reads is None) == (fraction is None):
            raise ValueError("a budget solve takes exactly one of budget_reads and fraction")
        if budget_reads is not None:
            if int(budget_reads) < 0 or int(budget_reads) >= 1 << 64:
                raise ValueError("budget_reads must fit an unsigned 64-bit count")
            return int(budget_reads)
        if not 0.0 <= float(fraction) <= 1.0:
            raise ValueError("fraction must lie in 0 .. 1")
        if placed is None:
            raise ValueError("fraction needs the number of placed reads (placed_reads=)")
        return int(math.floor(float(fraction) * int(placed)))

    def solve_budget(self, starts, ends, contig_ids, contig_lengths, max_coverage, budget_reads=None, fraction=None,
                     flags=0, curve=False):
        """budget downsampling (qmcp_hip_solve_budget_host): solve_by_contig's reads, and the DEEPEST coverage M* in
        0 .. min(max_coverage, largest depth) whose solve keeps at most budget_reads reads -- or fraction (0 .. 1) of the
        placed reads, floor(fraction * placed), counted from contig_ids here.  flags: BUDGET_WHOLE_PAIRS counts and
        returns whole pairs (reads 2q, 2q + 1) among the placed reads.  -> (mask, M*, BudgetStats), the mask being
        solve_by_contig's at M* bit for bit (all zero for M* == 0); curve=True appends the curve S(M) = sum of
        min(cov, M), M = 0 .. min(top, BUDGET_CURVE_MAX), as a uint64 array.  last_stats: the solve at M*"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        budget = self._budget_of(budget_reads, fraction, int(np.count_nonzero(ids != NO_CONTIG)))
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        cap = BUDGET_CURVE_MAX + 1 if curve else 0
        table = np.zeros(cap, dtype=np.uint64) if curve else None
        st, bs = Stats(), BudgetStats()
        _check(_hip.qmcp_hip_solve_budget_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), n, _p32(lengths),
                                               lengths.size, int(max_coverage), budget, int(flags), _p64(table), cap,
                                               _p64(mask), C.byref(st), C.byref(bs)))
        self.last_stats, self.last_budget_stats = st, bs
        out = (mask[:mask_words(n)], int(bs.coverage), bs)
        return out + (table[:bs.curve_entries],) if curve else out

    def solve_budget_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, max_coverage, d_mask,
                            budget_reads=None, fraction=None, placed_reads=None, flags=0, curve=False, stream=0):
        """solve_budget on device pointers (ints); the input-order mask is written to d_mask.  fraction needs
        placed_reads, the number of ids that are not NO_CONTIG.  -> (M*, BudgetStats), with curve=True also the curve"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        budget = self._budget_of(budget_reads, fraction, placed_reads)
        cap = BUDGET_CURVE_MAX + 1 if curve else 0
        table = np.zeros(cap, dtype=np.uint64) if curve else None
        st, bs = Stats(), BudgetStats()
        _check(_hip.qmcp_hip_solve_budget_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                 C.c_void_p(d_contig_ids), int(n_reads), _p32(lengths), lengths.size,
                                                 int(max_coverage), budget, int(flags), _p64(table), cap,
                                                 C.c_void_p(d_mask), C.c_void_p(stream), C.byref(st), C.byref(bs)))
        self.last_stats, self.last_budget_stats = st, bs
        out = (int(bs.coverage), bs)
        return out + (table[:bs.curve_entries],) if curve else out

    @staticmethod
    def _base_budget_of(mean_depth, budget_bases, positions):
        """the base budget of a mean-depth solve: budget_bases, or floor(mean_depth * positions)"""
        if (mean_depth is None) == (budget_bases is None):
            raise ValueError("a mean-depth solve takes exactly one of mean_depth and budget_bases")
        if budget_bases is not None:
            if int(budget_bases) < 0 or int(budget_bases) >= 1 << 64:
                raise ValueError("budget_bases must fit an unsigned 64-bit count")
            return int(budget_bases)
        mean = float(mean_depth)
        if not (mean >= 0.0 and math.isfinite(mean)):
            raise ValueError("mean_depth must be a finite depth of at least 0")
        budget = int(math.floor(mean * int(positions)))
        if budget >= 1 << 64:
            raise ValueError("mean_depth * positions must fit an unsigned 64-bit count")
        return budget

    def _mean_depth_tables(self, lengths, mean_depth, budget_bases, region_offsets, region_starts, region_ends, curve):
        offs, r0, r1, _ = self._region_tables(lengths.size, region_offsets, region_starts, region_ends, None)
        positions = region_positions(lengths, offs, r0, r1) if mean_depth is not None else None
        budget = self._base_budget_of(mean_depth, budget_bases, positions)
        cap = BUDGET_CURVE_MAX + 1 if curve else 0
        return offs, r0, r1, budget, cap, np.zeros(cap, dtype=np.uint64) if curve else None

    def solve_mean_depth(self, starts, ends, contig_ids, contig_lengths, max_coverage, mean_depth=None, budget_bases=None,
                         region_offsets=None, region_starts=None, region_ends=None, flags=0, curve=False):
        """mean-depth downsampling (qmcp_hip_solve_mean_depth_host): solve_by_contig's reads, and the DEEPEST coverage M*
        in 0 .. min(max_coverage, largest depth) whose solve keeps at most budget_bases bases inside the regions -- or
        mean_depth, a mean over the regions' positions: floor(mean_depth * region_positions(...)).  Contig c owns regions
        [region_offsets[c], region_offsets[c + 1]) of region_starts / region_ends (inclusive, any order, overlaps
        allowed, clipped to the contig); region_offsets=None: every position.  flags: MEAN_DEPTH_WHOLE_PAIRS counts and
        returns whole pairs (reads 2q, 2q + 1) among the placed reads.  -> (mask, M*, MeanDepthStats), the mask being
        solve_by_contig's at M* bit for bit (all zero for M* == 0); curve=True appends S_R(M) = sum over the regions of
        min(cov, M), M = 0 .. min(top, BUDGET_CURVE_MAX), as a uint64 array.  last_stats: the solve at M*"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs, r0, r1, budget, cap, table = self._mean_depth_tables(lengths, mean_depth, budget_bases, region_offsets,
                                                                   region_starts, region_ends, curve)
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st, ms = Stats(), MeanDepthStats()
        _check(_hip.qmcp_hip_solve_mean_depth_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), n, _p32(lengths),
                                                   lengths.size, int(max_coverage), budget, _p32(offs), _p32(r0), _p32(r1),
                                                   int(flags), _p64(table), cap, _p64(mask), C.byref(st), C.byref(ms)))
        self.last_stats, self.last_mean_depth_stats = st, ms
        out = (mask[:mask_words(n)], int(ms.coverage), ms)
        return out + (table[:ms.curve_entries],) if curve else out

    def solve_mean_depth_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, max_coverage, d_mask,
                                mean_depth=None, budget_bases=None, region_offsets=None, region_starts=None,
                                region_ends=None, flags=0, curve=False, stream=0):
        """solve_mean_depth on device pointers (ints); the region tables are host arrays, the input-order mask is
        written to d_mask.  -> (M*, MeanDepthStats), with curve=True also the curve"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs, r0, r1, budget, cap, table = self._mean_depth_tables(lengths, mean_depth, budget_bases, region_offsets,
                                                                   region_starts, region_ends, curve)
        st, ms = Stats(), MeanDepthStats()
        _check(_hip.qmcp_hip_solve_mean_depth_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                     C.c_void_p(d_contig_ids), int(n_reads), _p32(lengths), lengths.size,
                                                     int(max_coverage), budget, _p32(offs), _p32(r0), _p32(r1), int(flags),
                                                     _p64(table), cap, C.c_void_p(d_mask), C.c_void_p(stream),
                                                     C.byref(st), C.byref(ms)))
        self.last_stats, self.last_mean_depth_stats = st, ms
        out = (int(ms.coverage), ms)
        return out + (table[:ms.curve_entries],) if curve else out

    @staticmethod
    def _thresholds_counts(coverage_lo, coverage_hi, counts):
        cap = max(int(coverage_hi) - int(coverage_lo) + 1, 0) if counts else 0
        if cap > THRESHOLDS_COVERAGE_MAX:  # (the call refuses such a range)
            cap = THRESHOLDS_COVERAGE_MAX
        return cap, np.zeros(max(cap, 1), dtype=np.uint64) if counts else None

    def solve_thresholds(self, starts, ends, contig_ids, contig_lengths, coverage_hi, coverage_lo=1, flags=0, counts=False):
        """coverage thresholds (qmcp_hip_solve_thresholds_host): solve_by_contig's reads, and per read the SMALLEST
        coverage M in coverage_lo .. coverage_hi at which solve_by_contig keeps it -- THRESHOLD_NEVER for an unplaced read
        and for one that no such M keeps.  One grouping, one whole solve per coverage from coverage_lo up, stopping once
        every placed read has a threshold (ThresholdsStats.top).  While ThresholdsStats.nesting_violations is 0 -- it has
        been on every input seen; not proven -- threshold_mask(thresholds, M) is solve_by_contig's mask at M bit for bit
        for every M of the range.  flags: THRESHOLDS_WHOLE_PAIRS gives a placed read the smaller of its own and its
        placed mate's threshold (reads 2q, 2q + 1).  -> (thresholds uint16, ThresholdsStats); counts=True appends the
        reads with threshold <= M for M = coverage_lo .. coverage_hi as a uint64 array.  last_stats: the last solve"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        cap, table = self._thresholds_counts(coverage_lo, coverage_hi, counts)
        thr = np.full(max(n, 1), THRESHOLD_NEVER, dtype=np.uint16)
        st, ts = Stats(), ThresholdsStats()
        _check(_hip.qmcp_hip_solve_thresholds_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), n, _p32(lengths),
                                                   lengths.size, int(coverage_lo), int(coverage_hi), int(flags),
                                                   thr.ctypes.data_as(_u16p), _p64(table), cap, C.byref(st), C.byref(ts)))
        self.last_stats, self.last_thresholds_stats = st, ts
        out = (thr[:n], ts)
        return out + (table[:ts.count_entries],) if counts else out

    def solve_thresholds_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, coverage_hi, d_thresholds,
                                coverage_lo=1, flags=0, counts=False, stream=0):
        """solve_thresholds on device pointers (ints); the uint16 thresholds are written to d_thresholds (n_reads
        entries).  -> ThresholdsStats, with counts=True (ThresholdsStats, counts)"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        cap, table = self._thresholds_counts(coverage_lo, coverage_hi, counts)
        st, ts = Stats(), ThresholdsStats()
        _check(_hip.qmcp_hip_solve_thresholds_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                     C.c_void_p(d_contig_ids), int(n_reads), _p32(lengths), lengths.size,
                                                     int(coverage_lo), int(coverage_hi), int(flags),
                                                     C.c_void_p(d_thresholds), _p64(table), cap, C.c_void_p(stream),
                                                     C.byref(st), C.byref(ts)))
        self.last_stats, self.last_thresholds_stats = st, ts
        return (ts, table[:ts.count_entries]) if counts else ts

    def solve_pairs(self, starts, ends, contig_ids, contig_lengths, max_coverage, stages=None):
        """pair-aware downsampling (qmcp_hip_solve_pairs_host): reads (2q, 2q + 1) are pair q, stages the rising targets
        T_1 < ... < T_k = max_coverage (None: ceil(M / 2), then M).  Stage 1 is solve_by_contig at T_1 with the pairs
        completed; every further stage credits the depth of the reads already kept and tops up to its target among the
        others, then completes the pairs again.  -> (mask, stats, pair_stats): the host keep bitmask in INPUT order (whole
        pairs), stage 1's Stats, the PairStats.  Also left in last_stats / last_pair_stats"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        tg = None if stages is None else np.atleast_1d(np.ascontiguousarray(stages, dtype=np.uint32))
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st, ps = Stats(), PairStats()
        _check(_hip.qmcp_hip_solve_pairs_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), n, _p32(lengths),
                                              lengths.size, int(max_coverage), _p32(tg), 0 if tg is None else tg.size,
                                              _p64(mask), C.byref(st), C.byref(ps)))
        self.last_stats, self.last_pair_stats = st, ps
        return mask[:mask_words(n)], st, ps

    def solve_pairs_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, max_coverage, d_mask, stages=None,
                           stream=0):
        """solve_pairs on device pointers (ints); the input-order mask is written to d_mask.  -> (stats, pair_stats)"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        tg = None if stages is None else np.atleast_1d(np.ascontiguousarray(stages, dtype=np.uint32))
        st, ps = Stats(), PairStats()
        _check(_hip.qmcp_hip_solve_pairs_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                C.c_void_p(d_contig_ids), int(n_reads), _p32(lengths), lengths.size,
                                                int(max_coverage), _p32(tg), 0 if tg is None else tg.size,
                                                C.c_void_p(d_mask), C.c_void_p(stream), C.byref(st), C.byref(ps)))
        self.last_stats, self.last_pair_stats = st, ps
        return st, ps

    def solve_templates(self, starts, ends, contig_ids, template_ids, n_templates, contig_lengths, max_coverage,
                        stages=None):
        """template-aware downsampling (qmcp_hip_solve_templates_host): every row is a segment, template_ids[i] <
        n_templates names its template (a single-end read, a pair, the pieces of a split read, the aligned blocks of a
        spliced read and its mate), stages as in solve_pairs.  The staged solve of solve_pairs with the completion by
        template: a template is kept whole or not at all; depth is counted per segment.  -> (mask, stats,
        template_stats): the host keep bitmask in INPUT order, stage 1's Stats, the TemplateStats.  Also left in
        last_stats / last_template_stats"""
        starts, ends, ids, tids = _u32(starts), _u32(ends), _u32(contig_ids), _u32(template_ids)
        n = starts.size
        assert ends.size == n and ids.size == n and tids.size == n, \
            "starts, ends, contig_ids and template_ids must have one entry per segment"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        tg = None if stages is None else np.atleast_1d(np.ascontiguousarray(stages, dtype=np.uint32))
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st, ts = Stats(), TemplateStats()
        _check(_hip.qmcp_hip_solve_templates_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), _p32(tids), n,
                                                  int(n_templates), _p32(lengths), lengths.size, int(max_coverage),
                                                  _p32(tg), 0 if tg is None else tg.size, _p64(mask), C.byref(st),
                                                  C.byref(ts)))
        self.last_stats, self.last_template_stats = st, ts
        return mask[:mask_words(n)], st, ts

    def solve_templates_device(self, d_starts, d_ends, d_contig_ids, d_template_ids, n_reads, n_templates, contig_lengths,
                               max_coverage, d_mask, stages=None, stream=0):
        """solve_templates on device pointers (ints); the input-order mask is written to d_mask.  -> (stats,
        template_stats)"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        tg = None if stages is None else np.atleast_1d(np.ascontiguousarray(stages, dtype=np.uint32))
        st, ts = Stats(), TemplateStats()
        _check(_hip.qmcp_hip_solve_templates_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                    C.c_void_p(d_contig_ids), C.c_void_p(d_template_ids), int(n_reads),
                                                    int(n_templates), _p32(lengths), lengths.size, int(max_coverage),
                                                    _p32(tg), 0 if tg is None else tg.size, C.c_void_p(d_mask),
                                                    C.c_void_p(stream), C.byref(st), C.byref(ts)))
        self.last_stats, self.last_template_stats = st, ts
        return st, ts

    def clip_templates(self, starts, ends, contig_ids, template_ids, n_templates, contig_lengths):
        """the overlap clip of fragment depth (qmcp_hip_clip_templates_host): within every (template, contig) group, in
        the order (start, input index), a segment that begins inside what the earlier members cover starts behind it, and
        one that lies wholly inside becomes unplaced.  -> (clipped_starts, clipped_contig_ids, stats) in INPUT order;
        ends do not change.  Depth per segment on the clipped columns (depth_report, depth_track, solve_templates_profile)
        is fragment depth: a template counts once per position.  Also left in last_fragment_stats"""
        starts, ends, ids, tids = _u32(starts), _u32(ends), _u32(contig_ids), _u32(template_ids)
        n = starts.size
        assert ends.size == n and ids.size == n and tids.size == n, \
            "starts, ends, contig_ids and template_ids must have one entry per segment"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        out_s, out_c = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        fs = FragmentStats()
        _check(_hip.qmcp_hip_clip_templates_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), _p32(tids), n,
                                                 int(n_templates), _p32(lengths), lengths.size, _p32(out_s), _p32(out_c),
                                                 C.byref(fs)))
        self.last_fragment_stats = fs
        return out_s[:n], out_c[:n], fs

    def clip_templates_device(self, d_starts, d_ends, d_contig_ids, d_template_ids, n_reads, n_templates, contig_lengths,
                              d_clipped_starts, d_clipped_contig_ids, stream=0):
        """clip_templates on device pointers (ints); the two clipped columns are written to d_clipped_starts and
        d_clipped_contig_ids, which must not overlap the inputs.  -> stats"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        fs = FragmentStats()
        _check(_hip.qmcp_hip_clip_templates_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                   C.c_void_p(d_contig_ids), C.c_void_p(d_template_ids), int(n_reads),
                                                   int(n_templates), _p32(lengths), lengths.size,
                                                   C.c_void_p(d_clipped_starts), C.c_void_p(d_clipped_contig_ids),
                                                   C.c_void_p(stream), C.byref(fs)))
        self.last_fragment_stats = fs
        return fs

    def solve_fragments(self, starts, ends, contig_ids, template_ids, n_templates, contig_lengths, max_coverage,
                        stages=None):
        """template-aware downsampling on FRAGMENT depth (qmcp_hip_solve_fragments_host): solve_templates on
        clip_templates' columns, so that a template counts once where its segments overlap (the two mates of a
        short-insert pair).  -> (mask, stats, template_stats, fragment_stats): whole templates whose fragment depth is at
        least min(fragment depth, max_coverage) everywhere.  Also left in last_stats / last_template_stats /
        last_fragment_stats"""
        starts, ends, ids, tids = _u32(starts), _u32(ends), _u32(contig_ids), _u32(template_ids)
        n = starts.size
        assert ends.size == n and ids.size == n and tids.size == n, \
            "starts, ends, contig_ids and template_ids must have one entry per segment"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        tg = None if stages is None else np.atleast_1d(np.ascontiguousarray(stages, dtype=np.uint32))
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st, ts, fs = Stats(), TemplateStats(), FragmentStats()
        _check(_hip.qmcp_hip_solve_fragments_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), _p32(tids), n,
                                                  int(n_templates), _p32(lengths), lengths.size, int(max_coverage),
                                                  _p32(tg), 0 if tg is None else tg.size, _p64(mask), C.byref(st),
                                                  C.byref(ts), C.byref(fs)))
        self.last_stats, self.last_template_stats, self.last_fragment_stats = st, ts, fs
        return mask[:mask_words(n)], st, ts, fs

    def solve_fragments_device(self, d_starts, d_ends, d_contig_ids, d_template_ids, n_reads, n_templates, contig_lengths,
                               max_coverage, d_mask, stages=None, stream=0):
        """solve_fragments on device pointers (ints); the input-order mask is written to d_mask, the caller's columns are
        not modified.  -> (stats, template_stats, fragment_stats)"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        tg = None if stages is None else np.atleast_1d(np.ascontiguousarray(stages, dtype=np.uint32))
        st, ts, fs = Stats(), TemplateStats(), FragmentStats()
        _check(_hip.qmcp_hip_solve_fragments_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                    C.c_void_p(d_contig_ids), C.c_void_p(d_template_ids), int(n_reads),
                                                    int(n_templates), _p32(lengths), lengths.size, int(max_coverage),
                                                    _p32(tg), 0 if tg is None else tg.size, C.c_void_p(d_mask),
                                                    C.c_void_p(stream), C.byref(st), C.byref(ts), C.byref(fs)))
        self.last_stats, self.last_template_stats, self.last_fragment_stats = st, ts, fs
        return st, ts, fs

    def solve_templates_profile(self, starts, ends, contig_ids, template_ids, n_templates, contig_lengths, max_coverage,
                                default_cap, region_offsets=None, region_starts=None, region_ends=None, region_caps=None,
                                stages=None, flags=0, fragment_depth=False):
        """template-aware downsampling under a cap table (qmcp_hip_solve_templates_profile_host): solve_templates'
        segments and template ids, solve_profile's regions and default_cap.  Stage j of the schedule T_1 < ... < T_k =
        max_coverage (None: ceil(M / 2), then M) runs under ceil(cap(p) * T_j / M), credits the depth of the templates
        already kept and completes the templates again.  -> (mask, stats, template_stats, template_profile_stats): the
        host keep bitmask in INPUT order (whole templates that cover min(cov(p), cap(p)) everywhere), stage 1's Stats,
        the TemplateStats, the TemplateProfileStats.  Also left in last_stats / last_template_stats /
        last_template_profile_stats.  fragment_depth=True: clip_templates runs first and the solve runs on its columns
        (two calls), so the caps bound fragment depth; its stats are left in last_fragment_stats"""
        if fragment_depth:
            starts, contig_ids, _ = self.clip_templates(starts, ends, contig_ids, template_ids, n_templates, contig_lengths)
        starts, ends, ids, tids = _u32(starts), _u32(ends), _u32(contig_ids), _u32(template_ids)
        n = starts.size
        assert ends.size == n and ids.size == n and tids.size == n, \
            "starts, ends, contig_ids and template_ids must have one entry per segment"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs, r0, r1, caps = self._region_tables(lengths.size, region_offsets, region_starts, region_ends, region_caps)
        tg = None if stages is None else np.atleast_1d(np.ascontiguousarray(stages, dtype=np.uint32))
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st, ts, qs = Stats(), TemplateStats(), TemplateProfileStats()
        _check(_hip.qmcp_hip_solve_templates_profile_host(
            self._ctx, _p32(starts), _p32(ends), _p32(ids), _p32(tids), n, int(n_templates), _p32(lengths), lengths.size,
            _p32(offs), _p32(r0), _p32(r1), _p32(caps), int(default_cap), int(flags), int(max_coverage), _p32(tg),
            0 if tg is None else tg.size, _p64(mask), C.byref(st), C.byref(ts), C.byref(qs)))
        self.last_stats, self.last_template_stats, self.last_template_profile_stats = st, ts, qs
        return mask[:mask_words(n)], st, ts, qs

    def solve_templates_profile_device(self, d_starts, d_ends, d_contig_ids, d_template_ids, n_reads, n_templates,
                                       contig_lengths, max_coverage, default_cap, d_mask, region_offsets=None,
                                       region_starts=None, region_ends=None, region_caps=None, stages=None, flags=0,
                                       stream=0, fragment_depth=False, d_clipped_starts=0, d_clipped_contig_ids=0):
        """solve_templates_profile on device pointers (ints); the input-order mask is written to d_mask.  -> (stats,
        template_stats, template_profile_stats).  fragment_depth=True: clip_templates_device runs first, into the two
        device columns the caller provides (d_clipped_starts, d_clipped_contig_ids), and the solve runs on them"""
        if fragment_depth:
            if not d_clipped_starts or not d_clipped_contig_ids:
                raise ValueError("fragment_depth=True needs d_clipped_starts and d_clipped_contig_ids")
            self.clip_templates_device(d_starts, d_ends, d_contig_ids, d_template_ids, n_reads, n_templates,
                                       contig_lengths, d_clipped_starts, d_clipped_contig_ids, stream=stream)
            d_starts, d_contig_ids = d_clipped_starts, d_clipped_contig_ids
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs, r0, r1, caps = self._region_tables(lengths.size, region_offsets, region_starts, region_ends, region_caps)
        tg = None if stages is None else np.atleast_1d(np.ascontiguousarray(stages, dtype=np.uint32))
        st, ts, qs = Stats(), TemplateStats(), TemplateProfileStats()
        _check(_hip.qmcp_hip_solve_templates_profile_device(
            self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends), C.c_void_p(d_contig_ids), C.c_void_p(d_template_ids),
            int(n_reads), int(n_templates), _p32(lengths), lengths.size, _p32(offs), _p32(r0), _p32(r1), _p32(caps),
            int(default_cap), int(flags), int(max_coverage), _p32(tg), 0 if tg is None else tg.size, C.c_void_p(d_mask),
            C.c_void_p(stream), C.byref(st), C.byref(ts), C.byref(qs)))
        self.last_stats, self.last_template_stats, self.last_template_profile_stats = st, ts, qs
        return st, ts, qs

    def _depth_call(self, entry, head, n, lengths, mask_arg, max_coverage, target_offsets, target_starts, target_ends,
                    padding, n_bins, tail):
        offs, t0, t1 = self._target_tables(lengths.size, target_offsets, target_starts, target_ends)
        n_bins = int(n_bins)
        cap = 0 if offs is None else int(offs[-1])
        contig_rows = np.zeros(lengths.size, DEPTH_ROW_DTYPE)
        region_rows = np.zeros(cap, DEPTH_ROW_DTYPE)
        hist_in, hist_kept = np.zeros(max(n_bins, 1), np.uint64), np.zeros(max(n_bins, 1), np.uint64)
        n_rows, st = C.c_uint64(0), DepthStats()
        _check(entry(self._ctx, *head, n, _p32(lengths), lengths.size, mask_arg, int(max_coverage), _p32(offs), _p32(t0),
                     _p32(t1), int(padding), n_bins, contig_rows.ctypes.data, region_rows.ctypes.data, cap,
                     C.byref(n_rows), _p64(hist_in), _p64(hist_kept), *tail, C.byref(st)))
        self.last_depth_stats = st
        return DepthReport(contig_rows, region_rows[:n_rows.value].copy(), hist_in[:n_bins], hist_kept[:n_bins], st)

    def depth_report(self, starts, ends, contig_ids, contig_lengths, max_coverage, keep_mask=None, target_offsets=None,
                     target_starts=None, target_ends=None, padding=0, n_bins=0):
        """depth before and after (qmcp_hip_depth_report_host): the reads of solve_by_contig, a keep mask in input order
        (None: every placed read is kept) and optional regions in solve_targets' CSR form -> a DepthReport with one row
        per contig, one per MERGED region, histograms of both depths over the positions in scope (the regions when given,
        everything otherwise; depth d counts in bin min(d, n_bins - 1)) and the positions short of
        min(coverage, max_coverage).  Computed on the device; nothing per position comes back"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        mask = None
        if keep_mask is not None:
            mask = np.ascontiguousarray(keep_mask, dtype=np.uint64)
            assert mask.size >= mask_words(n), "keep_mask needs ceil(n_reads / 64) words"
        return self._depth_call(_hip.qmcp_hip_depth_report_host, (_p32(starts), _p32(ends), _p32(ids)), n, lengths,
                                _p64(mask), max_coverage, target_offsets, target_starts, target_ends, padding, n_bins, ())

    def depth_report_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, max_coverage, d_keep_mask=0,
                            target_offsets=None, target_starts=None, target_ends=None, padding=0, n_bins=0, stream=0):
        """depth_report on device pointers (ints; d_keep_mask 0: every placed read is kept); the tables and the report
        itself are host memory"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        head = (C.c_void_p(d_starts), C.c_void_p(d_ends), C.c_void_p(d_contig_ids))
        return self._depth_call(_hip.qmcp_hip_depth_report_device, head, int(n_reads), lengths,
                                C.c_void_p(d_keep_mask or None), max_coverage, target_offsets, target_starts, target_ends,
                                padding, n_bins, (C.c_void_p(stream),))

    def _track_call(self, entry, head, n, lengths, mask_arg, max_coverage, target_offsets, target_starts, target_ends,
                    padding, channels, short_only, skip_zero, depth_cap, tail):
        offs, t0, t1 = self._target_tables(lengths.size, target_offsets, target_starts, target_ends)
        flags = track_flags(channels, short_only, skip_zero)
        # the header's bound on the runs: 2 x reads + contigs + regions (the merged regions are no more than those given)
        bound = 2 * int(n) + int(lengths.size) + (0 if offs is None else int(offs[-1]))
        capacity = min(bound, TRACK_FIRST_CAPACITY)
        for attempt in range(2):
            runs = np.zeros(capacity, TRACK_RUN_DTYPE)
            n_runs, st = C.c_uint64(0), TrackStats()
            rc = entry(self._ctx, *head, n, _p32(lengths), lengths.size, mask_arg, int(max_coverage), _p32(offs), _p32(t0),
                       _p32(t1), int(padding), flags, int(depth_cap), runs.ctypes.data, capacity, C.byref(n_runs), *tail,
                       C.byref(st))
            if rc == QMCP_ERANGE and attempt == 0 and n_runs.value > capacity:
                capacity = int(n_runs.value)          # the exact count, once
                continue
            _check(rc)
            break
        self.last_track_stats = st
        return runs[:n_runs.value].copy(), st

    def depth_track(self, starts, ends, contig_ids, contig_lengths, max_coverage, keep_mask=None, target_offsets=None,
                    target_starts=None, target_ends=None, padding=0, channels=("in", "kept"), short_only=False,
                    skip_zero=False, depth_cap=0):
        """per-base depth before and after as runs (qmcp_hip_depth_track_host): depth_report's inputs -> (runs, stats),
        runs a numpy structured array of TRACK_RUN_DTYPE in ascending (contig, start) order -- one record per maximal
        interval [start, end] of one contig (and one merged region, when regions are given) on which depth_in =
        min(cov, depth_cap), depth_kept = min(kept, depth_cap) and short = [kept < min(cov, max_coverage)] are constant.
        channels: which of "in" and "kept" are compared and reported (the other is 0); short_only: only short positions;
        skip_zero: no positions whose selected channels are all 0 (genomecov -bg); depth_cap 0: no clamp.
        stats (TrackStats, also last_track_stats): short_positions counts every short position in scope whatever the
        flags.  write_bedgraph turns the runs into a file"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        mask = None
        if keep_mask is not None:
            mask = np.ascontiguousarray(keep_mask, dtype=np.uint64)
            assert mask.size >= mask_words(n), "keep_mask needs ceil(n_reads / 64) words"
        return self._track_call(_hip.qmcp_hip_depth_track_host, (_p32(starts), _p32(ends), _p32(ids)), n, lengths,
                                _p64(mask), max_coverage, target_offsets, target_starts, target_ends, padding, channels,
                                short_only, skip_zero, depth_cap, ())

    def depth_track_device(self, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, max_coverage, d_keep_mask=0,
                           target_offsets=None, target_starts=None, target_ends=None, padding=0, channels=("in", "kept"),
                           short_only=False, skip_zero=False, depth_cap=0, stream=0):
        """depth_track on device pointers (ints; d_keep_mask 0: every placed read is kept); the tables, the runs and
        the stats are host memory"""
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        head = (C.c_void_p(d_starts), C.c_void_p(d_ends), C.c_void_p(d_contig_ids))
        return self._track_call(_hip.qmcp_hip_depth_track_device, head, int(n_reads), lengths,
                                C.c_void_p(d_keep_mask or None), max_coverage, target_offsets, target_starts, target_ends,
                                padding, channels, short_only, skip_zero, depth_cap, (C.c_void_p(stream),))

    def solve64(self, start_inds, end_inds, contig_lengths, max_coverage, contig_read_offsets=None):
        """the reference's own size_t columns in (qmcp_hip_solve_host64: narrowed inside the library),
        host keep bitmask out; self.last_breakdown tells how (threads, chunks, columns sent)"""
        s64 = np.ascontiguousarray(start_inds, dtype=np.uint64)
        e64 = np.ascontiguousarray(end_inds, dtype=np.uint64)
        n = s64.size
        offs, lengths = _contig_tables(n, contig_read_offsets, contig_lengths)
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        st, bd = Stats(), HostBreakdown()
        _check(_hip.qmcp_hip_solve_host64(self._ctx, _p64(s64), _p64(e64), n, _p64(offs), _p32(lengths),
                                          lengths.size, int(max_coverage), _p64(mask), C.byref(st), C.byref(bd)))
        self.last_stats, self.last_breakdown = st, bd
        return mask[:mask_words(n)]

    def solve_device(self, d_starts, d_ends, n_reads, contig_lengths, max_coverage, d_mask,
                     contig_read_offsets=None, stream=0):
        """device pointers (ints) in; the mask is written to d_mask (device pointer)"""
        offs, lengths = _contig_tables(n_reads, contig_read_offsets, contig_lengths)
        st = Stats()
        _check(_hip.qmcp_hip_solve_device(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                          int(n_reads), _p64(offs), _p32(lengths), lengths.size,
                                          int(max_coverage), C.c_void_p(d_mask),
                                          C.c_void_p(stream), C.byref(st)))
        self.last_stats = st
        return st

    def get_options(self):
        o = Options()
        _check(_hip.qmcp_hip_get_options(self._ctx, C.byref(o)))
        return o

    def set_options(self, options=None, **fields):
        """qmcp_hip_set_options: `options` (an Options; default: the library's defaults) with `fields` set on top --
        e.g. set_options(sweep="ev", cut_points=1); sweep takes "fast" | "gen" | "ev" or a SWEEP_* number"""
        o = Options()
        if options is not None:
            C.memmove(C.byref(o), C.byref(options), C.sizeof(Options))
        else:
            _hip.qmcp_hip_default_options(C.byref(o))
        for k, v in fields.items():
            if k == "sweep" and not isinstance(v, int):
                v = _SWEEP_NAMES[v]
            if not hasattr(o, k) or k == "struct_size":
                raise AttributeError(f"qmcp_hip_options has no field {k!r}")
            setattr(o, k, v)
        o.struct_size = C.sizeof(Options)
        _check(_hip.qmcp_hip_set_options(self._ctx, C.byref(o)))

    @contextlib.contextmanager
    def options(self, **fields):
        """with solver.options(sweep="ev"): ...   -- the fields on top of the current options, restored afterwards"""
        old = self.get_options()
        self.set_options(old, **fields)
        try:
            yield self
        finally:
            self.set_options(old)

    def solve_device_begin(self, d_starts, d_ends, n_reads, contig_lengths, max_coverage, d_mask,
                           contig_read_offsets=None, stream=0):
        """enqueue a device-resident solve and return without waiting for it (one pending solve per
        Solver; pipeline with a second Solver on the same device); solve_end() collects it"""
        offs, lengths = _contig_tables(n_reads, contig_read_offsets, contig_lengths)
        _check(_hip.qmcp_hip_solve_device_begin(self._ctx, C.c_void_p(d_starts), C.c_void_p(d_ends),
                                                int(n_reads), _p64(offs), _p32(lengths), lengths.size,
                                                int(max_coverage), C.c_void_p(d_mask), C.c_void_p(stream)))

    def solve_end(self):
        st = Stats()
        _check(_hip.qmcp_hip_solve_end(self._ctx, C.byref(st)))
        self.last_stats = st
        return st

    def coverage(self, starts, ends, contig_lengths, contig_read_offsets=None, keep_mask=None):
        starts, ends = _u32(starts), _u32(ends)
        n = starts.size
        offs, lengths = _contig_tables(n, contig_read_offsets, contig_lengths)
        cov = np.zeros(max(int(lengths.sum()), 1), dtype=np.uint32)
        if keep_mask is None:
            _check(_hip.qmcp_hip_coverage_host(self._ctx, _p32(starts), _p32(ends), n, _p64(offs),
                                               _p32(lengths), lengths.size, _p32(cov)))
        else:
            km = np.ascontiguousarray(keep_mask, dtype=np.uint64)
            _check(_hip.qmcp_hip_filtered_coverage_host(self._ctx, _p32(starts), _p32(ends), n,
                                                        _p64(offs), _p32(lengths), lengths.size,
                                                        _p64(km), _p32(cov)))
        return cov[:int(lengths.sum())]

    def demand(self, starts, ends, ref_genome_length, max_coverage):
        """(b, d) of the reference's flow network for one contig, computed on the device:
        create_b_function / create_demand_function, quasi_mcp_cpu_max_flow_solver.cpp:58-87"""
        s, e = _u32(starts), _u32(ends)
        b = np.zeros(int(ref_genome_length) + 1, np.int32)
        d = np.zeros(int(ref_genome_length) + 1, np.int32)
        _check(_hip.qmcp_hip_demand_host(self._ctx, _p32(s), _p32(e), s.size, int(ref_genome_length),
                                         int(max_coverage), b.ctypes.data_as(C.POINTER(C.c_int32)),
                                         d.ctypes.data_as(C.POINTER(C.c_int32))))
        return b, d

    def complete_pairs(self, mask, n_reads):
        out = np.ascontiguousarray(mask, dtype=np.uint64).copy()
        _check(_hip.qmcp_hip_complete_pairs_host(self._ctx, _p64(out), int(n_reads)))
        return out

    def complete_pairs_device(self, d_mask, n_reads, stream=0):
        _check(_hip.qmcp_hip_complete_pairs_device(self._ctx, C.c_void_p(d_mask), int(n_reads),
                                                   C.c_void_p(stream)))

    def filter_solve(self, starts, ends, ref_genome_length, max_coverage, amp_starts=None,
                     amp_ends=None, seq_lengths=None, qualities=None, min_length=0, min_mapq=0,
                     complete_pairs=False):
        """FILTER -> compaction -> solve -> (find_pairs) in one device-resident call; returns
        (keep mask over the ORIGINAL read indices, number of pairs the pre-pass dropped)"""
        starts, ends = _u32(starts), _u32(ends)
        n = starts.size
        a0 = _u32(amp_starts) if amp_starts is not None else None
        a1 = _u32(amp_ends) if amp_ends is not None else None
        sl = _u32(seq_lengths) if seq_lengths is not None else None
        q = _u32(qualities) if qualities is not None else None
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        dropped = C.c_uint64(0)
        st = Stats()
        _check(_hip.qmcp_hip_filter_solve_host(self._ctx, _p32(starts), _p32(ends), _p32(sl), _p32(q), n,
                                               _p32(a0), _p32(a1), 0 if a0 is None else a0.size,
                                               int(min_length), int(min_mapq), int(ref_genome_length),
                                               int(max_coverage), int(bool(complete_pairs)),
                                               _p64(mask), C.byref(dropped), C.byref(st)))
        self.last_stats = st
        return mask[:mask_words(n)], int(dropped.value)

    def filter_solve_by_contig(self, starts, ends, contig_ids, contig_lengths, max_coverage, amp_offsets=None,
                               amp_starts=None, amp_ends=None, seq_lengths=None, qualities=None, min_length=0,
                               min_mapq=0, complete_pairs=False):
        """filter_solve for pairs on several contigs (qmcp_hip_filter_solve_by_contig_host): the amplicons of contig c
        are [amp_offsets[c], amp_offsets[c + 1]) of amp_starts / amp_ends (amp_offsets None: IGNORE, only the length /
        MAPQ filters act); a pair survives iff both mates lie on one contig, inside one of its amplicons.  Returns
        (keep mask over the ORIGINAL read indices, number of pairs the FILTER dropped)"""
        starts, ends, ids = _u32(starts), _u32(ends), _u32(contig_ids)
        n = starts.size
        assert ends.size == n and ids.size == n, "starts, ends and contig_ids must have one entry per read"
        lengths = np.atleast_1d(np.ascontiguousarray(contig_lengths, dtype=np.uint32))
        offs = _u32(amp_offsets) if amp_offsets is not None else None
        if offs is not None:
            assert offs.size == lengths.size + 1, "amp_offsets needs n_contigs + 1 entries"
        a0 = _u32(amp_starts) if amp_starts is not None else None
        a1 = _u32(amp_ends) if amp_ends is not None else None
        sl = _u32(seq_lengths) if seq_lengths is not None else None
        q = _u32(qualities) if qualities is not None else None
        mask = np.zeros(max(mask_words(n), 1), dtype=np.uint64)
        dropped = C.c_uint64(0)
        st = Stats()
        _check(_hip.qmcp_hip_filter_solve_by_contig_host(self._ctx, _p32(starts), _p32(ends), _p32(ids), _p32(sl),
                                                         _p32(q), n, _p32(lengths), lengths.size, _p32(offs),
                                                         _p32(a0), _p32(a1), int(min_length), int(min_mapq),
                                                         int(max_coverage), int(bool(complete_pairs)), _p64(mask),
                                                         C.byref(dropped), C.byref(st)))
        self.last_stats = st
        return mask[:mask_words(n)], int(dropped.value)

    def amplicon_filter(self, starts, ends, amp_starts, amp_ends, seq_lengths=None, qualities=None,
                        min_length=0, min_mapq=0):
        starts, ends = _u32(starts), _u32(ends)
        a0, a1 = _u32(amp_starts), _u32(amp_ends)
        sl = _u32(seq_lengths) if seq_lengths is not None else None
        q = _u32(qualities) if qualities is not None else None
        n = starts.size
        out = np.zeros(max(mask_words(n // 2), 1), dtype=np.uint64)
        _check(_hip.qmcp_hip_amplicon_filter_host(self._ctx, _p32(starts), _p32(ends), _p32(sl),
                                                  _p32(q), n, _p32(a0), _p32(a1), a0.size,
                                                  int(min_length), int(min_mapq), _p64(out)))
        return out[:mask_words(n // 2)]


# ---------------------------------------------------------------- host mirror (libqmcp_host.so)
class MultiSolver:
    """several devices behind one call (qmcp_hip_multi_*): contigs dealt to the devices by cost, one
    context and one host thread per entry of `devices` (a device may be named more than once)"""

    def __init__(self, devices):
        self.devices = [int(d) for d in devices]
        arr = (C.c_int * len(self.devices))(*self.devices)
        self._m = C.c_void_p()
        _check(_hip.qmcp_hip_multi_create(arr, len(self.devices), C.byref(self._m)))
        self.last_stats = []
        self.last_assignment = None

    def close(self):
        if getattr(self, "_m", None):
            _hip.qmcp_hip_multi_destroy(self._m)
            self._m = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def solve(self, starts, ends, contig_lengths, max_coverage, contig_read_offsets=None):
        starts, ends = _u32(starts), _u32(ends)
        offs, lengths = _contig_tables(starts.size, contig_read_offsets, contig_lengths)
        mask = np.zeros(mask_words(starts.size), dtype=np.uint64)
        stats = (Stats * len(self.devices))()
        where = (C.c_int * lengths.size)()
        _check(_hip.qmcp_hip_multi_solve_host(self._m, _p32(starts), _p32(ends), starts.size, _p64(offs),
                                              _p32(lengths), lengths.size, int(max_coverage), _p64(mask),
                                              stats, where))
        self.last_stats = list(stats)
        self.last_assignment = list(where)
        return mask


def _need_host():
    if _host is None:
        raise ImportError(f"{HOST_LIB_PATH} is missing: build it with `make lib`")


def reads_gen(kind, pairs, genome_length, read_length=150, seed=12345, with_qualities=False,
              aos=False):
    """reads-gen restatement (libs/reads-gen): returns (starts, ends[, qualities]) as uint32"""
    _need_host()
    n = 2 * int(pairs)
    s = np.empty(n, dtype=np.uint32)
    e = np.empty(n, dtype=np.uint32)
    q = np.empty(n, dtype=np.uint32) if with_qualities else None
    fn = _host.qmcp_host_reads_gen_aos if aos else _host.qmcp_host_reads_gen
    rc = fn(int(seed), int(kind), int(pairs), int(genome_length), int(read_length), _p32(s), _p32(e),
            _p32(q))
    if rc != 0:
        raise ValueError(f"reads_gen failed ({rc})")
    return (s, e, q) if with_qualities else (s, e)


def amplicons_from_files(bed_path, tsv_path=None):
    """BED (+ optional TSV) -> (amp_starts, amp_ends), as BamApi::set_amplicon_filter builds them"""
    _need_host()
    cap = 1 << 16
    a0 = np.empty(cap, dtype=np.uint32)
    a1 = np.empty(cap, dtype=np.uint32)
    n = _host.qmcp_host_amplicons_from_files(str(bed_path).encode(),
                                             str(tsv_path).encode() if tsv_path else None,
                                             _p32(a0), _p32(a1), cap)
    if n < 0:
        raise OSError(f"cannot build amplicon set from {bed_path} / {tsv_path} ({n})")
    return a0[:n].copy(), a1[:n].copy()


def amplicons_by_reference(bed_path, tsv_path, reference_names):
    """BED (+ optional TSV) matched to references by name (BamApiConfig::amplicons_by_reference) -> (offsets, starts,
    ends): reference c owns amplicons [offsets[c], offsets[c + 1]).  ValueError naming an unknown chrom or a TSV pair
    across references"""
    _need_host()
    names = [str(n) for n in reference_names]
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    cap = 1 << 20
    offs = np.zeros(len(names) + 1, dtype=np.uint32)
    a0 = np.empty(cap, dtype=np.uint32)
    a1 = np.empty(cap, dtype=np.uint32)
    err = C.create_string_buffer(1024)
    n = _host.qmcp_host_amplicons_by_reference(str(bed_path).encode(), str(tsv_path).encode() if tsv_path else None,
                                               arr, len(names), _p32(offs), _p32(a0), _p32(a1), cap, err, 1024)
    if n == -4:
        raise ValueError(err.value.decode())
    if n < 0:
        raise OSError(f"cannot build amplicons by reference from {bed_path} / {tsv_path} ({n})")
    return offs, a0[:n].copy(), a1[:n].copy()


def amplicon_inserts_by_reference(bed_path, tsv_path, reference_names):
    """the inserts and left primer names of amplicons_by_reference's amplicons, in the same order -> (insert_starts,
    insert_ends, left_names).  From BED primers [ls, le) and [rs, re) the amplicon is [ls, re] (the reference's
    inclusive quirk) and the insert [le, rs - 1], inclusive: what Solver.solve_amplicons takes as insert_starts /
    insert_ends.  ValueError for what amplicons_by_reference refuses and for a primer pair that leaves no insert (its
    primers touch or overlap), naming the pair"""
    _need_host()
    names = [str(n) for n in reference_names]
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    cap = 1 << 20
    i0 = np.empty(cap, dtype=np.uint32)
    i1 = np.empty(cap, dtype=np.uint32)
    buf = C.create_string_buffer(1 << 24)
    err = C.create_string_buffer(1024)
    fn = _host.qmcp_host_amplicon_inserts_by_reference
    fn.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_uint64, _u32p, _u32p, C.c_uint64, C.c_char_p,
                   C.c_size_t, C.c_char_p, C.c_size_t]
    fn.restype = C.c_int64
    n = fn(str(bed_path).encode(), str(tsv_path).encode() if tsv_path else None, arr, len(names), _p32(i0), _p32(i1), cap,
           buf, len(buf), err, 1024)
    if n == -4:
        raise ValueError(err.value.decode())
    if n < 0:
        raise OSError(f"cannot build amplicon inserts by reference from {bed_path} / {tsv_path} ({n})")
    return i0[:n].copy(), i1[:n].copy(), buf.value.decode().split("\n")[:n]


def write_amplicon_report(path, chroms, amp_starts, amp_ends, left_names, units, reads_kept, rows):
    """the TSV of downsample_bam(amplicon_report=): one line per amplicon -- chrom, amplicon start / end, insert start /
    end (rows' start / end: the insert the solve used), left primer, units assigned, reads kept, minimum and mean depth
    over the insert before and after, positions short of min(before, max_coverage).  chroms, amp_starts, amp_ends,
    left_names, units and reads_kept hold one entry per amplicon; rows are Solver.solve_amplicons' (DEPTH_ROW_DTYPE
    records, or tuples in that field order)"""
    with open(path, "w") as f:
        f.write("#chrom\tamplicon_start\tamplicon_end\tinsert_start\tinsert_end\tleft_primer\tunits\treads_kept\t"
                "min_depth_in\tmean_depth_in\tmin_depth_kept\tmean_depth_kept\tdeficit_positions\n")
        for k, row in enumerate(rows):
            r = dict(zip(DEPTH_ROW_DTYPE.names, (int(x) for x in tuple(row))))
            f.write(f"{chroms[k]}\t{int(amp_starts[k])}\t{int(amp_ends[k])}\t{r['start']}\t{r['end']}\t{left_names[k]}\t"
                    f"{int(units[k])}\t{int(reads_kept[k])}\t{r['min_in']}\t{r['sum_in'] / r['positions']:.6f}\t"
                    f"{r['min_kept']}\t{r['sum_kept'] / r['positions']:.6f}\t{r['deficit_positions']}\n")


def targets_from_bed(bed_path, reference_names):
    """target regions from a BED file (BED3+, further columns ignored) matched to references by name -> (offsets, starts,
    ends) as Solver.solve_targets takes them: reference c owns regions [offsets[c], offsets[c + 1]), in file order.  BED
    is 0-based half-open, so a line "chrom s e" is the inclusive region [s, e - 1]; `track`, `browser` and `#` lines and
    blank lines are skipped.  ValueError naming a chrom that matches no reference exactly, or a malformed line"""
    names = [str(n) for n in reference_names]
    index = {}
    for k, name in enumerate(names):
        index.setdefault(name, k)
    per_ref = [[] for _ in names]
    with open(bed_path) as bed:
        for lineno, line in enumerate(bed, 1):
            text = line.strip()
            if not text or text.startswith("#") or text.split()[0] in ("track", "browser"):
                continue
            fields = text.split("\t") if "\t" in text else text.split()
            if len(fields) < 3:
                raise ValueError(f"{bed_path}:{lineno}: a BED line needs chrom, start and end")
            chrom = fields[0]
            try:
                start, end = int(fields[1]), int(fields[2])
            except ValueError:
                raise ValueError(f"{bed_path}:{lineno}: start and end must be integers") from None
            if start < 0 or end <= start or end > 0xFFFFFFFF:
                raise ValueError(f"{bed_path}:{lineno}: region [{start}, {end}) is empty or out of range")
            if chrom not in index:
                raise ValueError(f"{bed_path}:{lineno}: chrom {chrom!r} matches no reference of the file")
            per_ref[index[chrom]].append((start, end - 1))
    offsets = np.zeros(len(names) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(r) for r in per_ref])
    flat = [reg for r in per_ref for reg in r]
    t0 = np.array([a for a, _ in flat], dtype=np.uint32)
    t1 = np.array([b for _, b in flat], dtype=np.uint32)
    return offsets, t0, t1


def targets_as_regions(target_offsets, target_starts, target_ends, contig_lengths, padding, cap):
    """target regions (as targets_from_bed gives them: CSR per contig, inclusive bounds, any order, overlapping and
    nested allowed) as a cap table for Solver.solve_profile / solve_templates_profile -> (offsets, starts, ends, caps):
    per contig, by the rule of qmcp_hip_solve_targets_*, every region padded to [start - padding, end + padding] (the
    start saturating at 0), clipped to [0, length - 1] (dropped when it begins at or beyond the contig's length), sorted,
    overlapping and adjacent regions merged; every merged region carries `cap`.  ValueError for offsets that do not fit
    the contigs, a region with start > end, or a cap outside [0, 2^31)"""
    lengths = np.atleast_1d(np.asarray(contig_lengths, dtype=np.int64))
    offs = np.atleast_1d(np.asarray(target_offsets, dtype=np.int64))
    t0 = np.atleast_1d(np.asarray(target_starts, dtype=np.int64))
    t1 = np.atleast_1d(np.asarray(target_ends, dtype=np.int64))
    padding, cap = int(padding), int(cap)
    if offs.size != lengths.size + 1 or offs[0] != 0 or np.any(np.diff(offs) < 0) or offs[-1] > min(t0.size, t1.size):
        raise ValueError("target_offsets needs one entry per contig plus one, starting at 0 and never decreasing")
    if np.any(t0[:offs[-1]] > t1[:offs[-1]]):
        raise ValueError("a target region has start > end")
    if padding < 0 or cap < 0 or cap >= 1 << 31:
        raise ValueError("padding must not be negative and the cap must lie in [0, 2^31)")
    out_offs, out0, out1 = [0], [], []
    for c, length in enumerate(lengths.tolist()):
        a = np.maximum(t0[offs[c]:offs[c + 1]] - padding, 0)
        b = np.minimum(t1[offs[c]:offs[c + 1]] + padding, length - 1)
        inside = a < length
        order = np.argsort(a[inside], kind="stable")
        first = len(out0)
        for lo, hi in zip(a[inside][order].tolist(), b[inside][order].tolist()):
            if len(out0) > first and lo <= out1[-1] + 1:
                out1[-1] = max(out1[-1], hi)
            else:
                out0.append(lo)
                out1.append(hi)
        out_offs.append(len(out0))
    u = lambda x: np.asarray(x, dtype=np.uint32)
    return u(out_offs), u(out0), u(out1), np.full(len(out0), cap, dtype=np.uint32)


def profile_from_bedgraph(path, reference_names):
    """a coverage profile from a bedGraph file (four columns: chrom start end cap) matched to references by name ->
    (offsets, starts, ends, caps) as Solver.solve_profile takes them: reference c owns regions
    [offsets[c], offsets[c + 1]), ascending and disjoint.  bedGraph is 0-based half-open, so a line "chrom s e cap" is
    the inclusive region [s, e - 1]; `track`, `browser` and `#` lines and blank lines are skipped.  Overlapping lines are
    flattened here with the LATER line winning (the C ABI takes disjoint regions only); neighbouring pieces with one
    cap are joined.  ValueError naming a chrom that matches no reference exactly, a cap that is no integer in
    [0, 2^31), or a malformed line"""
    names = [str(n) for n in reference_names]
    index = {}
    for k, name in enumerate(names):
        index.setdefault(name, k)
    per_ref = [[] for _ in names]
    with open(path) as src:
        for lineno, line in enumerate(src, 1):
            text = line.strip()
            if not text or text.startswith("#") or text.split()[0] in ("track", "browser"):
                continue
            fields = text.split("\t") if "\t" in text else text.split()
            if len(fields) < 4:
                raise ValueError(f"{path}:{lineno}: a bedGraph line needs chrom, start, end and cap")
            chrom = fields[0]
            try:
                start, end = int(fields[1]), int(fields[2])
            except ValueError:
                raise ValueError(f"{path}:{lineno}: start and end must be integers") from None
            try:
                cap = int(fields[3])
            except ValueError:
                raise ValueError(f"{path}:{lineno}: the cap {fields[3]!r} is not an integer") from None
            if start < 0 or end <= start or end > 0xFFFFFFFF:
                raise ValueError(f"{path}:{lineno}: region [{start}, {end}) is empty or out of range")
            if cap < 0 or cap >= 1 << 31:
                raise ValueError(f"{path}:{lineno}: the cap {cap} is not in [0, 2^31)")
            if chrom not in index:
                raise ValueError(f"{path}:{lineno}: chrom {chrom!r} matches no reference of the file")
            per_ref[index[chrom]].append((start, end - 1, cap))
    flat_refs = []
    for lines in per_ref:
        # elementary intervals between the lines' bounds; each takes the cap of the last line that covers it (a sweep
        # with a heap of the covering lines, latest on top, ended lines dropped lazily)
        cuts = sorted({a for a, _, _ in lines} | {b + 1 for _, b, _ in lines})
        order = sorted(range(len(lines)), key=lambda i: lines[i][0])
        live, nxt, pieces = [], 0, []
        for lo, hi in zip(cuts, cuts[1:]):
            while nxt < len(order) and lines[order[nxt]][0] <= lo:
                heapq.heappush(live, -order[nxt])
                nxt += 1
            while live and lines[-live[0]][1] < lo:
                heapq.heappop(live)
            if not live:
                continue
            cap = lines[-live[0]][2]
            if pieces and pieces[-1][1] + 1 == lo and pieces[-1][2] == cap:
                pieces[-1][1] = hi - 1
            else:
                pieces.append([lo, hi - 1, cap])
        flat_refs.append(pieces)
    offsets = np.zeros(len(names) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(r) for r in flat_refs])
    flat = [reg for r in flat_refs for reg in r]
    return (offsets, np.array([a for a, _, _ in flat], dtype=np.uint32), np.array([b for _, b, _ in flat], dtype=np.uint32),
            np.array([c for _, _, c in flat], dtype=np.uint32))


def window_regions(contig_lengths, size):
    """fixed windows of `size` positions over every contig (the last window of a contig is shorter), in the CSR form
    depth_report and solve_targets take: (offsets, starts, ends), inclusive bounds -- the regions of a mosdepth-style "--by size" report.  The report merges adjacent regions like
    overlapping ones (target_table.h's rule), so windows passed as they are come back as one row per contig; shorten
    each by one position (ends - 1 where ends > starts) to keep one row per window"""
    size = int(size)
    if size < 1:
        raise ValueError("window size must be at least 1")
    lengths = np.atleast_1d(np.asarray(contig_lengths, dtype=np.int64))
    counts = (lengths + size - 1) // size
    offsets = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    if offsets[-1] >= 1 << 32:
        raise ValueError("more than 2^32 - 1 windows")
    within = np.arange(offsets[-1], dtype=np.int64) - np.repeat(offsets[:-1], counts)
    starts = within * size
    ends = np.minimum(starts + size, np.repeat(lengths, counts)) - 1
    return offsets.astype(np.uint32), starts.astype(np.uint32), ends.astype(np.uint32)


DEPTH_REPORT_COLUMNS = ("kind", "reference", "start", "end", "positions", "mean_in", "mean_kept", "min_in", "max_in",
                        "min_kept", "max_kept", "capped_positions", "deficit_positions", "deficit_sum")


def tiers_from_mapq(mapq, thresholds):
    """MAPQ bands as tiers for Solver.solve_tiers: thresholds must fall strictly (e.g. [30, 10, 0]); mapq >=
    thresholds[0] is tier 0, thresholds[0] > mapq >= thresholds[1] tier 1, and so on; a value below the last threshold
    is NO_TIER.  -> uint32 array, one tier per read; the number of tiers is len(thresholds)"""
    th = [int(x) for x in np.atleast_1d(thresholds).tolist()]
    if not th or any(x < 0 for x in th):
        raise ValueError("thresholds must be a non-empty list of non-negative MAPQ values")
    if any(a <= b for a, b in zip(th, th[1:])):
        raise ValueError(f"thresholds must fall strictly, not {th}")
    if len(th) > TIERS_MAX:
        raise ValueError(f"at most {TIERS_MAX} tiers, not {len(th)}")
    q = np.asarray(mapq).astype(np.int64)
    rising = np.array(th[::-1], dtype=np.int64)
    at_least = np.searchsorted(rising, q, side="right")         # the thresholds a value reaches
    return np.where(at_least == 0, NO_TIER, len(th) - at_least).astype(np.uint32)


def write_tiers_report(path, rows, bands, total_length, records_written=None, mates_added=None):
    """the TSV of a tiered solve: a '#'-prefixed header line, then one line per tier -- its band (`bands`: one label per
    tier, e.g. "mapq>=30"), reads, kept, mean depth before and after (bases / total_length, six decimals), demand and
    asked positions --, then records_written and mates_added as name<TAB>value lines when given.  rows: a list of
    TierRow"""
    total = float(total_length) if total_length else 1.0
    with open(path, "w") as out:
        out.write("#tier\tband\treads\tkept\tmean_depth_in\tmean_depth_kept\tdemand\tasked_positions\n")
        for t, (row, band) in enumerate(zip(rows, bands)):
            out.write(f"{t}\t{band}\t{row.n_reads}\t{row.n_kept}\t{row.bases_in / total:.6f}\t"
                      f"{row.bases_kept / total:.6f}\t{row.demand}\t{row.asked_positions}\n")
        if records_written is not None:
            out.write(f"records_written\t{int(records_written)}\n")
        if mates_added is not None:
            out.write(f"mates_added\t{int(mates_added)}\n")


def write_depth_report(path, report, reference_names):
    """a DepthReport as TSV: a '#'-prefixed header line (DEPTH_REPORT_COLUMNS), then one line per contig row and one per
    region row -- start 0-based, end exclusive (BED style), the means with six decimals.  Histograms, when the report
    has any, follow as '#hist' comment lines (bin, positions before, positions after)"""
    names = list(reference_names)
    with open(path, "w") as f:
        f.write("#" + "\t".join(DEPTH_REPORT_COLUMNS) + "\n")
        for kind, rows in (("contig", report.contig_rows), ("region", report.region_rows)):
            for r in rows:
                pos = int(r["positions"])
                end = int(r["end"]) + 1 if pos else int(r["start"])
                mean_in = int(r["sum_in"]) / pos if pos else 0.0
                mean_kept = int(r["sum_kept"]) / pos if pos else 0.0
                f.write("\t".join([kind, names[int(r["contig"])], str(int(r["start"])), str(end), str(pos),
                                   f"{mean_in:.6f}", f"{mean_kept:.6f}", str(int(r["min_in"])), str(int(r["max_in"])),
                                   str(int(r["min_kept"])), str(int(r["max_kept"])), str(int(r["capped_positions"])),
                                   str(int(r["deficit_positions"])), str(int(r["deficit_sum"]))]) + "\n")
        for b in range(len(report.hist_in)):
            f.write(f"#hist\t{b}\t{int(report.hist_in[b])}\t{int(report.hist_kept[b])}\n")


def track_flags(channels=("in", "kept"), short_only=False, skip_zero=False):
    """the QMCP_TRACK_* word of Solver.depth_track's keywords; channels: "in", "kept", "both" or a collection of the
    first two"""
    if isinstance(channels, str):
        channels = ("in", "kept") if channels == "both" else (channels,)
    channels = tuple(channels)
    if not channels or any(ch not in ("in", "kept") for ch in channels):
        raise ValueError(f'channels must name "in", "kept" or both, not {channels!r}')
    return (TRACK_IN if "in" in channels else 0) | (TRACK_KEPT if "kept" in channels else 0) | \
        (TRACK_SHORT_ONLY if short_only else 0) | (TRACK_SKIP_ZERO if skip_zero else 0)


def write_bedgraph(path, runs, reference_names, channel="kept"):
    """the runs of Solver.depth_track as bedGraph: chrom<TAB>start<TAB>end + 1<TAB>value, 0-based half-open, in the runs'
    order; channel "kept" or "in" writes that depth, "both" writes depth_in and depth_kept as two value columns under a
    '#chrom start end depth_in depth_kept' header line.  Neighbouring runs of one contig that touch and have the same
    written value(s) are joined, so the file does not depend on the channels the call compared.  profile_from_bedgraph
    reads a one-channel file back.  Returns the number of lines written (without the header)"""
    if channel not in ("kept", "in", "both"):
        raise ValueError(f'channel must be "kept", "in" or "both", not {channel!r}')
    names = [str(x) for x in reference_names]
    runs = np.asarray(runs)
    contig = runs["contig"].astype(np.int64)
    start, end = runs["start"].astype(np.int64), runs["end"].astype(np.int64)
    values = [runs["depth_in"]] if channel == "in" else [runs["depth_kept"]] if channel == "kept" else \
        [runs["depth_in"], runs["depth_kept"]]
    if runs.size:
        joined = (contig[1:] == contig[:-1]) & (start[1:] == end[:-1] + 1)
        for v in values:
            joined &= v[1:] == v[:-1]
        first = np.flatnonzero(np.concatenate([[True], ~joined]))
        last = np.concatenate([first[1:] - 1, [runs.size - 1]])
    else:
        first = last = np.zeros(0, np.int64)
    with open(path, "w") as f:
        if channel == "both":
            f.write("#chrom\tstart\tend\tdepth_in\tdepth_kept\n")
        cols = [[names[c] for c in contig[first].tolist()], start[first].tolist(), (end[last] + 1).tolist()] + \
            [v[first].tolist() for v in values]
        f.writelines("\t".join(map(str, line)) + "\n" for line in zip(*cols))
    return int(first.size)


def _reference_table(path):
    """the BAM header's references, in header order -> (names, lengths)"""
    _need_host()
    buf = C.create_string_buffer(1 << 24)
    lengths = np.empty(1 << 24, dtype=np.uint32)
    n = _host.qmcp_host_reference_names(str(path).encode(), buf, len(buf), _p32(lengths), lengths.size)
    if n < 0:
        raise OSError(f"reference_names({path}) failed ({n}): {buf.value.decode(errors='replace') if n == -1 else ''}")
    return [x for x in buf.value.decode().split("\n") if x][:n], lengths[:n].copy()


def reference_names(path):
    """the BAM header's reference names, in header order"""
    return _reference_table(path)[0]


def bamapi_probe(starts, ends, ref_genome_length, ids, layout=0):
    """in-memory BamApi of the host mirror: (find_input_cover, find_filtered_cover(ids), find_pairs(ids))"""
    _need_host()
    starts, ends = _u32(starts), _u32(ends)
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    cin = np.zeros(max(ref_genome_length, 1), dtype=np.uint32)
    cout = np.zeros(max(ref_genome_length, 1), dtype=np.uint32)
    paired = np.zeros(max(starts.size, 1), dtype=np.uint64)
    n = _host.qmcp_host_bamapi_probe(_p32(starts), _p32(ends), starts.size, int(ref_genome_length),
                                     int(layout), _p64(ids), ids.size, _p32(cin), _p32(cout),
                                     _p64(paired))
    if n < 0:
        raise RuntimeError("bamapi probe failed")
    return cin[:ref_genome_length], cout[:ref_genome_length], paired[:n].copy()


def solver_names():
    _need_host()
    buf = C.create_string_buffer(4096)
    n = _host.qmcp_host_solver_names(buf, len(buf))
    if n < 0:
        raise RuntimeError("solver name buffer too small")
    return [x for x in buf.value.decode().split("\n") if x]


def solver_uses_quality(solver_name):
    """Solver::uses_quality_of_reads() of the default manager's solvers and of "quasi-mcp-hip-quality" (True / False),
    None for an unknown name; builds nothing on the device"""
    _need_host()
    rc = _host.qmcp_host_solver_uses_quality(solver_name.encode())
    return None if rc < 0 else bool(rc)


def host_solve(solver_name, starts, ends, ref_genome_length, max_coverage, with_pairs=False, qualities=None,
               adapter_pairs=False):
    """SolverManager::get(name).solve(M, BamApi) through the C++ adapter; ascending ReadIndex.  qualities (one per read)
    go into the reads' quality field (otherwise 0); "quasi-mcp-hip-quality" is resolved beside the default manager.
    adapter_pairs=True (with qualities only): the adapter completes mate pairs on the device (set_complete_pairs)"""
    _need_host()
    starts, ends = _u32(starts), _u32(ends)
    kept = np.empty(max(starts.size, 1), dtype=np.uint64)
    assert qualities is not None or not adapter_pairs, "adapter_pairs goes through the entry with qualities"
    if qualities is None:
        n = _host.qmcp_host_solve(solver_name.encode(), _p32(starts), _p32(ends), starts.size,
                                  int(ref_genome_length), int(max_coverage), int(bool(with_pairs)),
                                  _p64(kept))
    else:
        q = _u32(qualities)
        assert q.size == starts.size, "one quality per read"
        n = _host.qmcp_host_solve_with_qualities(solver_name.encode(), _p32(starts), _p32(ends), _p32(q), starts.size,
                                                 int(ref_genome_length), int(max_coverage), int(bool(with_pairs)),
                                                 int(bool(adapter_pairs)), _p64(kept))
    if n < 0:
        raise KeyError(solver_name)
    return kept[:n].copy()


def plugin_solve_timed(solver_name, starts, ends, ref_genome_length, max_coverage):
    """the reference's "solve took" span (src/app.cpp:132-139) at the plugin boundary: a BamApi holding
    SOAPairedReads (size_t columns) -> Solver::solve -> Solution.  Returns (kept ReadIndex array, dict of
    host wall-clock milliseconds)"""
    _need_host()
    starts, ends = _u32(starts), _u32(ends)
    kept = np.empty(max(starts.size, 1), dtype=np.uint64)
    t = (C.c_float * 9)()
    n = _host.qmcp_host_plugin_solve_timed(solver_name.encode(), _p32(starts), _p32(ends), starts.size,
                                           int(ref_genome_length), int(max_coverage), _p64(kept), t)
    if n < 0:
        raise KeyError(solver_name)
    names = ("solve_call_ms", "library_ms", "narrow_h2d_ms", "device_solve_ms", "d2h_ms", "expand_ms")
    out = {k: round(float(t[i]), 3) for i, k in enumerate(names)}
    out["host_threads"], out["chunks"], out["columns_sent"] = int(t[6]), int(t[7]), int(t[8])
    return kept[:n].copy(), out


def write_synthetic_bam(path, ref_length, names, flags, pos, mapq, clip_front, match, deletion, match2):
    """single-reference BAM whose record i has qname "q<names[i]>" and CIGAR <clip>S<match>M<del>D<match2>M
    (zero-length parts left out); written by the in-repo BGZF writer (tests only)"""
    _need_host()
    n = len(names)
    a = lambda x, t: np.ascontiguousarray(x, dtype=t)
    names, pos, clip_front, match, deletion, match2 = (a(x, np.uint32) for x in (names, pos, clip_front, match, deletion, match2))
    flags, mapq = a(flags, np.uint16), a(mapq, np.uint8)
    rc = _host.qmcp_host_write_synthetic_bam(str(path).encode(), int(ref_length), n, _p32(names),
                                             flags.ctypes.data_as(C.POINTER(C.c_uint16)), _p32(pos),
                                             mapq.ctypes.data_as(C.POINTER(C.c_uint8)), _p32(clip_front),
                                             _p32(match), _p32(deletion), _p32(match2))
    if rc != 0:
        raise OSError(f"cannot write {path}")


def read_bam(path, bed=None, tsv=None, amplicon_mode=0, min_length=0, min_mapq=0, capacity=1 << 24,
             per_reference=False, amplicons_by_reference=False, stratify=None, templates=False, split_spliced=True,
             include_secondary=False):
    """BamApi(path, config).get_paired_reads_soa() of the host mirror: dict of columns + filtered-out ids.
    templates=True (BamApiConfig::template_aware; needs per_reference=True, takes no amplicon files and no stratify,
    ValueError otherwise): one SEGMENT per aligned block of every record instead of paired reads -- a record is cut at
    every N of its CIGAR (split_spliced=False: one segment per record), D stays inside its block, an unmapped record
    (flag 0x4 or refID -1) is one NO_CONTIG segment, secondary records (0x100) are skipped and listed in filtered_out
    unless include_secondary=True, supplementary records (0x800) are taken, and a CG:B,I field replaces the placeholder
    CIGAR <l_seq>S<rlen>N.  A template is the accepted records of one QNAME; min_mapq / min_length drop a template when
    any of its accepted mapped records fails.  Columns: starts, ends, contig_ids, template_ids (dense, in order of first
    appearance), qualities, seq_lengths, segment_records (each segment's BAM record id), in file order, a record's
    blocks left to right; plus n_templates, contig_lengths and filtered_out.
    stratify ("strand" | "read_group"; BamApiConfig::stratify_by, needs per_reference=True and no amplicon files,
    ValueError otherwise): also "strata" (one stratum id per read) and "stratum_names" -- ["+", "-"] (flag 0x10), or the
    header's @RG IDs in header order followed by "*" for records without an RG:Z field the header lists.
    per_reference=True (BamApiConfig::per_reference): also "contig_ids" (each read's refID, NO_CONTIG if unmapped) and
    "contig_lengths" (every reference's length, header order); amplicons are refused there (ValueError) unless
    amplicons_by_reference=True (BamApiConfig::amplicons_by_reference: BED chroms matched to the references by name;
    only with per_reference, ValueError otherwise)"""
    _need_host()
    if templates:
        if not per_reference:
            raise ValueError("read_bam(templates=True) needs per_reference=True")
        if bed or tsv or amplicons_by_reference:
            raise ValueError("read_bam(templates=True) does not take amplicon files")
        if stratify is not None:
            raise ValueError("read_bam(templates=True) does not take stratify")
        return _read_bam_templates(path, min_length, min_mapq, split_spliced, include_secondary, capacity)
    if not split_spliced or include_secondary:
        raise ValueError("split_spliced and include_secondary need templates=True")
    if stratify is not None:
        if stratify not in ("strand", "read_group"):
            raise ValueError(f'stratify must be "strand" or "read_group", not {stratify!r}')
        if not per_reference:
            raise ValueError("stratified downsampling needs per_reference=True")
        if bed or tsv or amplicons_by_reference:
            raise ValueError("read_bam(stratify=...) does not take amplicon files")
        return _read_bam_stratified(path, stratify, min_length, min_mapq, capacity)
    if amplicons_by_reference:
        return _read_bam_by_reference(path, bed, tsv, amplicon_mode, per_reference, min_length, min_mapq, capacity)
    if per_reference:
        return _read_bam_per_reference(path, bed, tsv, min_length, min_mapq, capacity)
    ids = np.empty(capacity, np.uint64)
    cols = {k: np.empty(capacity, np.uint32) for k in ("starts", "ends", "qualities", "seq_lengths")}
    first = np.empty(capacity, np.uint8)
    filt = np.empty(capacity, np.uint64)
    nf, ref = C.c_uint64(0), C.c_uint32(0)
    n = _host.qmcp_host_read_bam(str(path).encode(), str(bed).encode() if bed else None,
                                 str(tsv).encode() if tsv else None, int(amplicon_mode), int(min_length),
                                 int(min_mapq), capacity, _p64(ids), _p32(cols["starts"]), _p32(cols["ends"]),
                                 _p32(cols["qualities"]), _p32(cols["seq_lengths"]),
                                 first.ctypes.data_as(C.POINTER(C.c_uint8)), capacity, _p64(filt), C.byref(nf),
                                 C.byref(ref))
    if n < 0:
        raise OSError(f"read_bam({path}) failed ({n})")
    out = {k: v[:n].copy() for k, v in cols.items()}
    out.update(bam_ids=ids[:n].copy(), is_first=first[:n].astype(bool), filtered_out=filt[:nf.value].copy(),
               ref_genome_length=int(ref.value))
    return out


# the column arguments of the qmcp_host_read_bam_* entries that hand out paired reads, in their order
_PAIRED_COLUMNS = (("bam_ids", np.uint64), ("starts", np.uint32), ("ends", np.uint32), ("qualities", np.uint32),
                   ("seq_lengths", np.uint32), ("is_first", np.uint8), ("contig_ids", np.uint32))


def _read_bam_call(entry, path, head, capacity, columns, what, tail=(), ref_capacity=1 << 24):
    """one qmcp_host_read_bam_* call on buffers of `capacity` entries: (path, *head, capacity, one buffer per (name,
    dtype) of `columns`, the filtered-out ids, the reference lengths, *tail, the message) -> the columns cut to the
    entry's count, with filtered_out and contig_lengths.  -4 raises ValueError with the entry's message, another
    negative return OSError naming the call as read_bam(path<what>)"""
    bufs = {name: np.empty(capacity, dtype) for name, dtype in columns}
    filt, refs = np.empty(capacity, np.uint64), np.empty(ref_capacity, np.uint32)
    nf, nr = C.c_uint64(0), C.c_uint64(0)
    err = C.create_string_buffer(1024)
    pointers = (b.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(b.dtype))) for b in bufs.values())
    n = entry(str(path).encode(), *head, capacity, *pointers, capacity, _p64(filt), C.byref(nf), ref_capacity, _p32(refs),
              C.byref(nr), *tail, err, 1024)
    if n == -4:
        raise ValueError(err.value.decode())
    if n < 0:
        message = err.value.decode(errors="replace")
        raise OSError(f"read_bam({path}{what}) failed ({n})" + (f": {message}" if message else ""))
    out = {name: b[:n].copy() for name, b in bufs.items()}
    out.update(filtered_out=filt[:nf.value].copy(), contig_lengths=refs[:nr.value].copy())
    if "is_first" in out:
        out.update(is_first=out["is_first"].astype(bool),
                   ref_genome_length=int(out["contig_lengths"][0]) if out["contig_lengths"].size else 0)
    return out


def _read_bam_per_reference(path, bed, tsv, min_length, min_mapq, capacity):
    head = (str(bed).encode() if bed else None, str(tsv).encode() if tsv else None, int(min_length), int(min_mapq))
    return _read_bam_call(_host.qmcp_host_read_bam_per_reference, path, head, capacity, _PAIRED_COLUMNS,
                          ", per_reference=True")


def _read_bam_by_reference(path, bed, tsv, amplicon_mode, per_reference, min_length, min_mapq, capacity):
    head = (str(bed).encode() if bed else None, str(tsv).encode() if tsv else None, int(amplicon_mode),
            int(bool(per_reference)), 1, int(min_length), int(min_mapq))
    return _read_bam_call(_host.qmcp_host_read_bam_by_reference, path, head, capacity, _PAIRED_COLUMNS,
                          ", amplicons_by_reference=True")


def _read_bam_stratified(path, stratify, min_length, min_mapq, capacity, names_capacity=1 << 22):
    names, ns = C.create_string_buffer(names_capacity), C.c_uint64(0)
    out = _read_bam_call(_host.qmcp_host_read_bam_stratified, path, (stratify.encode(), int(min_length), int(min_mapq)),
                         capacity, _PAIRED_COLUMNS + (("strata", np.uint32),), f", stratify={stratify!r}",
                         tail=(names, names_capacity, C.byref(ns), 1))
    out["stratum_names"] = names.value.decode().split("\n")[:ns.value]
    return out


def _read_bam_templates(path, min_length, min_mapq, split_spliced, include_secondary, capacity):
    columns = tuple((k, np.uint32) for k in ("starts", "ends", "contig_ids", "template_ids", "qualities", "seq_lengths"))
    nt = C.c_uint64(0)
    out = _read_bam_call(_host.qmcp_host_read_bam_templates, path,
                         (int(min_length), int(min_mapq), int(bool(split_spliced)), int(bool(include_secondary))), capacity,
                         columns + (("segment_records", np.uint64),), ", templates=True", tail=(C.byref(nt),))
    out["n_templates"] = int(nt.value)
    return out


def check_bam(path):
    """read_bam's own verdict on a file (no exit-on-error as in BamApi): (True, reads imported, "") or
    (False, 0, the reader's message)"""
    _need_host()
    n = C.c_uint64(0)
    buf = C.create_string_buffer(512)
    rc = _host.qmcp_host_check_bam(str(path).encode(), C.byref(n), buf, 512)
    return rc == 0, int(n.value) if rc == 0 else 0, buf.value.decode(errors="replace")


def copy_records(in_path, out_path, ids):
    """BamApi::write_bam: the header and the records with the given running ids, to a BAM (".bam") or to SAM text"""
    _need_host()
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    err = C.create_string_buffer(512)
    _host.qmcp_host_copy_records.restype = C.c_int64
    _host.qmcp_host_copy_records.argtypes = [C.c_char_p, C.c_char_p, _u64p, C.c_uint64, C.c_char_p, C.c_size_t]
    n = _host.qmcp_host_copy_records(str(in_path).encode(), str(out_path).encode(), _p64(ids), ids.size, err, 512)
    if n < 0:
        raise OSError(err.value.decode())
    return int(n)


def copy_records_tagged(in_path, out_path, ids, values, tag="XC"):
    """copy_records with the aux field <tag>:S:<values[k]> appended to the record ids[k] -- five bytes, block_size grown by
    five; <tag>:i:<value> in SAM text.  OSError, before anything is written, for a tag that is not [A-Za-z][A-Za-z0-9]
    and for a record that carries the tag already"""
    _need_host()
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    values = np.ascontiguousarray(values, dtype=np.uint16)
    assert ids.size == values.size, "one value per record"
    err = C.create_string_buffer(512)
    _host.qmcp_host_copy_records_tagged.restype = C.c_int64
    _host.qmcp_host_copy_records_tagged.argtypes = [C.c_char_p, C.c_char_p, _u64p, _u16p, C.c_uint64, C.c_char_p,
                                                    C.c_char_p, C.c_size_t]
    n = _host.qmcp_host_copy_records_tagged(str(in_path).encode(), str(out_path).encode(), _p64(ids),
                                            values.ctypes.data_as(_u16p), ids.size, str(tag).encode(), err, 512)
    if n < 0:
        raise OSError(err.value.decode())
    return int(n)


def check_targets_config(in_path, targets, per_reference=True, target_padding=0):
    """BamApi(in_path, BamApiConfig{targets_filepath, target_padding, per_reference}) without a solve: the number of
    regions it parsed.  ValueError with BamApi's message when it refuses (targets without per_reference, a chrom that
    names no reference, a malformed line)"""
    _need_host()
    err = C.create_string_buffer(1024)
    n_regions = C.c_uint64(0)
    rc = _host.qmcp_host_check_targets_config(str(in_path).encode(), str(targets).encode() if targets else None,
                                              int(bool(per_reference)), int(target_padding), C.byref(n_regions), err,
                                              1024)
    if rc == -4:
        raise ValueError(err.value.decode())
    if rc < 0:
        raise OSError(f"check_targets_config({in_path}) failed ({rc})")
    return int(n_regions.value)


def write_template_report(path, template_stats, records_written=None, template_profile_stats=None):
    """downsample_bam(template_report=)'s TSV: the TemplateStats as stat<TAB>value lines (the per-stage arrays as
    stage<j>_<name>), then one size<TAB>templates line per bin of the template-size histogram (1 .. 7, 8+).  With the
    TemplateProfileStats of a call under a cap table: segments_on_cap, templates_on_cap, regions_in, regions_used and
    positions_in_regions as well"""
    ts = template_stats
    k = ts.n_stages
    with open(path, "w") as f:
        f.write("#stat\tvalue\n")
        if records_written is not None:
            f.write(f"records_written\t{int(records_written)}\n")
        f.write(f"templates_used\t{ts.n_templates_used}\ntemplates_kept\t{ts.n_templates_kept}\n")
        f.write(f"segments_kept\t{ts.n_kept[k - 1] if k else 0}\nmax_template_size\t{ts.max_template_size}\n")
        if template_profile_stats is not None:
            qs = template_profile_stats
            f.write(f"segments_on_cap\t{qs.n_segments_on_cap}\ntemplates_on_cap\t{qs.n_templates_on_cap}\n")
            f.write(f"regions_in\t{qs.regions_in}\nregions_used\t{qs.regions_used}\n")
            f.write(f"positions_in_regions\t{qs.positions_in_regions}\n")
        f.write(f"stages\t{k}\n")
        for j in range(k):
            for name in ("target", "n_selected", "n_kept", "capped_positions", "demand", "sweeps"):
                f.write(f"stage{j + 1}_{name}\t{getattr(ts, name)[j]}\n")
        f.write("#size\ttemplates\n")
        for b, count in enumerate(ts.size_hist):
            f.write(f"{b + 1 if b < 7 else '8+'}\t{count}\n")


class _Mode:
    """one mode of downsample_bam as its refusals name it: `name` ("disjoint replicates", plural), the options it does
    not go together with in the order they are reported -- one_sentence: the older modes name them all in one sentence
    --, and whether it takes amplicon files and a solver that grades by quality"""

    def __init__(self, name, refuses, plural=False, one_sentence=False, amplicon_files=False, quality_solver=False):
        self.name, self.refuses, self.plural, self.one_sentence = name, refuses, plural, one_sentence
        self.amplicon_files, self.quality_solver = amplicon_files, quality_solver


_THRESHOLDS = _Mode("coverage thresholds", ("a mean depth", "a proportion", "replicates", "a budget", "ceiling",
                                            "pair_aware", "template_aware", "targets", "a depth report", "a depth track",
                                            "a coverage ladder", "stratify", "dedup", "a coverage profile"),
                    plural=True)
_MEAN_DEPTH = _Mode("mean-depth downsampling", ("a proportion", "replicates", "a budget", "ceiling", "pair_aware",
                                                "template_aware", "targets", "a depth report", "a depth track",
                                                "a coverage ladder", "stratify", "dedup", "a coverage profile"))
_PROPORTIONAL = _Mode("proportional downsampling", ("replicates", "a budget", "ceiling", "pair_aware", "template_aware",
                                                    "targets", "a depth report", "a depth track", "a coverage ladder",
                                                    "stratify", "dedup", "a coverage profile"))
_REPLICATES = _Mode("disjoint replicates", ("a budget", "ceiling", "pair_aware", "template_aware", "targets", "a depth report",
                                            "a depth track", "a coverage ladder", "stratify", "dedup", "a coverage profile"),
                    plural=True)
_BUDGET = _Mode("budget downsampling", ("ceiling", "pair_aware", "template_aware", "targets", "a depth report",
                                        "a depth track", "a coverage ladder", "stratify", "dedup", "a coverage profile"))
_CEILING = _Mode("ceiling downsampling", ("pair_aware", "template_aware", "targets", "a depth report", "a depth track",
                                          "a coverage ladder", "stratify", "dedup"))
_TEMPLATES = _Mode("template-aware downsampling", ("pair_aware", "targets", "a depth report", "a depth track",
                                                   "a coverage ladder", "stratify", "dedup", "a coverage profile"))
_PAIRS = _Mode("pair-aware downsampling", ("targets", "a depth report", "a depth track", "a coverage ladder", "stratify",
                                           "dedup", "a coverage profile"))
_TRACK = _Mode("a depth track", ("a coverage ladder", "stratify", "dedup", "a coverage profile"), one_sentence=True,
               amplicon_files=True, quality_solver=True)
_PROFILE = _Mode("a coverage profile", ("targets", "a depth report", "a coverage ladder", "stratify", "dedup"),
                 one_sentence=True)
_DEDUP = _Mode("duplicate-aware downsampling", ("targets", "a depth report", "a coverage ladder", "stratify"),
               one_sentence=True)
_STRATIFIED = _Mode("stratified downsampling", ("targets", "a depth report", "a coverage ladder"), one_sentence=True)
_LADDER = _Mode("a coverage ladder", ("targets", "a depth report"), one_sentence=True, amplicon_files=True)
_START_CAP = _Mode("a start cap", ("coverage thresholds", "a mean depth", "a proportion", "replicates", "a budget", "ceiling",
                                   "pair_aware", "template_aware", "targets", "a depth report", "a depth track",
                                   "a coverage ladder", "stratify", "dedup", "a coverage profile"))
_AMPLICONS = _Mode("amplicon-aware downsampling", ("a start cap",) + _START_CAP.refuses, amplicon_files=True)
_TIERS = _Mode("tiered downsampling", ("amplicon-aware downsampling",) + _AMPLICONS.refuses)

_REGION_FIELDS = ("region_offsets", "region_starts", "region_ends", "region_caps")
_COUNT_FIELDS = {"ladder_levels": "n_ladder_levels", "pair_stages": "n_pair_stages", "template_stages": "n_template_stages",
                 "replicates_further": "n_replicates_further", "mapq_tiers": "n_mapq_tiers"}


def _downsample_request(**fields):
    """a DownsampleRequest from its fields by name (an unknown name is a KeyError): None is "not given"; a path or a
    name is anything str() renders; an array is a sequence of uint32, its count field filled in with it.  The fields
    whose "not given" is not zero start there: amplicon_mode -1, split_spliced 1, budget_fraction -1"""
    types = dict(DownsampleRequest._fields_)
    request = DownsampleRequest(struct_size=C.sizeof(DownsampleRequest), amplicon_mode=-1, split_spliced=1,
                                budget_fraction=-1.0)
    request.arrays = []  # (the request points into them)
    for name, value in fields.items():
        if value is None:
            continue
        if types[name] is C.c_char_p:
            value = str(value).encode()
        elif types[name] is _u32p:
            array = np.ascontiguousarray(value, dtype=np.uint32)
            request.arrays.append(array)
            if name in _COUNT_FIELDS:
                setattr(request, _COUNT_FIELDS[name], array.size)
            value = _p32(array)
        setattr(request, name, value)
    return request


def downsample_bam(solver_name, in_path, out_path, max_coverage, filtered_path=None, min_length=0, min_mapq=0,
                   per_reference=False, bed=None, tsv=None, amplicon_mode=None, amplicons_by_reference=False,
                   targets=None, target_padding=0, keep_off_target=False, report=None, report_bins=0, ladder=None,
                   ladder_out=None, stratify=None, strata_report=None, dedup=False, dedup_report=None, profile=None,
                   track=None, track_channel="kept", track_cap=0, pair_aware=False, pair_stages=None,
                   template_aware=False, split_spliced=True, include_secondary=False, template_stages=None,
                   template_report=None, template_targets=None, template_target_padding=0, template_profile=None,
                   ceiling=False, ceiling_report=None, budget_reads=None, budget_fraction=None, budget_report=None,
                   replicates=None, replicates_out=None, replicates_report=None, proportion=None, proportion_floor=0,
                   proportional_report=None, fragment_depth=False, fragment_report=None, mean_depth=None,
                   budget_bases=None, mean_depth_targets=None, mean_depth_report=None, thresholds=None,
                   thresholds_tag="XC", thresholds_report=None, start_cap=None, start_cap_by_strand=False,
                   start_cap_report=None, primer_clip=False, per_amplicon=False, amplicon_report=None, mapq_tiers=None,
                   tiers_report=None):
    """BamApi(in) -> solve -> find_pairs -> write_paired_reads(out): App::execute's file-to-file flow.
    per_reference=True: one coverage problem per reference of the file (BamApiConfig::per_reference).
    bed / tsv (amplicon_mode: 0 IGNORE, 1 FILTER, 2 GRADE; None: the solver decides, as App::execute does -- GRADE for
    "quasi-mcp-hip-quality", FILTER for "quasi-mcp-hip") need per_reference=True and amplicons_by_reference=True:
    the BED's chroms are matched to the file's references by name (ValueError otherwise).
    targets (a BED3+ file; BamApiConfig::targets_filepath, with target_padding and keep_off_target): coverage is capped
    inside the target regions only, reads that touch none are dropped (or all kept with keep_off_target=True); needs
    per_reference=True (ValueError otherwise), chroms matched to the references by name.  Amplicon files may be given as
    well: FILTER / GRADE act at ingest, the targets in the solve.
    report (a path; BamApiConfig::depth_report_filepath, with report_bins histogram bins): after the output has been
    written, the depth report (write_depth_report's TSV) of the reads the solve saw -- those that passed the ingest
    filters -- against the FINAL kept set (after mate completion), with max_coverage and, if given, the targets and
    their padding as regions; needs per_reference=True (ValueError otherwise).  None: nothing changes.
    ladder (a list of coverages strictly below max_coverage and strictly decreasing; BamApiConfig::coverage_ladder) with
    ladder_out (a path template holding "{M}"): a titration in one call.  The level at max_coverage goes to out_path as
    always; every further level is solved on the reads the level above kept, completed by find_pairs (monotone, so the
    files stay nested) and written to ladder_out with {M} replaced by its coverage.  Returns the list of written
    counts, out_path's first.  Needs per_reference=True; not together with targets, report or
    "quasi-mcp-hip-quality" (ValueError).  Amplicon FILTER at ingest works as before.  None: nothing changes.
    stratify ("strand" | "read_group"; BamApiConfig::stratify_by): one coverage cap per stratum in one
    qmcp_hip_solve_stratified_host call.  "read_group": every @RG of the header (and "*", the records without a listed
    RG) is brought to max_coverage on its own -- every sample to M x.  "strand": the forward reads are capped at
    ceil(max_coverage / 2), the reverse reads at floor(max_coverage / 2).  Every stratum keeps its own floor
    min(its coverage, its cap); a stratum with little data is not topped up from another.  find_pairs then completes
    mates as always -- it only adds reads, so every floor still holds; with "strand" the mates of a proper pair lie on
    the OTHER strand, so the per-strand totals of the written file exceed the caps.  strata_report (a path): after the
    output, a TSV with one line per stratum -- name, cap, reads, kept, mean depth before and after -- of the solve's
    kept set.  Needs per_reference=True; not together with targets, report, ladder, amplicon files or
    "quasi-mcp-hip-quality" (ValueError).  None: nothing changes.
    dedup=True (BamApiConfig::dedup): duplicate pairs -- equal unordered pair of (reference, start, end, strand) cells
    -- are collapsed to the pair of highest summed MAPQ (then the first in the file's pairing order) before the solve:
    one qmcp_hip_solve_dedup_host call in pair mode with mate completion.  Duplicates are simply not written;
    filtered_path keeps its meaning of ingest filters only.  dedup_report (a path): a TSV with the statistics, then one
    size<TAB>families line per family-size bin (DEDUP_REPORT_BINS bins, the last holding the larger sizes).  Needs
    per_reference=True; not together with targets, report, ladder, stratify, amplicon files or
    "quasi-mcp-hip-quality" (ValueError).  False: nothing changes.
    profile (a bedGraph file: chrom start end cap; profile_from_bedgraph): a cap that varies along the genome, with
    max_coverage as the cap outside the file's regions -- one qmcp_hip_solve_profile_host call.  Chroms are matched to
    the file's references by name, overlapping lines are flattened with the later line winning.  Needs
    per_reference=True; not together with targets, report, ladder, stratify, dedup, amplicon files or
    "quasi-mcp-hip-quality" (ValueError).  None: nothing changes.
    track (a path; BamApiConfig::depth_track_filepath, with track_channel "kept" | "in" | "both" and track_cap, a clamp
    on the written depths, 0: none): after the output has been written, the per-base depth (write_bedgraph's bedGraph;
    Solver.depth_track with both channels) of the reads the solve saw against the FINAL kept set (after mate
    completion), inside the targets with their padding when given.  Needs per_reference=True; goes together with
    targets, report and amplicon files as report does; not together with ladder, stratify, dedup or profile
    (ValueError).  None: nothing changes.
    pair_aware=True (BamApiConfig::pair_aware, with pair_stages: rising targets that end at max_coverage; None:
    ceil(max_coverage / 2), then max_coverage): one qmcp_hip_solve_pairs_host call -- the solve runs in stages that
    credit the coverage of the mates already kept, so the output stays near max_coverage instead of near twice that.
    The output is written from the final mask, which holds whole pairs: no find_pairs follows.  Needs
    per_reference=True; not together with targets, report, track, ladder, stratify, dedup, profile, amplicon files or
    "quasi-mcp-hip-quality" (ValueError).  False: nothing changes.
    template_aware=True (BamApiConfig::template_aware, with split_spliced and include_secondary as in
    read_bam(templates=True), and template_stages as pair_stages): one qmcp_hip_solve_templates_host call on the file's
    segments -- single-end reads, pairs, split reads with their supplementary alignments and spliced reads are kept or
    dropped as whole templates, and an intron gets no depth.  A record is written if and only if its template is kept;
    no find_pairs follows.  template_report (a path): a TSV with the statistics, then one size<TAB>templates line per
    bin of the template-size histogram (1 .. 7 and 8+).  Needs per_reference=True; not together with pair_aware or
    anything pair_aware refuses (ValueError).  False: nothing changes.
    template_targets (a BED3+ file, with template_target_padding) or template_profile (a bedGraph file), with
    template_aware=True and per_reference=True: whole templates under a cap per region -- one
    qmcp_hip_solve_templates_profile_host call.  template_targets: the cap is max_coverage inside the targets (padded,
    clipped and merged by targets_as_regions) and 0 outside, so reads off target come out only as part of a template that
    is kept for its depth on target.  template_profile: the caps of profile_from_bedgraph, max_coverage elsewhere.
    max_coverage is the scale of template_stages in both.  template_report then also lists segments_on_cap,
    templates_on_cap, regions_in, regions_used and positions_in_regions.  Not both at once, and not with anything
    template_aware refuses -- targets= and profile= included (ValueError).  None: nothing changes.
    fragment_depth=True (BamApiConfig::fragment_depth, with template_aware=True): a template counts ONCE where its
    segments overlap -- the two mates of a short-insert pair -- as in mosdepth, samtools depth -s and GATK: the solve is
    one qmcp_hip_solve_fragments_host call, or with template_targets / template_profile qmcp_hip_clip_templates_host
    followed by the cap-table entry on the clipped columns.  fragment_report (a path) gets a stat<TAB>value TSV with the
    FragmentStats (segments_placed, segments_clipped, segments_emptied, bases_in, bases_removed, templates_overlapping,
    max_group, ms_clip) and records_written.  Either without template_aware=True is a ValueError, and so is
    fragment_report without fragment_depth=True.  False: nothing changes.
    ceiling=True (BamApiConfig::ceiling): max_coverage is a CEILING -- the written depth is at most max_coverage at every
    position and as many reads as possible are kept -- one qmcp_hip_solve_ceiling_host call with CEILING_WHOLE_PAIRS on
    the reads as the pair-aware flow pairs them.  With profile (a bedGraph file) the file's caps are ceilings and
    max_coverage applies elsewhere.  The output is written from the final mask, which holds whole pairs: no find_pairs
    follows (it would put depth back).  The depth may fall below min(coverage, cap) next to deeper positions;
    ceiling_report (a path) gets a stat<TAB>value TSV with the CeilingStats (short_positions, short_bases, ...) and
    records_written.  Needs per_reference=True; not together with targets, report, track, ladder, stratify, dedup,
    pair_aware, template_aware, amplicon files or "quasi-mcp-hip-quality" (ValueError).  False: nothing changes.
    budget_reads=N or budget_fraction=f (BamApiConfig::budget_reads / budget_fraction): the deepest downsample that
    writes at most N records -- or at most floor(f * placed reads), f in 0 .. 1, the placed reads being those that
    passed the ingest filters.  max_coverage is the upper end of the search; one qmcp_hip_solve_budget_host call with
    BUDGET_WHOLE_PAIRS on the reads as the ceiling and pair-aware flows pair them finds the largest coverage whose solve,
    completed to whole pairs, fits.  The output is written from the final mask and no find_pairs follows (it would add
    reads): records written <= budget.  budget_report (a path) gets a stat<TAB>value TSV with the BudgetStats and
    records_written, then one M<TAB>bases line per entry of the curve S(M).  Needs per_reference=True; exactly one of
    the two budgets; not together with targets, report, track, ladder, stratify, dedup, profile, pair_aware,
    template_aware, ceiling, amplicon files or "quasi-mcp-hip-quality" (ValueError).  None: nothing changes.
    replicates=K or [c_2, .., c_K] (BamApiConfig::replicates) with replicates_out (a path template holding "{R}"): the
    file split into K disjoint downsamples in one qmcp_hip_solve_replicates_host call with REPLICATES_WHOLE_PAIRS |
    REPLICATES_SHORTFALL on the reads as the ceiling and pair-aware flows pair them.  An int K: K replicates at
    max_coverage; a list: replicate 1 at max_coverage, then the list's coverages.  Replicate 1 goes to out_path,
    replicate R to replicates_out with {R} replaced.  Every file is written from its label and no find_pairs follows (it
    would copy a record into two files): every input record is written at most once over all files.  Returns the list
    of written counts.  replicates_report (a path) gets a TSV with one line per replicate -- coverage, offered, kept,
    mates, short_positions, short_bases, records_written -- and an n_full line.  Replicates are disjoint, not
    exchangeable: replicate 1 gets the first choices.  Needs per_reference=True; not together with targets, report,
    track, ladder, stratify, dedup, profile, pair_aware, template_aware, ceiling, a budget, amplicon files or
    "quasi-mcp-hip-quality" (ValueError).  None: nothing changes.
    proportion=f (a float, a fractions.Fraction or a (num, den) pair: as_ratio; BamApiConfig::proportion) with
    proportion_floor: every position keeps at least ceil(f * its depth), positions at or below proportion_floor are
    kept whole, and max_coverage is a hard upper end of the demand (2**31 - 1: none) -- one
    qmcp_hip_solve_proportional_host call.  find_pairs then completes mates as always: it only adds reads, so every
    floor still holds.  proportional_report (a path) gets a stat<TAB>value TSV with the ProportionalStats and
    records_written.  Needs per_reference=True; not together with replicates, a budget, ceiling, pair_aware,
    template_aware, targets, report, track, ladder, stratify, dedup, profile, amplicon files or
    "quasi-mcp-hip-quality" (ValueError).  None: nothing changes.
    mean_depth=d or budget_bases=N (BamApiConfig::mean_depth / budget_bases) with mean_depth_targets (a BED3+ file; None:
    every position of every reference): the deepest downsample whose written records hold at most N bases inside the
    regions -- or at most floor(d * the regions' positions), the regions clipped to their references and merged: "make
    this file 30 x", "bring the exome to 100 x mean on target".  max_coverage is the upper end of the search; one
    qmcp_hip_solve_mean_depth_host call with MEAN_DEPTH_WHOLE_PAIRS on the reads as the budget flow pairs them.  The
    output is written from the final mask and no find_pairs follows (it would add bases).  mean_depth_report (a path)
    gets a stat<TAB>value TSV with the MeanDepthStats, records_written and the two means mean_depth_in and
    mean_depth_kept over the regions' positions, then one M<TAB>bases line per entry of the curve S_R(M).  Needs
    per_reference=True; exactly one of mean_depth and budget_bases; not together with a proportion, replicates, a
    budget, ceiling, pair_aware, template_aware, targets, report, track, ladder, stratify, dedup, profile, amplicon
    files or "quasi-mcp-hip-quality" (ValueError).  None: nothing changes.
    thresholds=hi or (lo, hi) (BamApiConfig::thresholds_lo / thresholds_hi, lo = 1 when only hi is given) with
    thresholds_tag (two characters, [A-Za-z][A-Za-z0-9]): tag the file once, cut any downsample later with a filter.  One
    ingest and one qmcp_hip_solve_thresholds_host call with THRESHOLDS_WHOLE_PAIRS on the reads as the budget flow pairs
    them; every record whose threshold is <= hi is written with the aux field <tag>:S:<threshold> -- the smallest
    coverage of lo .. hi at which the by-contig solve, completed to whole pairs, keeps it -- and no find_pairs follows.
    `samtools view -e '[XC]<=30'` of the output is then the downsample at 30 (while the report's nesting_violations is
    0: it has been on every input seen, which is not proven).  max_coverage is not used.  An input record that carries
    the tag already is refused before anything is written.  thresholds_report (a path) gets a stat<TAB>value TSV with
    the ThresholdsStats and records_written, then one M<TAB>reads line per coverage of the range.  Needs
    per_reference=True; not together with a mean depth, a proportion, replicates, a budget, ceiling, pair_aware,
    template_aware, targets, report, track, ladder, stratify, dedup, profile, amplicon files or "quasi-mcp-hip-quality"
    (ValueError).  None: nothing changes.
    start_cap=K (BamApiConfig::start_cap, with start_cap_by_strand): every alignment start -- (reference, start), with
    start_cap_by_strand=True (reference, start, strand) -- offers the solve at most K reads: those of highest MAPQ, then
    the longest, then the first in the file's pairing order.  One qmcp_hip_solve_start_cap_host call with
    START_CAP_SHORTFALL on the reads that passed the ingest filters, then find_pairs and the write exactly as the plain
    flow.  Mate completion only adds reads: every floor the solve reached still holds, but a written start may exceed K
    through a mate -- the cap is on what the solve may choose from, as GATK's --max-reads-per-alignment-start is.
    start_cap_report (a path) gets a stat<TAB>value TSV with the StartCapStats (cells_kept, short_positions, ...) and
    records_written, then one size<TAB>cells line per cell-size bin (START_CAP_REPORT_BINS bins, the last holding the
    larger sizes).  Needs per_reference=True; not together with any other mode -- thresholds, a mean depth, a
    proportion, replicates, a budget, ceiling, pair_aware, template_aware, targets, report, track, ladder, stratify,
    dedup, profile --, amplicon files or "quasi-mcp-hip-quality" (ValueError); start_cap_by_strand or start_cap_report
    without start_cap is a ValueError too.  None: nothing changes.
    primer_clip / per_amplicon / amplicon_report (BamApiConfig::primer_clip, per_amplicon, amplicon_report_filepath):
    amplicon-aware downsampling in one qmcp_hip_solve_amplicons_host call on the pairs that passed the ingest (its
    FILTER included).  primer_clip=True counts depth on the reads clipped to their amplicon's insert -- from BED primers
    [ls, le) and [rs, re) the amplicon stays [ls, re], the insert is [le, rs - 1]; a pair that leaves no insert is a
    ValueError naming it -- so "M x" of output is M x after primer trimming.  per_amplicon=True solves every amplicon as
    a coverage problem of its own (ARTIC's --normalise): it keeps more reads, and where inserts overlap the kept depth
    reaches up to about twice M and more.  Clipping decides what COUNTS as depth, not what is written: the output holds
    the original, unclipped records of the kept reads, completed by find_pairs as always.  amplicon_report (a path) gets
    one line per amplicon (write_amplicon_report's TSV); alone it runs the entry with clipping off and pooled, which
    selects what the plain flow selects.  They need bed, per_reference=True, amplicons_by_reference=True and
    "quasi-mcp-hip"; not together with any other mode -- a start cap, thresholds, a mean depth, a proportion,
    replicates, a budget, ceiling, pair_aware, template_aware, targets, report, track, ladder, stratify, dedup, profile
    (ValueError).  False / None: nothing changes
    mapq_tiers / tiers_report (BamApiConfig::mapq_tiers): tiered downsampling by MAPQ band in one
    qmcp_hip_solve_tiers_host call on the reads that passed the ingest filters -- strictly falling thresholds, e.g.
    [30, 10, 0]: the reads of MAPQ >= 30 are solved first, those of 10 .. 29 only fill what they leave short of
    min(coverage, max_coverage), those below 10 only what both leave short; then find_pairs and the write, as in the plain
    flow (completion only adds reads, so the floor holds).  The last threshold must equal min_mapq, so that every read
    the ingest lets through has a tier; at most TIERS_MAX thresholds.  tiers_report (a path) gets one line per tier --
    band, reads, kept, mean depth before and after, demand, asked positions --, then records_written and mates_added
    (the records completion added); without mapq_tiers it is a ValueError.  Needs per_reference=True and
    "quasi-mcp-hip"; not together with any other mode -- amplicon-aware downsampling, a start cap, thresholds, a mean
    depth, a proportion, replicates, a budget, ceiling, pair_aware, template_aware, targets, report, track, ladder,
    stratify, dedup, profile --, nor with amplicon files (ValueError).  None: nothing changes"""
    _need_host()
    given = {"amplicon-aware downsampling": bool(primer_clip or per_amplicon or amplicon_report is not None),
             "a start cap": start_cap is not None, "coverage thresholds": thresholds is not None,
             "a mean depth": mean_depth is not None or budget_bases is not None, "a proportion": proportion is not None, "replicates": replicates is not None,
             "a budget": budget_reads is not None or budget_fraction is not None, "ceiling": bool(ceiling),
             "pair_aware": bool(pair_aware), "template_aware": bool(template_aware), "targets": bool(targets),
             "a depth report": bool(report), "a depth track": track is not None, "a coverage ladder": ladder is not None,
             "stratify": stratify is not None, "dedup": bool(dedup), "a coverage profile": profile is not None}
    amplicon_files = bool(bed or tsv or amplicons_by_reference)

    def need_per_reference(mode):
        if not per_reference:
            raise ValueError(f"{mode.name} {'need' if mode.plural else 'needs'} per_reference=True")

    def refuse(mode):
        does_not = f"{mode.name} {'do' if mode.plural else 'does'} not"
        offences = [what for what in mode.refuses if given[what]]
        if offences and mode.one_sentence:
            raise ValueError(f"{does_not} go together with {', '.join(mode.refuses[:-1])} or {mode.refuses[-1]}")
        if offences:
            raise ValueError(f"{does_not} go together with {offences[0]}")
        if amplicon_files and not mode.amplicon_files:
            raise ValueError(f"{does_not} take amplicon files")
        if not mode.quality_solver and solver_uses_quality(solver_name):
            raise ValueError(f"{does_not} take a solver that grades by quality")

    def stages_of(stages, name):
        stages = None if stages is None else [int(t) for t in stages]
        if stages is not None and not stages:
            raise ValueError(f"{name} must hold at least one target (or be None for the default schedule)")
        return stages

    def solve_fields():
        """what Solver::solve's own flow takes, with or without a depth track or a ladder: amplicons, targets, a report"""
        if (bed or tsv) and not (per_reference and amplicons_by_reference):
            raise ValueError("amplicon files (bed / tsv) need per_reference=True and amplicons_by_reference=True")
        if report and not per_reference:
            raise ValueError("a depth report needs per_reference=True")
        if targets and not per_reference:
            raise ValueError("targets need per_reference=True")
        return dict(bed=bed or None, tsv=tsv or None, amplicon_mode=None if amplicon_mode is None else int(amplicon_mode),
                    amplicons_by_reference=bool(amplicons_by_reference), targets=targets or None,
                    target_padding=int(target_padding), keep_off_target=bool(keep_off_target), report=report or None,
                    report_bins=int(report_bins))

    # the request, by field name; what a mode does not name stays "not given"
    fields = dict(solver_name=solver_name, in_path=in_path, out_path=out_path, filtered_path=filtered_path or None,
                  max_coverage=int(max_coverage), min_len=int(min_length), min_mapq=int(min_mapq),
                  per_reference=bool(per_reference))
    n_files = None  # a ladder and replicates write several files and return a list
    if (fragment_depth or fragment_report is not None) and not template_aware:
        raise ValueError("fragment_depth and fragment_report need template_aware=True")
    if fragment_report is not None and not fragment_depth:
        raise ValueError("fragment_report needs fragment_depth=True")
    if (proportion_floor or proportional_report is not None) and proportion is None:
        raise ValueError("proportion_floor and proportional_report need proportion")
    if (mean_depth_targets is not None or mean_depth_report is not None) and mean_depth is None and budget_bases is None:
        raise ValueError("mean_depth_targets and mean_depth_report need mean_depth or budget_bases")
    if thresholds is None and thresholds_report is not None:
        raise ValueError("thresholds_report needs thresholds")
    if start_cap is None and (start_cap_by_strand or start_cap_report is not None):
        raise ValueError("start_cap_by_strand and start_cap_report need start_cap")
    if tiers_report is not None and mapq_tiers is None:
        raise ValueError("tiers_report needs mapq_tiers")
    if mapq_tiers is not None:
        bands = [int(x) for x in mapq_tiers]
        tiers_from_mapq([], bands)  # (ValueError: empty, negative, not strictly falling, more than TIERS_MAX)
        if bands[-1] != int(min_mapq):
            raise ValueError(f"the last threshold of mapq_tiers ({bands[-1]}) must equal min_mapq ({int(min_mapq)}): every "
                             "read the ingest lets through needs a tier")
        need_per_reference(_TIERS)
        refuse(_TIERS)
        fields.update(mapq_tiers=bands, tiers_report=tiers_report)
    elif primer_clip or per_amplicon or amplicon_report is not None:
        if not (bed and per_reference and amplicons_by_reference):
            raise ValueError("primer_clip, per_amplicon and amplicon_report need bed, per_reference=True and "
                             "amplicons_by_reference=True")
        refuse(_AMPLICONS)
        fields.update(bed=bed, tsv=tsv or None, amplicon_mode=None if amplicon_mode is None else int(amplicon_mode),
                      amplicons_by_reference=True, primer_clip=bool(primer_clip), per_amplicon=bool(per_amplicon),
                      amplicon_report=amplicon_report)
    elif start_cap is not None:
        if not 1 <= int(start_cap) < 1 << 32:
            raise ValueError("start_cap must lie in 1 .. 2^32 - 1")
        need_per_reference(_START_CAP)
        refuse(_START_CAP)
        fields.update(start_cap=int(start_cap), start_cap_by_strand=bool(start_cap_by_strand),
                      start_cap_report=start_cap_report)
    elif thresholds is not None:
        lo, hi = (1, thresholds) if np.isscalar(thresholds) else thresholds
        lo, hi = int(lo), int(hi)
        if not 1 <= lo <= hi <= THRESHOLDS_COVERAGE_MAX:
            raise ValueError(f"thresholds need 1 <= lo <= hi <= {THRESHOLDS_COVERAGE_MAX}")
        tag = str(thresholds_tag)
        if not (len(tag) == 2 and tag.isascii() and tag[0].isalpha() and tag[1].isalnum()):
            raise ValueError("thresholds_tag must be [A-Za-z][A-Za-z0-9]")
        need_per_reference(_THRESHOLDS)
        refuse(_THRESHOLDS)
        fields.update(has_thresholds=1, thresholds_lo=lo, thresholds_hi=hi, thresholds_tag=str(thresholds_tag),
                      thresholds_report=thresholds_report)
    elif mean_depth is not None or budget_bases is not None:
        if mean_depth is not None and budget_bases is not None:
            raise ValueError("mean-depth downsampling takes mean_depth or budget_bases, not both")
        if budget_bases is not None and not 0 <= int(budget_bases) < 1 << 64:
            raise ValueError("budget_bases must fit an unsigned 64-bit count")
        if mean_depth is not None and not (float(mean_depth) >= 0.0 and math.isfinite(float(mean_depth))):
            raise ValueError("mean_depth must be a finite depth of at least 0")
        need_per_reference(_MEAN_DEPTH)
        refuse(_MEAN_DEPTH)
        fields.update(has_mean_depth=mean_depth is not None, mean_depth=float(mean_depth or 0.0),
                      has_budget_bases=budget_bases is not None, budget_bases=int(budget_bases or 0),
                      mean_depth_targets=mean_depth_targets, mean_depth_report=mean_depth_report)
    elif proportion is not None:
        num, den = as_ratio(proportion)
        if den > PROPORTION_DEN_MAX:
            raise ValueError(f"proportion: the denominator must not exceed {PROPORTION_DEN_MAX}")
        if not 0 <= int(proportion_floor) < 1 << 32:
            raise ValueError("proportion_floor must fit an unsigned 32-bit depth")
        if not 0 <= int(max_coverage) < 1 << 31:
            raise ValueError("proportional downsampling: max_coverage must lie in 0 .. 2^31 - 1")
        need_per_reference(_PROPORTIONAL)
        refuse(_PROPORTIONAL)
        fields.update(has_proportion=1, proportion_num=num, proportion_den=den, proportion_floor=int(proportion_floor),
                      proportional_report=proportional_report)
    elif (replicates_out is not None or replicates_report is not None) and replicates is None:
        raise ValueError("replicates_out and replicates_report need replicates")
    elif replicates is not None:
        if isinstance(replicates, (int, np.integer)):
            if not 1 <= int(replicates) <= REPLICATES_MAX:
                raise ValueError(f"replicates must lie in 1 .. {REPLICATES_MAX}")
            further = [int(max_coverage)] * (int(replicates) - 1)
        else:
            further = [int(c) for c in replicates]
            if len(further) + 1 > REPLICATES_MAX:
                raise ValueError(f"replicates: at most {REPLICATES_MAX} replicates in one call")
        if any(not 1 <= c < 1 << 31 for c in further + [int(max_coverage)]):
            raise ValueError("replicates: every coverage must lie in 1 .. 2^31 - 1")
        need_per_reference(_REPLICATES)
        if further and (replicates_out is None or "{R}" not in str(replicates_out)):
            raise ValueError("replicates_out must be a path template holding {R}")
        refuse(_REPLICATES)
        n_files = len(further) + 1
        fields.update(has_replicates=1, replicates_further=further or None, replicates_template=replicates_out,
                      replicates_report=replicates_report)
    elif budget_report is not None and (budget_reads is None) == (budget_fraction is None):
        raise ValueError("budget_report needs exactly one of budget_reads and budget_fraction")
    elif given["a budget"]:
        if budget_reads is not None and budget_fraction is not None:
            raise ValueError("budget downsampling takes budget_reads or budget_fraction, not both")
        if budget_reads is not None and not 0 <= int(budget_reads) < 1 << 64:
            raise ValueError("budget_reads must fit an unsigned 64-bit count")
        if budget_fraction is not None and not 0.0 <= float(budget_fraction) <= 1.0:
            raise ValueError("budget_fraction must lie in 0 .. 1")
        need_per_reference(_BUDGET)
        refuse(_BUDGET)
        fields.update(has_budget_reads=budget_reads is not None, budget_reads=int(budget_reads or 0),
                      budget_fraction=None if budget_fraction is None else float(budget_fraction),
                      budget_report=budget_report)
    elif ceiling_report is not None and not ceiling:
        raise ValueError("ceiling_report needs ceiling=True")
    elif ceiling:
        need_per_reference(_CEILING)
        refuse(_CEILING)
        fields.update(ceiling=1, ceiling_report=ceiling_report)
        if profile is not None:
            names = reference_names(in_path)
            fields.update(zip(_REGION_FIELDS, profile_from_bedgraph(profile, names)), has_regions=1, n_refs=len(names))
    elif (template_targets is not None or template_profile is not None) and not (template_aware and per_reference):
        raise ValueError("template_targets and template_profile need template_aware=True and per_reference=True")
    elif template_targets is not None and template_profile is not None:
        raise ValueError("template_targets and template_profile do not go together: give one table")
    elif template_target_padding and template_targets is None:
        raise ValueError("template_target_padding needs template_targets")
    elif template_aware:
        need_per_reference(_TEMPLATES)
        refuse(_TEMPLATES)
        fields.update(template_aware=1, split_spliced=bool(split_spliced), include_secondary=bool(include_secondary),
                      template_stages=stages_of(template_stages, "template_stages"),
                      fragment_depth=bool(fragment_depth), fragment_report=fragment_report)
        if template_targets is not None or template_profile is not None:
            if int(template_target_padding) < 0:
                raise ValueError("template_target_padding must not be negative")
            names, ref_lengths = _reference_table(in_path)
            if template_targets is not None:
                table = targets_as_regions(*targets_from_bed(template_targets, names), ref_lengths,
                                           int(template_target_padding), int(max_coverage))
            else:
                table = profile_from_bedgraph(template_profile, names)
            fields.update(zip(_REGION_FIELDS, table), has_regions=1, n_refs=len(names),
                          default_cap=0 if template_targets is not None else int(max_coverage))
    elif template_stages is not None or template_report is not None or not split_spliced or include_secondary:
        raise ValueError("template_stages, template_report, split_spliced and include_secondary need template_aware=True")
    elif pair_aware:
        need_per_reference(_PAIRS)
        refuse(_PAIRS)
        fields.update(pair_aware=1, pair_stages=stages_of(pair_stages, "pair_stages"))
    elif pair_stages is not None:
        raise ValueError("pair_stages need pair_aware=True")
    elif track is not None:
        need_per_reference(_TRACK)
        if track_channel not in ("kept", "in", "both"):
            raise ValueError(f'track_channel must be "kept", "in" or "both", not {track_channel!r}')
        refuse(_TRACK)
        fields.update(solve_fields(), track=track, track_channel=track_channel, track_cap=int(track_cap))
    elif profile is not None:
        need_per_reference(_PROFILE)
        refuse(_PROFILE)
        names = reference_names(in_path)
        fields.update(zip(_REGION_FIELDS, profile_from_bedgraph(profile, names)), has_regions=1, n_refs=len(names))
    elif dedup:
        need_per_reference(_DEDUP)
        refuse(_DEDUP)
        fields.update(dedup=1, dedup_report=dedup_report)
    elif dedup_report is not None:
        raise ValueError("dedup_report needs dedup")
    elif stratify is not None:
        if stratify not in ("strand", "read_group"):
            raise ValueError(f'stratify must be "strand" or "read_group", not {stratify!r}')
        need_per_reference(_STRATIFIED)
        refuse(_STRATIFIED)
        fields.update(stratify=stratify, strata_report=strata_report)
    elif strata_report is not None:
        raise ValueError("strata_report needs stratify")
    elif ladder is not None:
        levels = [int(m) for m in ladder]
        need_per_reference(_LADDER)
        if ladder_out is None or "{M}" not in str(ladder_out):
            raise ValueError("ladder_out must be a path template holding {M}")
        refuse(_LADDER)
        if not levels or levels[0] >= int(max_coverage):
            raise ValueError("the levels of a coverage ladder must be strictly below max_coverage")
        if any(b >= a for a, b in zip(levels, levels[1:])) or levels[-1] < 1:
            raise ValueError("the levels of a coverage ladder must be strictly decreasing and >= 1")
        n_files = len(levels) + 1
        fields.update(solve_fields(), ladder_levels=levels, ladder_template=ladder_out)
    else:
        fields.update(solve_fields())

    counts = (C.c_int64 * (n_files or 1))()
    ts, qs = TemplateStats(), TemplateProfileStats()  # (the other modes' stats are in their reports)
    err = C.create_string_buffer(1024)
    n = _host.qmcp_host_downsample_bam(C.byref(_downsample_request(**fields)), counts, len(counts), None, None, None,
                                       C.byref(ts), C.byref(qs), err, 1024)
    if n == -4:
        raise ValueError(err.value.decode())
    if n == -1:
        raise KeyError(solver_name)
    if n < 0:
        message = err.value.decode(errors="replace")
        raise OSError(f"downsample_bam({in_path}) failed ({n})" + (f": {message}" if message else ""))
    if template_aware and template_report is not None:
        write_template_report(template_report, ts, int(n), qs if fields.get("has_regions") else None)
    return int(n) if n_files is None else [int(c) for c in counts[:n]]
