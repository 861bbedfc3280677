"""The depth report (qmcp_hip_depth_report_*), restated for the tests in numpy from its contract: a difference array per
contig, cumsum, rows by slicing, histograms by np.bincount with clipping.  Merged regions come from
target_model.merged_regions (boolean target sets), independent of target_table.h.
  coverages   per contig, (cov, kept): placed reads covering each position, and those of them whose mask bit is set
  row         one row over [a, b] of a contig, as a tuple in the field order of qmcp_hip_depth_row
  report      the whole call -> dict(contig_rows, region_rows, hist_in, hist_kept, stats)"""
import numpy as np

import target_model as tm

NO_CONTIG = 0xFFFFFFFF
FIELDS = ("contig", "start", "end", "min_in", "max_in", "min_kept", "max_kept", "reserved", "positions", "sum_in",
          "sum_kept", "capped_positions", "deficit_positions", "deficit_sum")


def kept_bits(keep_mask, n):
    if keep_mask is None:
        return np.ones(n, bool)
    bits = np.unpackbits(np.ascontiguousarray(keep_mask, np.uint64).view(np.uint8), bitorder="little")
    return bits[:n].astype(bool)


def coverages(starts, ends, contig_ids, contig_lengths, keep_mask=None):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    kept = kept_bits(keep_mask, s.size)
    out = []
    for c, L in enumerate(np.atleast_1d(np.asarray(contig_lengths, np.int64)).tolist()):
        pair = []
        for sel in (np.flatnonzero(ids == c), np.flatnonzero((ids == c) & kept)):
            diff = np.zeros(L + 1, np.int64)
            np.add.at(diff, s[sel], 1)
            np.add.at(diff, e[sel] + 1, -1)
            pair.append(np.cumsum(diff)[:L])
        out.append(tuple(pair))
    return out


def row(contig, a, b, cov, kept, M):
    if b < a:
        return (contig,) + (0,) * 13
    ci, ck = cov[a:b + 1], kept[a:b + 1]
    need = np.minimum(ci, M)
    short = np.maximum(need - ck, 0)
    return (contig, a, b, int(ci.min()), int(ci.max()), int(ck.min()), int(ck.max()), 0, b - a + 1, int(ci.sum()),
            int(ck.sum()), int((ci > M).sum()), int((short > 0).sum()), int(short.sum()))


def report(starts, ends, contig_ids, contig_lengths, M, keep_mask=None, target_offsets=None, target_starts=None,
           target_ends=None, padding=0, n_bins=0):
    lengths = np.atleast_1d(np.asarray(contig_lengths, np.int64))
    ids = np.asarray(contig_ids, np.int64)
    covs = coverages(starts, ends, ids, lengths, keep_mask)
    contig_rows = [row(c, 0, int(L) - 1, covs[c][0], covs[c][1], M) for c, L in enumerate(lengths.tolist())]
    region_rows, scope_in, scope_kept = [], [], []
    regions_in = 0
    if target_offsets is not None:
        regions_in = int(np.asarray(target_offsets)[-1])
        sets = tm.target_sets(lengths, target_offsets, target_starts if regions_in else [], target_ends if regions_in else [],
                              padding)
        for c, tset in enumerate(sets):
            for a, b, _ in tm.merged_regions(tset):
                region_rows.append(row(c, a, b, covs[c][0], covs[c][1], M))
            scope_in.append(covs[c][0][tset])
            scope_kept.append(covs[c][1][tset])
        scope_rows = region_rows
    else:
        scope_in = [cv[0] for cv in covs]
        scope_kept = [cv[1] for cv in covs]
        scope_rows = contig_rows
    scope_in = np.concatenate(scope_in) if scope_in else np.zeros(0, np.int64)
    scope_kept = np.concatenate(scope_kept) if scope_kept else np.zeros(0, np.int64)
    hist = lambda d: np.bincount(np.minimum(d, n_bins - 1), minlength=n_bins).astype(np.uint64) if n_bins \
        else np.zeros(0, np.uint64)
    placed = ids != NO_CONTIG
    stats = dict(reads_placed=int(placed.sum()), reads_kept=int((placed & kept_bits(keep_mask, ids.size)).sum()),
                 scope_positions=int(scope_in.size), deficit_positions=sum(r[12] for r in scope_rows),
                 regions_in=regions_in, regions_merged=len(region_rows))
    return dict(contig_rows=contig_rows, region_rows=region_rows, hist_in=hist(scope_in), hist_kept=hist(scope_kept),
                stats=stats)


def assert_equal(got, want, info=""):
    """a package DepthReport against report()'s dict, bit for bit"""
    assert [tuple(int(x) for x in r) for r in got.contig_rows.tolist()] == want["contig_rows"], info
    assert [tuple(int(x) for x in r) for r in got.region_rows.tolist()] == want["region_rows"], info
    assert np.array_equal(got.hist_in, want["hist_in"]) and np.array_equal(got.hist_kept, want["hist_kept"]), info
    for k, v in want["stats"].items():
        assert getattr(got.stats, k) == v, (info, k, getattr(got.stats, k), v)
    assert got.valid == (want["stats"]["deficit_positions"] == 0), info
