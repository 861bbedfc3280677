"""The depth track (qmcp_hip_depth_track_*), restated for the tests in numpy from its contract, twice.
  track            from EVENTS: per contig the change points (read starts, ends + 1, the bounds of the scope intervals) are
                   sorted and swept, so the cost follows the reads and not the positions -- two contigs of 1.2 x 10^9
                   positions take milliseconds.  Merged regions come from merge_regions below (pad, clip, sort, join
                   overlapping and adjacent), written here from the contract's words
  track_positions  per POSITION: depth_model.coverages and target_model.target_sets (boolean target sets), a Python loop
                   over every position; only for small inputs, to check the first form
Both return (runs, stats): runs a list of (contig, start, end, depth_in, depth_kept, short) in ascending (contig, start)
order, stats a dict of the fields of qmcp_hip_track_stats that the contract fixes (no position_batches, no time)."""
import numpy as np

import depth_model as dm
import target_model as tm

NO_CONTIG = 0xFFFFFFFF
IN, KEPT, SHORT_ONLY, SKIP_ZERO = 1, 2, 4, 8
FIELDS = ("contig", "start", "end", "depth_in", "depth_kept", "flags")


def merge_regions(length, starts, ends, padding):
    """the merged regions of one contig: [(lo, hi)], inclusive, ascending, at least one position apart"""
    regs = []
    for a, b in zip(np.asarray(starts, np.int64).tolist(), np.asarray(ends, np.int64).tolist()):
        a, b = max(a - padding, 0), min(b + padding, length - 1)
        if a < length and a <= b:
            regs.append((a, b))
    out = []
    for a, b in sorted(regs):
        if out and a <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]


def _scope(lengths, target_offsets, target_starts, target_ends, padding):
    """per contig the scope intervals, and (regions_in, regions_merged)"""
    if target_offsets is None:
        return [[(0, L - 1)] if L else [] for L in lengths.tolist()], 0, 0
    offs = np.asarray(target_offsets, np.int64)
    t0, t1 = np.asarray(target_starts, np.int64), np.asarray(target_ends, np.int64)
    scope = [merge_regions(L, t0[offs[c]:offs[c + 1]], t1[offs[c]:offs[c + 1]], padding) if offs[c + 1] > offs[c] else []
             for c, L in enumerate(lengths.tolist())]
    return scope, int(offs[-1]), sum(len(s) for s in scope)


def _tuples(cov, kept, M, flags, depth_cap):
    """vectorised: (depth_in, depth_kept, short, emitted-if-in-scope)"""
    cap = depth_cap if depth_cap else 1 << 62
    din = np.minimum(cov, cap) if flags & IN else np.zeros_like(cov)
    dk = np.minimum(kept, cap) if flags & KEPT else np.zeros_like(kept)
    short = kept < np.minimum(cov, M)
    em = np.ones(cov.shape, bool)
    if flags & SHORT_ONLY:
        em &= short
    if flags & SKIP_ZERO:
        em &= (din | dk) != 0
    return din, dk, short, em


def _stats(ids, keep_mask, runs, emitted, scope_positions, short_positions, regions_in, regions_merged):
    placed = ids != NO_CONTIG
    return dict(n_runs=len(runs), positions_in_runs=int(emitted), scope_positions=int(scope_positions),
                short_positions=int(short_positions), reads_placed=int(placed.sum()),
                reads_kept=int((placed & dm.kept_bits(keep_mask, ids.size)).sum()), regions_in=regions_in,
                regions_merged=regions_merged)


def track(starts, ends, contig_ids, contig_lengths, M, keep_mask=None, target_offsets=None, target_starts=None,
          target_ends=None, padding=0, flags=IN | KEPT, depth_cap=0):
    assert flags & (IN | KEPT) and not flags & ~15
    lengths = np.atleast_1d(np.asarray(contig_lengths, np.int64))
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    kept_bit = dm.kept_bits(keep_mask, s.size).astype(np.int64)
    scope, regions_in, regions_merged = _scope(lengths, target_offsets, target_starts, target_ends, padding)
    order = np.argsort(ids, kind="stable")
    bounds = np.searchsorted(ids[order], np.arange(lengths.size + 1))
    runs, emitted, scope_positions, short_positions = [], 0, 0, 0
    for c, L in enumerate(lengths.tolist()):
        if L == 0 or not scope[c]:
            continue
        sel = order[bounds[c]:bounds[c + 1]]
        lo = np.array([a for a, _ in scope[c]], np.int64)
        hi = np.array([b for _, b in scope[c]], np.int64)
        # change points: where a read begins, where one has ended, where a scope interval begins and where one has ended
        pos = np.concatenate([s[sel], e[sel] + 1])
        d_cov = np.concatenate([np.ones(sel.size, np.int64), -np.ones(sel.size, np.int64)])
        d_kept = np.concatenate([kept_bit[sel], -kept_bit[sel]])
        cuts = np.unique(np.concatenate([[0, L], pos, lo, hi + 1]))
        cuts = cuts[cuts <= L]
        at = np.searchsorted(cuts, pos[pos <= L])
        net_cov, net_kept = np.zeros(cuts.size, np.int64), np.zeros(cuts.size, np.int64)
        np.add.at(net_cov, at, d_cov[pos <= L])
        np.add.at(net_kept, at, d_kept[pos <= L])
        # segment i = [cuts[i], cuts[i + 1] - 1] with one depth and inside or outside one scope interval
        seg_lo, seg_hi = cuts[:-1], cuts[1:] - 1
        cov, kept = np.cumsum(net_cov)[:-1], np.cumsum(net_kept)[:-1]
        k = np.searchsorted(lo, seg_lo, side="right") - 1
        inside = (k >= 0) & (seg_lo <= hi[np.maximum(k, 0)])
        din, dk, short, em = _tuples(cov, kept, M, flags, depth_cap)
        em &= inside
        seg_len = seg_hi - seg_lo + 1
        emitted += int(seg_len[em].sum())
        scope_positions += int(seg_len[inside].sum())
        short_positions += int(seg_len[inside & short].sum())
        same = em[1:] & em[:-1] & (k[1:] == k[:-1]) & (din[1:] == din[:-1]) & (dk[1:] == dk[:-1]) & \
            (short[1:] == short[:-1])                              # segment i + 1 continues the run of segment i
        head = em & np.concatenate([[True], ~same])
        tail = em & np.concatenate([~same, [True]])
        h, t = np.flatnonzero(head), np.flatnonzero(tail)
        assert h.size == t.size
        runs += list(zip([c] * h.size, seg_lo[h].tolist(), seg_hi[t].tolist(), din[h].tolist(), dk[h].tolist(),
                         short[h].astype(np.int64).tolist()))
    return runs, _stats(ids, keep_mask, runs, emitted, scope_positions, short_positions, regions_in, regions_merged)


def track_positions(starts, ends, contig_ids, contig_lengths, M, keep_mask=None, target_offsets=None, target_starts=None,
                    target_ends=None, padding=0, flags=IN | KEPT, depth_cap=0):
    lengths = np.atleast_1d(np.asarray(contig_lengths, np.int64))
    ids = np.asarray(contig_ids, np.int64)
    covs = dm.coverages(starts, ends, ids, lengths, keep_mask)
    regions_in = regions_merged = 0
    if target_offsets is not None:
        regions_in = int(np.asarray(target_offsets)[-1])
        sets = tm.target_sets(lengths, target_offsets, target_starts if regions_in else [],
                              target_ends if regions_in else [], padding)
        regions_merged = sum(len(tm.merged_regions(t)) for t in sets)
    else:
        sets = [np.ones(int(L), bool) for L in lengths.tolist()]
    runs, emitted, scope_positions, short_positions = [], 0, 0, 0
    for c, L in enumerate(lengths.tolist()):
        cov, kept = covs[c]
        open_run = None                                             # [contig, start, end, din, dk, short]
        for p in range(L):
            tup = None
            if sets[c][p]:
                scope_positions += 1
                short = int(kept[p] < min(cov[p], M))
                short_positions += short
                din = (min(int(cov[p]), depth_cap) if depth_cap else int(cov[p])) if flags & IN else 0
                dk = (min(int(kept[p]), depth_cap) if depth_cap else int(kept[p])) if flags & KEPT else 0
                if not (flags & SHORT_ONLY and not short) and not (flags & SKIP_ZERO and din == 0 and dk == 0):
                    tup = (din, dk, short)
            # (p - 1 in scope and p in scope: one merged region, because merged regions are a position apart)
            if open_run is not None and tup is not None and tuple(open_run[3:]) == tup and sets[c][p - 1]:
                open_run[2] = p
                emitted += 1
                continue
            if open_run is not None:
                runs.append(tuple(open_run))
                open_run = None
            if tup is not None:
                open_run = [c, p, p, *tup]
                emitted += 1
        if open_run is not None:
            runs.append(tuple(open_run))
    return runs, _stats(ids, keep_mask, runs, emitted, scope_positions, short_positions, regions_in, regions_merged)


def run_bound(stats, n_contigs):
    """the header's invariant: n_runs <= min(positions_in_runs, 2 * reads_placed + n_contigs + regions_merged)"""
    return min(stats["positions_in_runs"], 2 * stats["reads_placed"] + n_contigs + stats["regions_merged"])


def assert_equal(got_runs, got_stats, want, info=""):
    """a package result (structured array, TrackStats) against (runs, stats) of a model, bit for bit"""
    want_runs, want_stats = want
    got = [tuple(int(x) for x in r) for r in got_runs.tolist()]
    assert len(got) == len(want_runs), (info, len(got), len(want_runs))
    assert got == want_runs, (info, next((i, g, w) for i, (g, w) in enumerate(zip(got, want_runs)) if g != w))
    for key, v in want_stats.items():
        assert getattr(got_stats, key) == v, (info, key, getattr(got_stats, key), v)
