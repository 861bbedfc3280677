"""Fragment depth (qmcp_hip_clip_templates_*, qmcp_hip_solve_fragments_*), restated for the tests.  Rows are the template
entry's segments: [start, end] inclusive on contig_id or NO_CONTIG, template_ids[i] < n_templates.
  clip            the definition, row by row: the placed segments of each (template, contig) group in the order (start,
                  input index); reach = the largest end among the earlier members; start <= reach < end moves the start
                  to reach + 1, end <= reach unplaces the row; -> (clipped starts, clipped contig ids, stats dict)
  fragment_depth  WITHOUT clip: per template the boolean union of its selected placed segments, summed over the templates
                  -> one int64 array per contig
  segment_depth   depth counted per segment -> one int64 array per contig
  staged          template_model.staged on clip's columns -> (mask, selected, kept, sets)
  random_fragments  templates whose segments are drawn around a common anchor so that most overlap: partial overlap,
                  containment, identical segments, abutting segments, members on another contig, about 5 % unplaced rows;
                  ids scattered as template_model.random_templates does (with its `large` template)
  contrast_pairs  the issue's contrast input: 600 pairs of 2 x 150 on one contig of 1 200 positions"""
import numpy as np

import profile_model as pm
import template_model as tm

NO_CONTIG = pm.NO_CONTIG
STAT_NAMES = ("n_placed", "n_clipped", "n_emptied", "bases_in", "bases_removed", "n_templates_overlapping", "max_group")


def clip(starts, ends, contig_ids, template_ids):
    s = np.asarray(starts, np.int64)
    e = np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    tids = np.asarray(template_ids, np.int64)
    n = s.size
    out_s, out_c = s.copy(), ids.copy()
    placed = np.flatnonzero(ids != NO_CONTIG)
    order = placed[np.lexsort((placed, s[placed], ids[placed], tids[placed]))] if placed.size else placed
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats["n_placed"] = int(placed.size)
    stats["bases_in"] = int((e[placed] - s[placed] + 1).sum())
    changed = set()
    group, reach, size = None, None, 0
    for i in order.tolist():
        key = (int(tids[i]), int(ids[i]))
        if key != group:
            group, reach, size = key, None, 0
        size += 1
        stats["max_group"] = max(stats["max_group"], size)
        if reach is not None:
            if e[i] <= reach:
                out_c[i] = NO_CONTIG
                stats["n_emptied"] += 1
                stats["bases_removed"] += int(e[i] - s[i] + 1)
                changed.add(key[0])
            elif s[i] <= reach:
                out_s[i] = reach + 1
                stats["n_clipped"] += 1
                stats["bases_removed"] += int(reach + 1 - s[i])
                changed.add(key[0])
        reach = int(e[i]) if reach is None else max(reach, int(e[i]))
    stats["n_templates_overlapping"] = len(changed)
    assert n == out_s.size
    return out_s.astype(np.uint32), out_c.astype(np.uint32), stats


def segment_depth(starts, ends, contig_ids, contig_lengths, selection=None):
    s, e, ids = np.asarray(starts, np.int64), np.asarray(ends, np.int64), np.asarray(contig_ids, np.int64)
    sel = np.ones(s.size, bool) if selection is None else np.asarray(selection, bool)
    out = []
    for c, L in enumerate(np.atleast_1d(contig_lengths).tolist()):
        on = sel & (ids == c)
        d = np.zeros(L + 1, np.int64)
        np.add.at(d, s[on], 1)
        np.add.at(d, e[on] + 1, -1)
        out.append(np.cumsum(d)[:L])
    return out


def fragment_depth(starts, ends, contig_ids, template_ids, contig_lengths, selection=None):
    """the number of templates that cover a position, by brute force: no sort, no reach"""
    s, e, ids = np.asarray(starts, np.int64), np.asarray(ends, np.int64), np.asarray(contig_ids, np.int64)
    tids = np.asarray(template_ids, np.int64)
    sel = np.ones(s.size, bool) if selection is None else np.asarray(selection, bool)
    out = []
    for c, L in enumerate(np.atleast_1d(contig_lengths).tolist()):
        depth = np.zeros(L, np.int64)
        rows = np.flatnonzero(sel & (ids == c))
        rows = rows[np.argsort(tids[rows], kind="stable")]
        cuts = np.flatnonzero(np.diff(tids[rows])) + 1
        for members in np.split(rows, cuts):
            if members.size == 0:
                continue
            lo, hi = int(s[members].min()), int(e[members].max())
            cover = np.zeros(hi - lo + 1, bool)
            for i in members.tolist():
                cover[s[i] - lo:e[i] - lo + 1] = True
            depth[lo:hi + 1] += cover
        out.append(depth)
    return out


def staged(starts, ends, contig_ids, template_ids, n_templates, contig_lengths, M, stages=None):
    cs, cc, _ = clip(starts, ends, contig_ids, template_ids)
    return tm.staged(cs, ends, cc, template_ids, n_templates, contig_lengths, M, stages)


def random_fragments(rng, n, contig_lengths, n_templates=None, large=0, unplaced=0.05):
    """-> (starts, ends, contig_ids, template_ids, n_templates), uint32"""
    lengths = np.atleast_1d(contig_lengths).astype(np.int64)
    tids, n_templates = tm.random_templates(rng, n, n_templates=n_templates, large=large)
    s, e = np.zeros(n, np.int64), np.zeros(n, np.int64)
    ids = np.full(n, NO_CONTIG, np.int64)
    order = np.argsort(tids, kind="stable")
    cuts = np.flatnonzero(np.diff(tids[order])) + 1 if n else np.zeros(0, np.int64)
    for members in (np.split(order, cuts) if n else []):
        c0 = int(rng.integers(0, lengths.size))
        anchor = int(rng.integers(0, lengths[c0]))
        prev = None
        for i in members.tolist():
            u = rng.random()
            if u < unplaced:
                s[i] = int(rng.integers(0, 50))
                e[i] = s[i] + int(rng.integers(0, 50))
                continue
            c = c0 if rng.random() < 0.9 else int(rng.integers(0, lengths.size))
            L = int(lengths[c])
            kind = rng.random()
            if prev is not None and prev[0] == c and kind < 0.12:                      # identical
                a, b = prev[1], prev[2]
            elif prev is not None and prev[0] == c and kind < 0.24 and prev[2] + 1 < L:  # abutting: no clip
                a = prev[2] + 1
                b = a + int(rng.integers(0, 40))
            elif prev is not None and prev[0] == c and kind < 0.36:                    # contained
                a = int(rng.integers(prev[1], prev[2] + 1))
                b = int(rng.integers(a, prev[2] + 1))
            else:                                                                      # around the anchor: most overlap
                base = anchor if c == c0 else int(rng.integers(0, L))
                a = base + int(rng.integers(-40, 41))
                b = a + int(rng.integers(0, 80))
            a = min(max(a, 0), L - 1)
            b = min(max(b, a), L - 1)
            s[i], e[i], ids[i] = a, b, c
            prev = (c, a, b)
    return s.astype(np.uint32), e.astype(np.uint32), ids.astype(np.uint32), tids, n_templates


def contrast_pairs():
    """one contig of 1 200 positions, 600 pairs of 2 x 150 with fragment lengths 160 .. 260 -> (s, e, ids, tids, n_templates,
    lengths, M)"""
    L, P, M = 1200, 600, 10
    rng = np.random.default_rng(1)
    fs = rng.integers(0, L - 260, P)
    fl = rng.integers(160, 261, P)
    s = np.empty(2 * P, np.int64)
    e = np.empty(2 * P, np.int64)
    s[0::2], e[0::2] = fs, fs + 149
    s[1::2], e[1::2] = fs + fl - 150, fs + fl - 1
    tids = (np.arange(2 * P) // 2).astype(np.uint32)
    return (s.astype(np.uint32), e.astype(np.uint32), np.zeros(2 * P, np.uint32), tids, P, np.array([L], np.uint32), M)
