"""The contract of qmcp_hip_solve_amplicons_* (include/qmcp_hip.h) stated literally: brute-force assignment of every unit
to an amplicon of its contig (greatest start, then smallest end, then smallest index among the amplicons that contain all
of its reads), the clip to the insert, both solves composed from the oracle (pooled: tests/multi_reference.py's
oracle_by_contig on the clipped reads; per amplicon: the same with the amplicon's index as contig id on the reads rebased
to the insert), oracle.find_pairs for the mates, and the rows and stats in numpy (tests/depth_model.py's row)."""
import numpy as np

import depth_model as dm
import multi_reference as mr
from dedup_model import pack, unpack  # noqa: F401  (the tests take both from here)

NO_CONTIG = mr.NO_CONTIG
NO_AMPLICON = 0xFFFFFFFF
STAT_KEYS = ("units", "units_assigned", "units_filtered", "units_no_amplicon", "units_in_several", "reads_shortened",
             "reads_clipped_away", "bases_clipped", "amplicons", "amplicons_unused")


def containers(offs, a0, a1, c, s, e):
    """the amplicons of contig c (indices in the table) that contain [s, e], best first by the rule"""
    lo, hi = int(offs[c]), int(offs[c + 1])
    ks = lo + np.flatnonzero((np.asarray(a0[lo:hi], np.int64) <= s) & (e <= np.asarray(a1[lo:hi], np.int64)))
    return sorted(ks.tolist(), key=lambda k: (-int(a0[k]), int(a1[k]), k))


def assign_unit(offs, a0, a1, ids, starts, ends):
    """one unit (the sequences hold its reads) -> (label or NO_AMPLICON, contained in several)"""
    ids = [int(x) for x in ids]
    if any(i == NO_CONTIG for i in ids) or len(set(ids)) != 1:
        return NO_AMPLICON, False
    ks = containers(offs, a0, a1, ids[0], min(int(x) for x in starts), max(int(x) for x in ends))
    return (ks[0], len(ks) > 1) if ks else (NO_AMPLICON, False)


def assign_and_clip(starts, ends, contig_ids, offs, a0, a1, i0=None, i1=None, seq_lengths=None, qualities=None,
                    min_length=0, min_mapq=0, single_end=False):
    """-> dict(labels, cs, ce, placed, stats): labels per unit; per read the clipped bounds in genome coordinates and
    whether the read is still placed (reads of unassigned units are not); the counters of the assign step"""
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    a0, a1 = np.asarray(a0, np.int64), np.asarray(a1, np.int64)
    i0 = a0 if i0 is None else np.asarray(i0, np.int64)
    i1 = a1 if i1 is None else np.asarray(i1, np.int64)
    n = s.size
    per = 1 if single_end else 2
    assert n % per == 0
    n_units = n // per
    ok = np.ones(n, bool)
    if qualities is not None:
        ok &= np.asarray(qualities, np.int64) >= min_mapq
    if seq_lengths is not None:
        ok &= np.asarray(seq_lengths, np.int64) >= min_length
    labels = np.full(n_units, NO_AMPLICON, np.uint32)
    cs, ce, placed = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["units"], st["amplicons"] = n_units, int(a0.size)
    for u in range(n_units):
        r = slice(per * u, per * u + per)
        if not ok[r].all():
            st["units_filtered"] += 1
            continue
        k, several = assign_unit(offs, a0, a1, ids[r], s[r], e[r])
        if k == NO_AMPLICON:
            st["units_no_amplicon"] += 1
            continue
        labels[u] = k
        st["units_assigned"] += 1
        st["units_in_several"] += int(several)
        for i in range(per * u, per * u + per):
            lo, hi = max(s[i], i0[k]), min(e[i], i1[k])
            if lo > hi:
                st["reads_clipped_away"] += 1
                st["bases_clipped"] += int(e[i] - s[i] + 1)
                continue
            if lo != s[i] or hi != e[i]:
                st["reads_shortened"] += 1
                st["bases_clipped"] += int((lo - s[i]) + (e[i] - hi))
            cs[i], ce[i], placed[i] = lo, hi, True
    st["amplicons_unused"] = int(a0.size - np.unique(labels[labels != NO_AMPLICON]).size)
    return dict(labels=labels, cs=cs, ce=ce, placed=placed, stats=st)


def rebased(ac, i0, single_end):
    """the clipped reads rebased to their amplicon's insert -> (starts, ends, amplicon ids with NO_CONTIG if unplaced)"""
    per = 1 if single_end else 2
    lab = np.repeat(ac["labels"].astype(np.int64), per)
    i0 = np.asarray(i0, np.int64)
    base = np.where(ac["placed"], i0[np.where(ac["placed"], lab, 0)] if i0.size else 0, 0)
    rid = np.where(ac["placed"], lab, NO_CONTIG)
    return ((ac["cs"] - base) * ac["placed"]).astype(np.uint32), ((ac["ce"] - base) * ac["placed"]).astype(np.uint32), \
        rid.astype(np.uint32)


def rows(rs, re, rid, i0, i1, M, keep):
    """one tuple in the field order of qmcp_hip_depth_row per amplicon, over its insert"""
    i0, i1 = np.asarray(i0, np.int64), np.asarray(i1, np.int64)
    covs = dm.coverages(rs, re, rid, i1 - i0 + 1, pack(keep))
    out = []
    for k in range(i0.size):
        r = dm.row(k, 0, int(i1[k] - i0[k]), covs[k][0], covs[k][1], M)
        out.append((k, int(i0[k]), int(i1[k])) + r[3:])
    return out


def solve(oracle, starts, ends, contig_ids, contig_lengths, M, offs, a0, a1, i0=None, i1=None, seq_lengths=None,
          qualities=None, min_length=0, min_mapq=0, single_end=False, per_amplicon=False, complete_pairs=False):
    """-> (keep bits in input order, labels, rows, stats dict)"""
    assert not (single_end and complete_pairs)
    ac = assign_and_clip(starts, ends, contig_ids, offs, a0, a1, i0, i1, seq_lengths, qualities, min_length, min_mapq,
                         single_end)
    a0, a1 = np.asarray(a0, np.int64), np.asarray(a1, np.int64)
    i0 = a0 if i0 is None else np.asarray(i0, np.int64)
    i1 = a1 if i1 is None else np.asarray(i1, np.int64)
    n = np.asarray(starts).size
    per = 1 if single_end else 2
    on = np.flatnonzero(np.repeat(ac["labels"] != NO_AMPLICON, per))   # the reads of the assigned units, input order
    rs, re, rid = rebased(ac, i0, single_end)
    keep = np.zeros(n, bool)
    if on.size:
        if per_amplicon:
            m = mr.oracle_by_contig(oracle, rs[on], re[on], rid[on], (i1 - i0 + 1).astype(np.uint32), M)
        else:
            ids = np.where(ac["placed"], np.asarray(contig_ids, np.int64), NO_CONTIG).astype(np.uint32)
            m = mr.oracle_by_contig(oracle, ac["cs"][on].astype(np.uint32), ac["ce"][on].astype(np.uint32), ids[on],
                                    contig_lengths, M)
        if complete_pairs:
            m = oracle.find_pairs(m, on.size)
        keep[on[unpack(m, on.size)]] = True
    return keep, ac["labels"], rows(rs, re, rid, i0, i1, M, keep), ac["stats"]


def fragmented_panel(seed, n_amp=9, size=400, step=300, primer=25, mean_yield=1050):
    """the motivating experiment's input: one contig of 3 000 bases (more if the panel needs it) tiled with n_amp amplicons,
    primers of `primer` bases, log-normal yields per amplicon, single reads of 60 - 200 bases placed at random inside
    their amplicon, 40 % of them flush with one of its edges (a fragmented library), shuffled
    -> (starts, ends, ids, lengths, offs, a0, a1, i0, i1)"""
    rng = np.random.default_rng(seed)
    a0 = np.arange(n_amp, dtype=np.int64) * step
    a1 = a0 + size - 1
    lengths = np.array([max(int(a1[-1]) + 1, 3000)], np.uint32)
    counts = np.maximum((mean_yield * rng.lognormal(0.0, 0.25, size=n_amp)).astype(np.int64), 1)
    k = np.repeat(np.arange(n_amp), counts)
    span = rng.integers(60, 201, size=k.size)
    s = a0[k] + (rng.random(k.size) * (size - span + 1)).astype(np.int64)
    edge = rng.random(k.size)
    s = np.where(edge < 0.2, a0[k], np.where(edge < 0.4, a1[k] - span + 1, s))
    perm = rng.permutation(k.size)
    s, e = s[perm], (s + span - 1)[perm]
    u32 = lambda x: np.asarray(x).astype(np.uint32)
    return (u32(s), u32(e), np.zeros(k.size, np.uint32), lengths, np.array([0, n_amp], np.uint32), u32(a0), u32(a1),
            u32(a0 + primer), u32(a1 - primer))


def trimmed_shortfall(starts, ends, contig_ids, contig_lengths, offs, a0, a1, i0, i1, M, keep, single_end=False):
    """positions where the primer-trimmed depth of `keep` is below min(primer-trimmed depth of all reads, M), and the
    worst shortfall: what the motivating experiment counts.  Reads are trimmed by their own assigned amplicon"""
    ac = assign_and_clip(starts, ends, contig_ids, offs, a0, a1, i0, i1, single_end=single_end)
    ids = np.where(ac["placed"], np.asarray(contig_ids, np.int64), NO_CONTIG)
    short, worst = 0, 0
    for cov, kept in dm.coverages(ac["cs"], ac["ce"], ids, contig_lengths, pack(keep)):
        lack = np.maximum(np.minimum(cov, M) - kept, 0)
        short += int((lack > 0).sum())
        worst = max(worst, int(lack.max()) if lack.size else 0)
    return short, worst
