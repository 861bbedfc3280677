"""On-target downsampling (qmcp_hip_solve_targets_*), restated for the tests with numpy prefix sums -- no binary search,
no merged table: a contig's target set is a boolean array, rank its exclusive prefix sum.
  target_sets      per contig, which positions are targets (regions padded, clipped to the contig)
  merged_regions   the maximal runs of a target set: what target_table.h's table must hold
  project          every read's projection [rank(s), rank(e + 1) - 1] and whether it is on target
  expected_mask    project, solve every contig's on-target reads in input order with the oracle, map back"""
import numpy as np

import multi_reference as mr

NO_CONTIG = 0xFFFFFFFF


def target_sets(contig_lengths, target_offsets, target_starts, target_ends, padding=0):
    lengths = np.atleast_1d(np.asarray(contig_lengths, np.int64))
    offs = np.asarray(target_offsets, np.int64)
    t0, t1 = np.asarray(target_starts, np.int64), np.asarray(target_ends, np.int64)
    sets = []
    for c, L in enumerate(lengths.tolist()):
        diff = np.zeros(L + 1, np.int64)
        for k in range(int(offs[c]), int(offs[c + 1])):
            a, b = max(int(t0[k]) - padding, 0), min(int(t1[k]) + padding, L - 1)
            if a < L:                       # (a region beyond the contig is dropped)
                diff[a] += 1
                diff[b + 1] -= 1
        sets.append(np.cumsum(diff)[:L] > 0)
    return sets


def merged_regions(target_set):
    """[(start, end, target positions before it)] of the maximal runs"""
    t = np.concatenate([[False], target_set, [False]]).astype(np.int8)
    d = np.diff(t)
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1
    cum = np.concatenate([[0], np.cumsum(ends - starts + 1)])[:-1]
    return list(zip(starts.tolist(), ends.tolist(), cum.tolist()))


def project(starts, ends, contig_ids, contig_lengths, target_offsets, target_starts, target_ends, padding=0):
    """-> (on_target, projected starts, projected ends, |T_c| per contig); the projection is 0 where off target"""
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    sets = target_sets(contig_lengths, target_offsets, target_starts, target_ends, padding)
    on = np.zeros(s.size, bool)
    ps, pe = np.zeros(s.size, np.int64), np.zeros(s.size, np.int64)
    for c, tset in enumerate(sets):
        sel = np.flatnonzero(ids == c)
        if sel.size == 0:
            continue
        rank = np.concatenate([[0], np.cumsum(tset)])          # rank[p] = targets before p
        a, b = rank[s[sel]], rank[e[sel] + 1] - 1
        hit = a <= b
        on[sel] = hit
        ps[sel] = np.where(hit, a, 0)
        pe[sel] = np.where(hit, b, 0)
    tlen = np.array([int(t.sum()) for t in sets], np.int64)
    return on, ps, pe, tlen


def expected_mask(oracle, starts, ends, contig_ids, contig_lengths, target_offsets, target_starts, target_ends, M,
                  padding=0, keep_off_target=False, qualities=None, quality_choice=None):
    """the input-order keep mask of the contract.  With qualities, quality_choice (quality_model.quality_choice) is
    applied to the projected problem.  -> (mask, on_target)"""
    ids = np.asarray(contig_ids, np.uint32)
    n = ids.size
    on, ps, pe, tlen = project(starts, ends, ids, contig_lengths, target_offsets, target_starts, target_ends, padding)
    sel = np.flatnonzero(on)
    bits = np.zeros(((n + 63) // 64) * 64, np.uint8)
    live = np.flatnonzero(tlen > 0)                              # the oracle never sees a contig without targets
    if sel.size:
        renum = np.full(tlen.size, NO_CONTIG, np.int64)
        renum[live] = np.arange(live.size)
        cid = renum[ids[sel].astype(np.int64)].astype(np.uint32)
        cs, ce = ps[sel].astype(np.uint32), pe[sel].astype(np.uint32)
        m = mr.oracle_by_contig(oracle, cs, ce, cid, tlen[live].astype(np.uint32), M)
        if qualities is not None:
            m = quality_choice(m, cs, ce, cid, np.asarray(qualities)[sel])
        kept = np.unpackbits(np.ascontiguousarray(m).view(np.uint8), bitorder="little")[:sel.size].astype(bool)
        bits[sel[kept]] = 1
    if keep_off_target:
        bits[np.flatnonzero((ids != NO_CONTIG) & ~on)] = 1
    return np.packbits(bits, bitorder="little").view(np.uint64)[:(n + 63) // 64].copy(), on


def random_regions(rng, lengths, max_regions=6, max_len=400, outside=0.1, empty=0.2):
    """CSR regions per contig: overlapping, nested, adjacent, some beyond the contig, some contigs without any"""
    offs, t0, t1 = [0], [], []
    for L in np.atleast_1d(lengths).tolist():
        k = 0 if rng.random() < empty else int(rng.integers(1, max_regions + 1))
        for _ in range(k):
            if L == 0 or rng.random() < outside:
                a = L + int(rng.integers(0, 50))
            else:
                a = int(rng.integers(0, L))
            b = a + int(rng.integers(0, max_len))
            t0.append(a)
            t1.append(b)
            if rng.random() < 0.3:                               # an adjacent one, and a nested one
                t0.append(b + 1)
                t1.append(b + 1 + int(rng.integers(0, max_len)))
                t0.append(a + (b - a) // 3)
                t1.append(a + (b - a) // 2)
        offs.append(len(t0))
    return np.array(offs, np.uint32), np.array(t0, np.uint32), np.array(t1, np.uint32)
