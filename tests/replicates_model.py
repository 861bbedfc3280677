"""Disjoint replicates (qmcp_hip_solve_replicates_*) restated on the oracle: replicate 1 is the per-contig canonical
selection of all reads (multi_reference.oracle_by_contig) at coverages[0]; replicate r + 1 the same selection, at
coverages[r], of the placed reads no earlier replicate took, alone, in input order with their contig ids.  Under
WHOLE_PAIRS a placed read whose placed mate (reads 2q, 2q + 1) is in the replicate joins it.  The result is one byte per
read: the replicate that holds it (1-based), 0 for none.  The shortfall is plain numpy on per-contig depth arrays."""
import numpy as np

import multi_reference as mr

WHOLE_PAIRS, SHORTFALL = 1, 2


def replicate_labels(oracle, starts, ends, contig_ids, contig_lengths, coverages, flags=0):
    """-> (uint8[n_reads] labels, dict of n_offered / n_kept / n_mates lists, one entry per replicate)"""
    s, e = np.asarray(starts, dtype=np.uint32), np.asarray(ends, dtype=np.uint32)
    ids = np.asarray(contig_ids, dtype=np.uint32)
    n = s.size
    assert not (flags & WHOLE_PAIRS) or n % 2 == 0
    labels = np.zeros(n, dtype=np.uint8)
    placed = ids != mr.NO_CONTIG
    info = {"n_offered": [], "n_kept": [], "n_mates": []}
    for r, M in enumerate(coverages, start=1):
        free = np.flatnonzero(placed & (labels == 0))       # input indices of the reads still free, in input order
        info["n_offered"].append(int(free.size))
        mask = mr.oracle_by_contig(oracle, s[free], e[free], ids[free], contig_lengths, int(M))
        bits = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[:free.size].astype(bool)
        labels[free[bits]] = r
        mates = 0
        if flags & WHOLE_PAIRS:
            a, b = labels[0::2], labels[1::2]               # views: the assignments below write labels
            join_b = (a == r) & (b == 0) & placed[1::2]
            join_a = (b == r) & (a == 0) & placed[0::2]
            b[join_b] = r
            a[join_a] = r
            mates = int(join_a.sum() + join_b.sum())
        info["n_mates"].append(mates)
        info["n_kept"].append(int((labels == r).sum()))
    return labels, info


def replicate_mask(labels, r):
    """the packed input-order mask of R_r"""
    labels = np.asarray(labels, dtype=np.uint8)
    bits = np.zeros(((labels.size + 63) // 64) * 64, dtype=np.uint8)
    bits[:labels.size] = labels == r
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def depth(s, e, L):
    d = np.zeros(L + 1, dtype=np.int64)
    np.add.at(d, np.asarray(s, dtype=np.int64), 1)
    np.add.at(d, np.asarray(e, dtype=np.int64) + 1, -1)
    return np.cumsum(d)[:L]


def depths_by_contig(starts, ends, contig_ids, contig_lengths, select):
    """per contig, the depth of the reads `select` (a bool per read) picks"""
    ids = np.asarray(contig_ids, dtype=np.uint32)
    out = []
    for c, L in enumerate(np.atleast_1d(contig_lengths).tolist()):
        on = np.flatnonzero((ids == c) & select)
        out.append(depth(np.asarray(starts)[on], np.asarray(ends)[on], int(L)))
    return out


def shortfall(labels, starts, ends, contig_ids, contig_lengths, coverages):
    """-> (short_positions, short_bases, n_full): per replicate the positions where its depth is below min(cov, coverage)
    with cov the depth of ALL placed reads, the sum of the differences, and the leading replicates without any"""
    labels = np.asarray(labels)
    everyone = np.ones(labels.size, dtype=bool)
    cov = depths_by_contig(starts, ends, contig_ids, contig_lengths, everyone)
    sp, sb = [], []
    for r, M in enumerate(coverages, start=1):
        mine = depths_by_contig(starts, ends, contig_ids, contig_lengths, labels == r)
        gap = [np.minimum(c, int(M)) - d for c, d in zip(cov, mine)]
        sp.append(int(sum(int((g > 0).sum()) for g in gap)))
        sb.append(int(sum(int(g[g > 0].sum()) for g in gap)))
    n_full = 0
    while n_full < len(sp) and sp[n_full] == 0:
        n_full += 1
    return sp, sb, n_full


def guarantee_holds(labels, starts, ends, contig_ids, contig_lengths, coverages):
    """cov_Rr(p) >= min(cov(p) - sum_{j<r} cov_Rj(p), coverages[r - 1]) at every position of every contig"""
    labels = np.asarray(labels)
    left = depths_by_contig(starts, ends, contig_ids, contig_lengths, np.ones(labels.size, dtype=bool))
    for r, M in enumerate(coverages, start=1):
        mine = depths_by_contig(starts, ends, contig_ids, contig_lengths, labels == r)
        for c in range(len(left)):
            if (mine[c] < np.minimum(left[c], int(M))).any():
                return False
            left[c] = left[c] - mine[c]
    return True


# the island generator of tests/test_gpu_pairs.py: reads of spans 1..max_span (both present) in islands at both ends of
# every contig and around a multiple of 64 inside it, shuffled over the contigs, so mates mostly lie on different contigs
def island_pairs(seed, lengths, max_span, per_island=30):
    rng = np.random.default_rng(seed)
    ss, ee, ii = [], [], []
    for c, L in enumerate(lengths):
        for a in (0, 64 * int(rng.integers(L // 256, L // 128)), L - 1):
            span = np.minimum(rng.integers(1, max_span + 1, size=per_island), L)
            span[0], span[1] = min(max_span, L), 1
            s = np.clip(a - rng.integers(0, span) + rng.integers(-2, 3, size=per_island), 0, L - span)
            ss.append(s); ee.append(s + span - 1); ii.append(np.full(per_island, c))
    s, e, ids = (np.concatenate(x) for x in (ss, ee, ii))
    perm = rng.permutation(s.size)
    u = lambda x: np.asarray(x, np.uint32)
    return u(s[perm]), u(e[perm]), u(ids[perm]), u(lengths)
