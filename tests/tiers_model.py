"""Tiered downsampling (qmcp_hip_solve_tiers_*), restated for the tests on the coverage profile's model
(tests/profile_model.py).  tiers[i] < n_tiers names read i's tier, 0 the best; NO_TIER and NO_CONTIG reads are never kept.
  S_(-1) = {}; tier t: R_t = the placed reads of tier t alone, in input order; credit(p) = the depth of S_(t-1);
  cap(p) = max(0, M - credit(p)); K_t = the canonical selection over R_t under that cap ARRAY, per contig
  (need_t = min(cov_(R_t), cap)); S_t = S_(t-1) | K_t.
  tiered        -> (kept bits of S_last in input order, rows[n_tiers, 7], [K_t as bool arrays]); fast=True walks the
                breakpoints (profile_model.fast_select over regions_of(cap)) instead of every position
                (profile_model.select).  rows: placed reads, kept reads, bases, kept bases, demand (the sum of need_t),
                asked positions (need_t > 0), capped positions (cov_(R_t) > cap); the last three are 0 for tier 0,
                whose plain solves build no need, and at M = 0, where no solver call is made
  needs         per contig, (need_t, cov_t, cap) of one tier given the kept bits before it: what brute-force checks and
                the guarantees read
  covers        the kept depth is >= min(cov of the tiered placed reads, M) on every contig (guarantee 1)
  rows_of / counters_of   a list of TierRow -> the same array
  instance      the generator: mixed spans on a few contigs, tiers drawn by weight, "repeat" stretches in which no read
                is of tier 0, a few NO_TIER and NO_CONTIG reads"""
import numpy as np

import profile_model as pm

NO_CONTIG = pm.NO_CONTIG
NO_TIER = 0xFFFFFFFF
TIERS_MAX = 16


def _select(s, e, L, cap, fast):
    if not fast:
        return pm.select(s, e, cap)
    _, r0, r1, caps = pm.regions_of(cap)
    return pm.fast_select(s, e, L, 0, list(zip(r0.tolist(), r1.tolist(), caps.tolist())))


def members(contig_ids, tiers, n_contigs, n_tiers):
    """on[t][c]: the input indices of tier t's reads on contig c, ascending"""
    ids, tr = np.asarray(contig_ids, np.int64), np.asarray(tiers, np.int64)
    return [[np.flatnonzero((tr == t) & (ids == c)) for c in range(n_contigs)] for t in range(n_tiers)]


def needs(starts, ends, on_t, lengths, kept_before, M, all_on):
    """one tier: per contig (need, cov, cap); kept_before: the kept bits of the tiers before it, all_on: every tiered
    placed read of the contig (any tier), to take the credit from"""
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    out = []
    for c, L in enumerate(lengths):
        have = all_on[c][kept_before[all_on[c]]]
        cap = np.maximum(0, int(M) - pm.coverage(s[have], e[have], L))
        cov = pm.coverage(s[on_t[c]], e[on_t[c]], L)
        out.append((np.minimum(cov, cap), cov, cap))
    return out


def tiered(starts, ends, contig_ids, tiers, contig_lengths, M, n_tiers, fast=False):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids, tr = np.asarray(contig_ids, np.int64), np.asarray(tiers, np.int64)
    lengths = np.atleast_1d(contig_lengths).tolist()
    on = members(ids, tr, len(lengths), n_tiers)
    all_on = [np.flatnonzero((ids == c) & (tr < n_tiers)) for c in range(len(lengths))]
    S = np.zeros(s.size, bool)
    rows = np.zeros((n_tiers, 7), np.int64)
    picks = []
    for t in range(n_tiers):
        K = np.zeros(s.size, bool)
        for c, (L, (need, cov, cap)) in enumerate(zip(lengths, needs(s, e, on[t], lengths, S, M, all_on))):
            sel = on[t][c]
            if sel.size == 0 or L == 0:
                continue
            K[sel] = _select(s[sel], e[sel], L, cap, fast)
            if t > 0 and int(M) > 0:
                rows[t, 4] += int(need.sum())
                rows[t, 5] += int((need > 0).sum())
                rows[t, 6] += int((cov > cap).sum())
        S |= K
        picks.append(K)
        mine = np.concatenate(on[t]) if on[t] else np.zeros(0, np.int64)
        span = e[mine] - s[mine] + 1
        rows[t, :4] = [mine.size, int(K.sum()), int(span.sum()), int(span[K[mine]].sum())]
    return S, rows, picks


def covers(starts, ends, contig_ids, tiers, contig_lengths, M, n_tiers, kept_bits):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids, tr = np.asarray(contig_ids, np.int64), np.asarray(tiers, np.int64)
    for c, L in enumerate(np.atleast_1d(contig_lengths).tolist()):
        sel = np.flatnonzero((ids == c) & (tr < n_tiers))
        sub = sel[kept_bits[sel]]
        if not np.all(pm.coverage(s[sub], e[sub], L) >= np.minimum(pm.coverage(s[sel], e[sel], L), int(M))):
            return False
    return True


def rows_of(tier_rows):
    return np.array([[r.n_reads, r.n_kept, r.bases_in, r.bases_kept, r.demand, r.asked_positions, r.capped_positions]
                     for r in tier_rows], dtype=np.int64).reshape(-1, 7)


def untiered(tiers):
    return int((np.asarray(tiers, np.uint32) == NO_TIER).sum())


def draw_tiers(rng, n, weights):
    w = np.asarray(weights, float)
    return rng.choice(w.size, size=n, p=w / w.sum()).astype(np.uint32)


def instance(rng, lengths, n_reads, spans, weights, repeats=(), no_tier=0.0, no_contig=0.0):
    """n_reads reads with spans in [spans[0], spans[1]] spread over the contigs by length, tiers drawn by `weights`;
    repeats: (contig, first, last) stretches -- a tier-0 read that touches one is redrawn among the later tiers (kept
    in tier 0 when there is no later tier).  -> starts, ends, contig_ids, tiers (uint32), in shuffled order"""
    lengths = np.atleast_1d(np.asarray(lengths, np.int64))
    ids = rng.choice(lengths.size, size=n_reads, p=lengths / lengths.sum())
    span = np.minimum(rng.integers(spans[0], spans[1] + 1, size=n_reads), lengths[ids])
    s = (rng.random(n_reads) * (lengths[ids] - span + 1)).astype(np.int64)
    e = s + span - 1
    tiers = draw_tiers(rng, n_reads, weights).astype(np.int64)
    if len(weights) > 1:
        for c, a, b in repeats:
            hit = np.flatnonzero((ids == c) & (tiers == 0) & (s <= b) & (e >= a))
            tiers[hit] = 1 + draw_tiers(rng, hit.size, weights[1:])
    ids = ids.astype(np.int64)
    tiers[rng.random(n_reads) < no_tier] = NO_TIER
    ids[rng.random(n_reads) < no_contig] = NO_CONTIG
    u = lambda x: np.asarray(x, np.int64).astype(np.uint32)
    return u(s), u(e), u(ids), u(tiers)


# ---------------------------------------------------------------- a BAM with MAPQ bands (tests only)
REFERENCES = [("chr1", 6_000), ("chr2", 3_000)]
LOW_STRETCH = (0, 2_000, 2_599)          # (reference, first, last): every record that touches it has MAPQ below 30


def write_tiers_bam(path, rng, n_pairs=1500):
    """pairs on two references in shuffled file order, MAPQ 30 .. 60 for 85 % of the records, 10 .. 29 for 10 %, 0 .. 9 for
    the rest; a record that touches LOW_STRETCH is redrawn below 30, so the best band is absent there; a few records
    unmapped -> (header, parsed records, reference lengths)"""
    import bam_py
    recs = []
    for q in range(n_pairs):
        ref = int(rng.integers(0, len(REFERENCES)))
        for first in (True, False):
            flag = (0x41 if first else 0x81) | (0x10 if rng.random() < 0.5 else 0)
            if rng.random() < 0.02:
                recs.append(bam_py.pack_record(f"p{q}", flag | 0x4, -1, 0, [], 100, ref_id=-1))
                continue
            L = REFERENCES[ref][1]
            match = int(rng.integers(60, 151))
            pos = int(rng.integers(0, L - match))
            roll = rng.random()
            mapq = int(rng.integers(30, 61)) if roll < 0.85 else int(rng.integers(10, 30)) if roll < 0.95 else int(rng.integers(0, 10))
            if ref == LOW_STRETCH[0] and pos <= LOW_STRETCH[2] and pos + match - 1 >= LOW_STRETCH[1] and mapq >= 30:
                mapq = int(rng.integers(0, 30))
            recs.append(bam_py.pack_record(f"p{q}", flag, pos, mapq, [(match, "M")], match, ref_id=ref))
    recs = [recs[i] for i in rng.permutation(len(recs))]
    bam_py.write_bam(path, REFERENCES, recs)
    return bam_py.parse(path)
