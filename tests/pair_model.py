"""Pair-aware downsampling (qmcp_hip_solve_pairs_*), restated for the tests on the coverage profile's model
(tests/profile_model.py) and the oracle's find_pairs.  Reads (2q, 2q + 1) are pair q; targets T_1 < ... < T_k = M.
  S_0 = {}; stage j: credit(p) = the depth of the placed reads of S_(j-1); cap(p) = max(0, T_j - credit(p)); K_j = the
  canonical selection under that cap ARRAY over the placed reads NOT in S_(j-1), alone, in input order, per contig;
  S_j = find_pairs(S_(j-1) | K_j).
  default_stages   {ceil(M / 2), M}, {1} for M = 1
  staged           -> (mask of S_k, [|K_j|], [|S_j|], [S_j as bool arrays]); fast=True walks the breakpoints
                   (profile_model.fast_select over regions_of(cap)) instead of every position (profile_model.select)
  plain            the by-contig selection at M and find_pairs: what the file flow does without the feature
  covers           every S_j is valid: its depth is >= min(cov, T_j) on every contig
  overshoot        the generator of the fixture: pairs of rl-base reads, the mate 100 .. 499 positions behind"""
import numpy as np

import profile_model as pm

NO_CONTIG = pm.NO_CONTIG


def default_stages(M):
    M = int(M)
    return [M] if M == 1 else [M - M // 2, M]


def _select_rest(s, e, L, cap, fast):
    if not fast:
        return pm.select(s, e, cap)
    _, r0, r1, caps = pm.regions_of(cap)
    return pm.fast_select(s, e, L, 0, list(zip(r0.tolist(), r1.tolist(), caps.tolist())))


def staged(oracle, starts, ends, contig_ids, contig_lengths, M, stages=None, fast=False):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    lengths = np.atleast_1d(contig_lengths).tolist()
    stages = default_stages(M) if stages is None else [int(t) for t in stages]
    assert stages[-1] == int(M) and all(a < b for a, b in zip(stages, stages[1:])) and stages[0] >= 1
    n = s.size
    assert n % 2 == 0
    on = [np.flatnonzero(ids == c) for c in range(len(lengths))]
    S = np.zeros(n, bool)
    selected, kept, sets = [], [], []
    for T in stages:
        K = np.zeros(n, bool)
        for c, L in enumerate(lengths):
            rest, have = on[c][~S[on[c]]], on[c][S[on[c]]]
            if rest.size == 0 or L == 0:
                continue
            cap = np.maximum(0, T - pm.coverage(s[have], e[have], L))
            K[rest] = _select_rest(s[rest], e[rest], L, cap, fast)
        S = pm.unpack(oracle.find_pairs(pm.pack(S | K), n), n) if n else S
        selected.append(int(K.sum()))
        kept.append(int(S.sum()))
        sets.append(S.copy())
    return pm.pack(S), selected, kept, sets


def plain(oracle, starts, ends, contig_ids, contig_lengths, M):
    """solve read by read at M, then complete the pairs"""
    import multi_reference as mr
    n = np.asarray(starts).size
    return oracle.find_pairs(mr.oracle_by_contig(oracle, starts, ends, contig_ids, contig_lengths, M), n)


def covers(starts, ends, contig_ids, contig_lengths, kept_bits, T):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    for c, L in enumerate(np.atleast_1d(contig_lengths).tolist()):
        sel = np.flatnonzero(ids == c)
        sub = sel[kept_bits[sel]]
        if not np.all(pm.coverage(s[sub], e[sub], L) >= np.minimum(pm.coverage(s[sel], e[sel], L), T)):
            return False
    return True


def whole_pairs(bits):
    return bool(np.array_equal(bits[0::2], bits[1::2]))


def mean_kept_depth(starts, ends, kept_bits, L):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    return float((e[kept_bits] - s[kept_bits] + 1).sum()) / L


def overshoot(seed, L, M, depth, rl=150):
    rng = np.random.default_rng(seed)
    npairs = int(depth * M * L / rl / 2)
    s1 = rng.integers(0, L - rl - 500, size=npairs)
    s2 = s1 + rng.integers(100, 500, size=npairs)
    s = np.empty(2 * npairs, np.int64)
    s[0::2] = s1
    s[1::2] = s2
    e = s + rl - 1
    return s.astype(np.uint32), e.astype(np.uint32), np.zeros(2 * npairs, np.uint32), np.array([L], np.uint32)
