"""Template-aware downsampling under a cap table (qmcp_hip_solve_templates_profile_*), restated for the tests:
tests/template_model.py's staged solve with a cap ARRAY per contig (tests/profile_model.py's cap_arrays) in the place of
the one target.  Targets T_1 < ... < T_k = M; the stage cap is c_j(p) = ceil(cap(p) * T_j / M).
  S_0 = {}; stage j: credit(p) = the depth of the placed segments of S_(j-1); need under max(0, c_j(p) - credit(p)); K_j =
  the canonical selection under that array over the placed segments NOT in S_(j-1), alone, in input order, per contig;
  S_j = complete(S_(j-1) | K_j).
  stage_cap        ceil(cap * T / M) on an int64 array (Python integers where the product could pass 2^63)
  staged           -> (mask of S_k, [|K_j|], [|S_j|], [S_j as bool arrays])
  covers           the depth of a set is >= min(cov, cap array) on every contig
  on_cap           -> (placed segments that cover a position with cap > 0, templates that own one)
  targets_as_regions   the brute-force restatement of the package's function: a boolean array per contig
  paired_targets   the seeded paired fixture under wide targets"""
import numpy as np

import pair_model
import profile_model as pm
import template_model as tm

NO_CONTIG = pm.NO_CONTIG
default_stages = pair_model.default_stages


def stage_cap(cap, T, M):
    cap = np.asarray(cap, np.int64)
    return (cap * int(T) + int(M) - 1) // int(M)              # caps stay below 2^31 and T <= M < 2^31: no overflow


def staged(starts, ends, contig_ids, template_ids, n_templates, contig_lengths, M, default_cap, offs=None, r0=None,
           r1=None, caps=None, stages=None, fast=True, counters=None, batches=None):
    """counters (a list): gets one (capped_positions, demand) per stage -- what the kernel that builds need[] counts in a
    stage after the first, (0, 0) for stage 1: over the position batches (lists of contigs; default: all contigs in one)
    that still hold a candidate and whose largest stage cap (the default's included) is positive, the positions with
    cov_rest > max(0, c_j - credit) and the sum of need"""
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    lengths = np.atleast_1d(contig_lengths).tolist()
    stages = default_stages(M) if stages is None else [int(t) for t in stages]
    assert stages[-1] == int(M) and all(a < b for a, b in zip(stages, stages[1:])) and stages[0] >= 1
    n = s.size
    assert n == 0 or int(np.max(template_ids)) < int(n_templates)
    cap = pm.cap_arrays(lengths, default_cap, offs, r0, r1, caps)
    on = [np.flatnonzero(ids == c) for c in range(len(lengths))]
    S = np.zeros(n, bool)
    selected, kept, sets = [], [], []
    batches = [list(range(len(lengths)))] if batches is None else batches
    batch_of = {c: b for b, group in enumerate(batches) for c in group}
    for j, T in enumerate(stages):
        K = np.zeros(n, bool)
        capped = demand = 0
        live = [any((~S[on[c]]).any() for c in group) for group in batches]          # a candidate is left
        top = [max([int(stage_cap(default_cap, T, M))] + [int(stage_cap(cap[c], T, M).max()) for c in group if lengths[c]])
               for group in batches]                                                  # the batch's largest stage cap
        for c, L in enumerate(lengths):
            rest, have = on[c][~S[on[c]]], on[c][S[on[c]]]
            if L == 0:
                continue
            room = np.maximum(0, stage_cap(cap[c], T, M) - pm.coverage(s[have], e[have], L))
            if j and live[batch_of[c]] and top[batch_of[c]] > 0:
                cov_rest = pm.coverage(s[rest], e[rest], L)
                capped += int((cov_rest > room).sum())
                demand += int(np.minimum(cov_rest, room).sum())
            if rest.size == 0:
                continue
            K[rest] = pair_model._select_rest(s[rest], e[rest], L, room, fast)
        if counters is not None:
            counters.append((capped, demand))
        S = tm.complete(S | K, template_ids, n_templates)
        selected.append(int(K.sum()))
        kept.append(int(S.sum()))
        sets.append(S.copy())
    return pm.pack(S), selected, kept, sets


def covers(starts, ends, contig_ids, cap_arrays, kept_bits):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    for c, cap in enumerate(cap_arrays):
        sel = ids == c
        if cap.size == 0:
            continue
        need = np.minimum(pm.coverage(s[sel], e[sel], cap.size), cap)
        if not np.all(pm.coverage(s[sel & kept_bits], e[sel & kept_bits], cap.size) >= need):
            return False
    return True


def on_cap(starts, ends, contig_ids, template_ids, cap_arrays):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    hit = np.zeros(s.size, bool)
    for c, cap in enumerate(cap_arrays):
        before = np.concatenate([[0], np.cumsum(cap > 0)])     # positive positions below x
        sel = np.flatnonzero(ids == c)
        hit[sel] = before[e[sel] + 1] > before[s[sel]]
    return int(hit.sum()), int(np.unique(np.asarray(template_ids, np.int64)[hit]).size)


def targets_as_regions(target_offsets, target_starts, target_ends, contig_lengths, padding, cap):
    offs, r0, r1, caps = [0], [], [], []
    for c, L in enumerate(np.atleast_1d(contig_lengths).tolist()):
        inside = np.zeros(L + 1, bool)                          # (one spare entry: the run below ends before it)
        for k in range(int(target_offsets[c]), int(target_offsets[c + 1])):
            a, b = max(int(target_starts[k]) - padding, 0), int(target_ends[k]) + padding
            if a < L:
                inside[a:min(b, L - 1) + 1] = True
        edges = np.flatnonzero(np.diff(np.concatenate([[False], inside]).astype(np.int8)))
        for a, b in zip(edges[0::2].tolist(), edges[1::2].tolist()):
            r0.append(a); r1.append(b - 1); caps.append(cap)
        offs.append(len(r0))
    u = lambda x: np.asarray(x, np.uint32)
    return u(offs), u(r0), u(r1), u(caps)


def paired_targets(seed, L, M, depth, width, period, rl=150):
    """pair_model.overshoot's pairs (150-base mates 100 .. 499 apart, `depth` x M deep) as templates of two on one contig
    of L positions; regions of `width` positions every `period`, cap M inside, 0 elsewhere -> (starts, ends, contig_ids,
    template_ids, n_templates, contig_lengths, offs, r0, r1, caps)"""
    s, e, ids, lengths = pair_model.overshoot(seed, L, M, depth, rl)
    tids = (np.arange(s.size) // 2).astype(np.uint32)
    r0 = np.arange(0, L, period, dtype=np.int64)
    r1 = np.minimum(r0 + width - 1, L - 1)
    u = lambda x: np.asarray(x, np.uint32)
    return s, e, ids, tids, s.size // 2, lengths, u([0, r0.size]), u(r0), u(r1), np.full(r0.size, M, np.uint32)
