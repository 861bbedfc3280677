"""Template-aware downsampling (qmcp_hip_solve_templates_*), restated for the tests: tests/pair_model.py's staged solve
with the completion by template id instead of the oracle's find_pairs.  Every row is a segment; template_ids[i] <
n_templates names its template; targets T_1 < ... < T_k = M.
  S_0 = {}; stage j: credit(p) = the depth of the placed segments of S_(j-1); cap(p) = max(0, T_j - credit(p)); K_j = the
  canonical selection under that cap ARRAY over the placed segments NOT in S_(j-1), alone, in input order, per contig;
  S_j = complete(S_(j-1) | K_j), complete(S) = the segments whose template has a segment in S.
  complete         np.bincount of the kept ids, gathered back
  staged           -> (mask of S_k, [|K_j|], [|S_j|], [S_j as bool arrays])
  template_counts  -> (size histogram for 1 .. 7 and >= 8 segments, templates in use, largest size)
  kept_templates   the number of templates with a segment in a set
  covers           pair_model.covers: the depth of a set is >= min(cov, T) on every contig
  whole_templates  a set holds every segment of each template it touches
  random_templates sizes 1 .. 6 and one large template, ids dealt through a random permutation"""
import numpy as np

import pair_model
import profile_model as pm

NO_CONTIG = pm.NO_CONTIG
default_stages = pair_model.default_stages
covers = pair_model.covers


def complete(bits, template_ids, n_templates):
    tids = np.asarray(template_ids, np.int64)
    if tids.size == 0:
        return np.zeros(0, bool)
    return np.bincount(tids[bits], minlength=int(n_templates))[tids] > 0


def staged(starts, ends, contig_ids, template_ids, n_templates, contig_lengths, M, stages=None, fast=True):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    lengths = np.atleast_1d(contig_lengths).tolist()
    stages = default_stages(M) if stages is None else [int(t) for t in stages]
    assert stages[-1] == int(M) and all(a < b for a, b in zip(stages, stages[1:])) and stages[0] >= 1
    n = s.size
    assert n == 0 or int(np.max(template_ids)) < int(n_templates)
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
            K[rest] = pair_model._select_rest(s[rest], e[rest], L, cap, fast)
        S = complete(S | K, template_ids, n_templates)
        selected.append(int(K.sum()))
        kept.append(int(S.sum()))
        sets.append(S.copy())
    return pm.pack(S), selected, kept, sets


def template_counts(template_ids, n_templates):
    sizes = np.bincount(np.asarray(template_ids, np.int64), minlength=int(n_templates))
    used = sizes[sizes > 0]
    hist = np.bincount(np.minimum(used, 8) - 1, minlength=8).tolist()
    return hist, int(used.size), int(used.max()) if used.size else 0


def kept_templates(bits, template_ids):
    return int(np.unique(np.asarray(template_ids, np.int64)[bits]).size)


def whole_templates(bits, template_ids, n_templates):
    return bool(np.array_equal(complete(bits, template_ids, n_templates), bits))


def random_templates(rng, n, n_templates=None, large=0, max_size=6):
    """template ids for n segments: sizes 1 .. max_size in random order and, when large > 0, one template of `large`
    segments; the segments of a template are scattered over the input by a random permutation, and the ids themselves
    are a random choice among n_templates (default: exactly as many as are used) -> (template_ids, n_templates)"""
    sizes = []
    left = n
    if large and left >= large:
        sizes.append(large)
        left -= large
    while left > 0:
        sz = min(left, int(rng.integers(1, max_size + 1)))
        sizes.append(sz)
        left -= sz
    used = len(sizes)
    n_templates = max(used, 1) if n_templates is None else int(n_templates)
    assert n_templates >= used
    names = rng.permutation(n_templates)[:used]
    if used and n_templates - 1 not in names:
        names[int(rng.integers(0, used))] = n_templates - 1          # the highest id is in use
    tids = np.repeat(names, sizes)[rng.permutation(n)] if n else np.zeros(0, np.int64)
    return tids.astype(np.uint32), n_templates
