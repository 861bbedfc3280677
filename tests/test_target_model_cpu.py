"""The reduction behind qmcp_hip_solve_targets_*: the unchanged oracle, run on the reads projected by
tests/target_model.py, gives a kept set that -- mapped back -- satisfies cov_kept(p) >= min(cov(p), M) at every target
position of the ORIGINAL axis and has the brute-force minimum size over all subsets of the reads."""
import itertools

import numpy as np

import target_model as tm


def _cover(s, e, L, sel):
    cov = np.zeros(L, np.int64)
    for i in sel:
        cov[s[i]:e[i] + 1] += 1
    return cov


def _brute_force_minimum(s, e, L, M, tset):
    n = len(s)
    need = np.minimum(_cover(s, e, L, range(n)), M)[tset]
    for k in range(n + 1):
        for sub in itertools.combinations(range(n), k):
            if np.all(_cover(s, e, L, sub)[tset] >= need):
                return k
    raise AssertionError("the whole set always satisfies the constraint")


def test_projected_oracle_solve_is_valid_and_minimum_on_the_original_axis(oracle):
    rng = np.random.default_rng(343)
    with_off_target = with_clipped = 0
    for trial in range(320):
        L = int(rng.integers(8, 40))
        n = int(rng.integers(1, 13))
        M = int(rng.integers(1, 4))
        span = rng.integers(1, min(L, 12) + 1, size=n)
        s = (rng.random(n) * (L - span + 1)).astype(np.int64)
        e = s + span - 1
        offs, t0, t1 = tm.random_regions(rng, [L], max_regions=3, max_len=8, outside=0.05, empty=0.05)
        padding = int(rng.choice([0, 0, 1]))
        ids = np.zeros(n, np.uint32)
        mask, on = tm.expected_mask(oracle, s, e, ids, [L], offs, t0, t1, M, padding=padding)
        kept = np.flatnonzero(np.unpackbits(mask.view(np.uint8), bitorder="little")[:n])
        tset = tm.target_sets([L], offs, t0, t1, padding)[0]
        assert set(kept.tolist()) <= set(np.flatnonzero(on).tolist()), trial
        need = np.minimum(_cover(s, e, L, range(n)), M)
        got = _cover(s, e, L, kept)
        assert np.all(got[tset] >= need[tset]), (trial, s, e, t0, t1)
        assert kept.size == _brute_force_minimum(s, e, L, M, tset), (trial, s, e, t0, t1, M)
        with_off_target += int((~on).any())
        _, ps, pe, _ = tm.project(s, e, ids, [L], offs, t0, t1, padding)
        with_clipped += int(np.any(on & (pe - ps < e - s)))
    assert with_off_target > 50 and with_clipped > 50   # the instances do exercise both
