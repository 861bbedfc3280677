"""The CPU-model figures of DESIGN.md 4.26 (numpy only, no device): 900 reads of 80 - 120 bases on 3 000 positions,
M = 10, tiers drawn 85 / 10 / 5 %, and a 300-base "repeat" in which every read is of tier 1 or 2.  Means over --seeds of
  filter      the by-contig selection of the tier-0 reads alone (what min_mapq at ingest gives)
  blind       the by-contig selection of all reads, tiers ignored
  tiered      tests/tiers_model.tiered
-- reads kept, positions short of min(coverage of all reads, M), tier-1/2 reads kept outside the repeat (not touching
it), tier-2 reads kept.  With --tiny N: N instances of at most 12 reads a tier on 60 positions, every stage's selection
against the brute-force minimum for its need.
    python lab/tiers_model_numbers.py [--seeds 20] [--tiny 200]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import profile_model as pm  # noqa: E402
import tiers_model as tm    # noqa: E402

L, M, N, REPEAT = 3000, 10, 900, (1350, 1649)


def figures(seed):
    rng = np.random.default_rng(seed)
    s, e, ids, tiers = tm.instance(rng, [L], N, (80, 120), [85, 10, 5], repeats=[(0,) + REPEAT])
    s64, e64 = s.astype(np.int64), e.astype(np.int64)
    need = np.minimum(pm.coverage(s64, e64, L), M)
    outside = (e64 < REPEAT[0]) | (s64 > REPEAT[1])
    sets = {
        "filter": tm.tiered(s, e, ids, np.where(tiers == 0, 0, tm.NO_TIER), [L], M, 1, fast=True)[0],
        "blind": tm.tiered(s, e, ids, np.zeros(N, np.uint32), [L], M, 1, fast=True)[0],
        "tiered": tm.tiered(s, e, ids, tiers, [L], M, 3, fast=True)[0],
    }
    return {name: (int(k.sum()), int((pm.coverage(s64[k], e64[k], L) < need).sum()),
                   int((k & (tiers > 0) & outside).sum()), int((k & (tiers == 2)).sum())) for name, k in sets.items()}


def tiny(count):
    checked = 0
    for seed in range(count):
        rng = np.random.default_rng(10_000 + seed)
        n_tiers = int(rng.integers(1, 4))
        s, e, ids, tiers = tm.instance(rng, [60], int(rng.integers(1, 12)), (1, 30), rng.random(n_tiers) + 0.1)
        _, _, picks = tm.tiered(s, e, ids, tiers, [60], 3, n_tiers)
        before = np.zeros(s.size, bool)
        on = tm.members(ids, tiers, 1, n_tiers)
        everyone = [np.arange(s.size)]
        for t in range(n_tiers):
            (_, _, cap), = tm.needs(s, e, on[t], [60], before, 3, everyone)
            sel = on[t][0]
            if sel.size:
                assert picks[t][sel].sum() == pm.brute_minimum(s[sel].astype(np.int64), e[sel].astype(np.int64), cap), seed
                checked += 1
            before |= picks[t]
    return checked


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--tiny", type=int, default=200)
    args = ap.parse_args()
    rows = [figures(seed) for seed in range(args.seeds)]
    print("selection\treads kept\tpositions short\ttier-1/2 kept outside the repeat\ttier-2 kept")
    for name in ("filter", "blind", "tiered"):
        print(name + "\t" + "\t".join(f"{np.mean([r[name][k] for r in rows]):.1f}" for k in range(4)))
    if args.tiny:
        print(f"{tiny(args.tiny)} stage selections on {args.tiny} tiny instances have the brute-force minimum size")


if __name__ == "__main__":
    main()
