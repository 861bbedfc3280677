"""The experiment behind amplicon-aware downsampling, on the CPU oracle (no device): what today's contig-wide selection,
the primer-clipped pooled solve and the primer-clipped per-amplicon solve keep on a fragmented amplicon panel, and where
each of them leaves the primer-trimmed depth short of min(primer-trimmed coverage, M).

    python lab/amplicon_clip_experiment.py [--seeds 1 2 3] [--coverage 50]

The panel is tests/amplicon_clip_model.py's fragmented_panel: one 3 000-base contig, 9 amplicons of 400 bases every 300,
25-base primers, log-normal yields, single reads of 60 - 200 bases inside their amplicon, 40 % flush with one of its
edges.  Prints one JSON line per seed; DESIGN.md 4.25 quotes them."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import amplicon_clip_model as am  # noqa: E402
import multi_reference as mr  # noqa: E402
import oracle_py as oracle  # noqa: E402


def run(seed, M):
    s, e, ids, lengths, offs, a0, a1, i0, i1 = am.fragmented_panel(seed)
    tables = (offs, a0, a1, i0, i1)
    short = lambda keep: am.trimmed_shortfall(s, e, ids, lengths, *tables, M, keep, single_end=True)
    today = am.unpack(mr.oracle_by_contig(oracle, s, e, ids, lengths, M), s.size)
    pooled, _, _, st = am.solve(oracle, s, e, ids, lengths, M, *tables, single_end=True)
    per, _, rows, _ = am.solve(oracle, s, e, ids, lengths, M, *tables, single_end=True, per_amplicon=True)
    covered = np.zeros(int(lengths[0]), bool)   # the contig positions some insert covers: what the short positions are of
    for lo, hi in zip(i0.tolist(), i1.tolist()):
        covered[lo:hi + 1] = True
    out = dict(seed=seed, reads=int(s.size), M=M, positions_covered_by_inserts=int(covered.sum()),
               reads_shortened=st["reads_shortened"])
    for name, keep in (("contig_wide", today), ("clipped_pooled", pooled), ("clipped_per_amplicon", per)):
        positions, worst = short(keep)
        out[name] = dict(kept=int(keep.sum()), short_positions=positions, worst_shortfall=worst)
    out["clipped_per_amplicon"]["short_positions_on_own_insert"] = sum(r[12] for r in rows)
    # the deepest kept primer-trimmed depth, in units of M: where two inserts overlap the per-amplicon mode stacks them
    ac = am.assign_and_clip(s, e, ids, *tables, single_end=True)
    for name, keep in (("clipped_pooled", pooled), ("clipped_per_amplicon", per)):
        depth = am.dm.coverages(ac["cs"], ac["ce"], ids, lengths, am.pack(keep))[0][1]
        out[name]["max_kept_depth_over_M"] = round(float(depth.max()) / M, 2)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--coverage", type=int, default=50)
    args = ap.parse_args()
    for seed in args.seeds:
        print(json.dumps(run(seed, args.coverage)))
