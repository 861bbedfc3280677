"""Times, on the device in one run: solve_tiers_device on cfg4's reads (8 contigs x 12.5 M reads, L = 10^6, M = 100) with
tiers 90 / 8 / 2 % (a) drawn uniformly, (b) the same with 2 % of every contig as stretches in which no read is of tier 0
(every tier-0 read that touches one is redrawn 8 : 2 among tiers 1 and 2); (c) the plain solve_by_contig_device at
M = 100 on the same reads.  Wall clock around blocking calls, alternating, medians of --reps after a warm-up call each;
then one profiled run of (a) and of (b) for the per-kernel times (qmcp_hip_set_profiling, a call of its own).
The rows and stats recorded are those of the second call of each shape (the first pays the arena's allocations).
--plain-only times (c) alone and touches nothing of the tiered entry: a copy of this script inside a checkout and build
of the parent commit gives the unchanged entry's time on the same box; --parent-json takes that run's output and records
its plain_ms and plain_solve_stats as plain_parent_build_* beside this run's.
    python lab/tiers_time.py [--pairs 6250000] [--reps 5] [--plain-only] [--parent-json FILE]
                             [--out profiles/tiers_time.json]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6_250_000, help="pairs per contig (cfg4: 6.25 M = 12.5 M reads)")
    ap.add_argument("--contigs", type=int, default=8)
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--parent-json", default=None, help="the output of a --plain-only run on a build of the parent commit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("genome-downsampler_amd")
    n_contigs, L, M = args.contigs, args.length, 100
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, args.pairs, L, seed=12345 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * args.pairs)
    rng = np.random.default_rng(4)
    perm = rng.permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    n = s.size
    uniform = rng.choice(3, size=n, p=[0.90, 0.08, 0.02]).astype(np.uint32)
    # (b): four stretches of L / 200 positions per contig, the same on every contig
    width = max(L // 200, 1)
    firsts = [L // 8, 3 * L // 8, 5 * L // 8, 7 * L // 8]
    inside = np.zeros(n, bool)
    for a in firsts:
        inside |= (s <= a + width - 1) & (e >= a)
    repeats = uniform.copy()
    hit = np.flatnonzero(inside & (uniform == 0))
    repeats[hit] = 1 + rng.choice(2, size=hit.size, p=[0.8, 0.2]).astype(np.uint32)
    lengths = np.full(n_contigs, L, dtype=np.uint32)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev)
    d_s, d_e, d_ids, d_uniform, d_repeats = up(s), up(e), up(ids), up(uniform), up(repeats)
    d_mask = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"commit": commit or "unknown", "library": "QMCP_HIP_LIB" if os.environ.get("QMCP_HIP_LIB") else "product",
           "reads": int(n), "contigs": n_contigs, "M": M, "tiers_percent": [90, 8, 2],
           "stretch_positions_per_contig": 4 * width, "reps": args.reps, "order": "shuffled"}
    with pkg.Solver(0) as solver:
        def tiers_of(column):
            return lambda: solver.solve_tiers_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), column.data_ptr(), n,
                                                     lengths, M, 3, d_mask.data_ptr())

        def plain():
            return solver.solve_by_contig_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, M,
                                                 d_mask.data_ptr())

        calls = [("plain", plain)]
        if not args.plain_only:
            calls = [("tiers_uniform", tiers_of(d_uniform)), ("tiers_repeats", tiers_of(d_repeats))] + calls
        for name, f in calls:   # the warm-up calls, and what a warmed call kept
            f()
            f()
            if name != "plain":
                out[name + "_rows"] = [r.as_dict() for r in solver.last_tier_rows]
                out[name + "_stats"] = solver.last_tiers_stats.as_dict()
            out[name + "_solve_stats"] = {k: v for k, v in solver.last_stats.as_dict().items()
                                          if k in ("n_reads", "n_kept", "path", "sort_passes", "ms_total")}
        times = {name: [] for name, _ in calls}
        for _ in range(args.reps):   # alternating
            for name, f in calls:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        for name, v in times.items():
            out[name + "_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        for name, f in calls:
            solver.set_profiling(True)
            f()
            out[name + "_kernel_times_ms"] = {k: [int(v[0]), round(v[1], 4)] for k, v in solver.kernel_times().items()}
            solver.set_profiling(False)
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.load(f)
        out["plain_parent_build_commit"] = parent["commit"]
        out["plain_parent_build_ms"] = parent["plain_ms"]
        out["plain_parent_build_solve_stats"] = parent["plain_solve_stats"]
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
