"""What qmcp_hip_solve_budget_device costs on cfg4's reads (bench.py: 8 contigs x 12.5 M reads of 150 bases on 10^6
positions each) shuffled over their contigs, max_coverage = 1 000, budgets at 1 %, 5 % and 50 % of the reads.
Per budget, alternating in one process, wall time of the blocking device call, medians over --reps after a warm-up:
  budget      solve_budget_device: one grouping, the depth histogram, the probes budget_plan.h picks
  bisection   the only route without the entry: plain bisection over 1 .. top with solve_by_contig_device per trial (it
              regroups the reads every time) and the count by torch; the largest depth is handed to it for nothing
and, from one more profiled call, ms_budget per kernel, ms_solves per probe and the number of probes.

  python lab/budget_time.py [--reps 5] [--scale 1.0] [--out profiles/budget_time.json]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("genome-downsampler_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of cfg4's reads per contig")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "budget_time.json"))
    args = ap.parse_args()
    n_contigs, pairs, L, rl, max_coverage = 8, int(6_250_000 * args.scale), 1_000_000, 150, 1000
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, rl, seed=12345 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    del ss, ee
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
    perm = np.random.default_rng(4).permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    del perm
    n = s.size
    lengths = np.full(n_contigs, L, np.uint32)
    dev = torch.device("cuda", 0)
    ds, de, di = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids))
    masks = [torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev) for _ in range(3)]
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    out = {"reads": n, "contigs": n_contigs, "positions": int(n_contigs * L), "max_coverage": max_coverage,
           "reps": args.reps, "budgets": {}}

    def popcount(mask):
        return int(torch.from_numpy(np.unpackbits(mask.cpu().numpy().view(np.uint8))).sum())

    def count_on_device(mask):      # what a caller without the entry would write: one pass over the mask words
        m = mask
        m = (m & 0x5555555555555555) + ((m >> 1) & 0x5555555555555555)
        m = (m & 0x3333333333333333) + ((m >> 2) & 0x3333333333333333)
        m = (m & 0x0F0F0F0F0F0F0F0F) + ((m >> 4) & 0x0F0F0F0F0F0F0F0F)
        return int(m.view(torch.uint8).sum(dtype=torch.int64))

    with pkg.Solver(0) as solver:
        state = {}

        def budget_call(budget):
            M, bs = solver.solve_budget_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, max_coverage,
                                               masks[0].data_ptr(), budget_reads=budget, stream=stream)
            torch.cuda.synchronize()
            state["budget"] = (M, bs)

        def bisection(budget):
            lo, hi, best, trial, trials = 0, state["top"] + 1, 1, 2, 0
            masks[best].zero_()
            while hi - lo > 1:
                mid = (lo + hi) // 2
                torch.cuda.synchronize()
                solver.solve_by_contig_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, mid,
                                              masks[trial].data_ptr(), stream=stream)
                trials += 1
                if count_on_device(masks[trial]) <= budget:
                    lo, best, trial = mid, trial, best
                else:
                    hi = mid
            torch.cuda.synchronize()
            state["bisection"] = (lo, best, trials)

        for share in (0.01, 0.05, 0.5):
            budget = int(n * share)
            budget_call(budget)                                                   # warm-up: arena growth
            state["top"] = int(state["budget"][1].top)
            bisection(budget)
            (M, bs), (M_b, best, trials) = state["budget"], state["bisection"]
            same = M == M_b and bool(torch.equal(masks[0], masks[best]))
            wall = {"budget": [], "bisection": []}
            for _ in range(args.reps):
                for name, call in (("budget", budget_call), ("bisection", bisection)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call(budget)
                    wall[name].append((time.perf_counter() - t0) * 1e3)
            solver.set_profiling(True)
            budget_call(budget)
            times = solver.kernel_times()
            solver.set_profiling(False)
            bs = state["budget"][1]
            part = lambda key: round(sum(v[1] for k, v in times.items() if k.startswith(key)), 4)
            out["budgets"][f"{share:g}"] = {
                "budget_reads": budget, "coverage": M, "same_coverage_and_mask_as_bisection": same,
                "budget_ms_median": round(statistics.median(wall["budget"]), 3),
                "budget_ms_runs": [round(x, 3) for x in wall["budget"]],
                "bisection_ms_median": round(statistics.median(wall["bisection"]), 3),
                "bisection_ms_runs": [round(x, 3) for x in wall["bisection"]], "bisection_trials": trials,
                "probes": int(bs.probes), "ms_budget": round(float(bs.ms_budget), 4),
                "k_budget_tally_ms": part("k_budget_tally"), "k_budget_curve_ms": part("k_budget_curve"),
                "k_budget_finish_ms": part("k_budget_finish"), "ms_solves": round(float(bs.ms_solves), 3),
                "ms_solves_per_probe": round(float(bs.ms_solves) / max(int(bs.probes), 1), 3),
                "grouping_ms": part("k_radix") + part("scan_radix") + part("k_bc_keys") + part("k_bc_bounds"),
                "kernels_ms": {k: round(v[1], 4) for k, v in sorted(times.items())},
                "kept": popcount(masks[0]), "stats": {k: v for k, v in bs.as_dict().items() if not k.startswith("ms_")},
            }
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
