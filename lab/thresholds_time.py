"""What qmcp_hip_solve_thresholds_device costs on cfg4's reads (bench.py: 8 contigs x 12.5 M reads of 150 bases on 10^6
positions each) shuffled over their contigs, ranges 1 .. 30 and 1 .. 100.
Per range, alternating in one process, wall time of the blocking device call, medians over --reps after a warm-up:
  thresholds  solve_thresholds_device: one grouping, one whole solve and one k_thresholds_step per coverage
  loop        the only route without the entry: solve_by_contig_device per coverage (it regroups the reads every time)
              and a torch where / minimum that accumulates the smallest keeping coverage
and, from one more profiled call, ms_thresholds per kernel beside ms_solves.

  python lab/thresholds_time.py [--reps 5] [--scale 1.0] [--out profiles/thresholds_time.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thresholds_time.json"))
    args = ap.parse_args()
    n_contigs, pairs, L, rl = 8, int(6_250_000 * args.scale), 1_000_000, 150
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
    d_thr = torch.zeros(n, dtype=torch.int16, device=dev)
    mask = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev)
    shifts = torch.arange(64, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    out = {"reads": n, "contigs": n_contigs, "positions": int(n_contigs * L), "reps": args.reps, "ranges": {}}

    with pkg.Solver(0) as solver:
        state = {}

        def thresholds_call(lo, hi):
            state["call"] = solver.solve_thresholds_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, hi,
                                                           d_thr.data_ptr(), coverage_lo=lo, stream=stream)
            torch.cuda.synchronize()

        def loop(lo, hi):
            acc = torch.full((n,), pkg.THRESHOLD_NEVER, dtype=torch.int32, device=dev)
            for M in range(lo, hi + 1):
                torch.cuda.synchronize()
                solver.solve_by_contig_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M, mask.data_ptr(),
                                              stream=stream)
                kept = ((mask.unsqueeze(1) >> shifts) & 1).reshape(-1)[:n].bool()
                acc = torch.minimum(acc, torch.where(kept, M, pkg.THRESHOLD_NEVER).to(torch.int32))
            torch.cuda.synchronize()
            state["loop"] = acc

        for lo, hi in ((1, 30), (1, 100)):
            thresholds_call(lo, hi)                                               # warm-up: arena growth
            loop(lo, hi)
            same = bool(torch.equal(d_thr.to(torch.int32) & 0xFFFF, state["loop"]))
            wall = {"thresholds": [], "loop": []}
            for _ in range(args.reps):
                for name, call in (("thresholds", thresholds_call), ("loop", loop)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call(lo, hi)
                    wall[name].append((time.perf_counter() - t0) * 1e3)
            solver.set_profiling(True)
            thresholds_call(lo, hi)
            times = solver.kernel_times()
            solver.set_profiling(False)
            ts = state["call"]
            part = lambda key: round(sum(v[1] for k, v in times.items() if k.startswith(key)), 4)
            out["ranges"][f"{lo}..{hi}"] = {
                "same_array_as_the_loop": same,
                "thresholds_ms_median": round(statistics.median(wall["thresholds"]), 3),
                "thresholds_ms_runs": [round(x, 3) for x in wall["thresholds"]],
                "loop_ms_median": round(statistics.median(wall["loop"]), 3),
                "loop_ms_runs": [round(x, 3) for x in wall["loop"]],
                "solves": int(ts.solves), "ms_thresholds": round(float(ts.ms_thresholds), 4),
                "k_thresholds_step_ms": part("k_thresholds_step"), "k_thresholds_finish_ms": part("k_thresholds_finish"),
                "k_thresholds_counts_ms": part("k_thresholds_counts"), "ms_solves": round(float(ts.ms_solves), 3),
                "ms_solves_per_solve": round(float(ts.ms_solves) / max(int(ts.solves), 1), 3),
                "grouping_ms": part("k_radix") + part("scan_radix") + part("k_bc_keys") + part("k_bc_bounds"),
                "stats": {k: v for k, v in ts.as_dict().items() if not k.startswith("ms_")},
            }
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
