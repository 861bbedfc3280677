"""What qmcp_hip_solve_ceiling_device costs on the shape of
tests/test_gpu_profile.py::test_capped_route_costs_little_more_than_the_plain_mixed_route: 2^22 reads of spans 100 and 150
on 8 contigs of 500 000 positions, shuffled, M = 60, near_uniform = speculation = cut_points = -1 (one chain per contig).
Two calls on the same reads and the same table (every cap M), alternating, wall time of the blocking device call, medians
over --reps after a warm-up:
  ceiling   solve_ceiling_device: the walk selects the cov - M reads per position that are DROPPED
  profile   solve_profile_device: the walk selects the M reads per position that are kept
and ms_ceiling with its parts (need, depth events + scan, check, finish) from the kernel times of one more call each.
The two times differ by design; the record is there so that the next change has a parent number to compare with.

  python lab/ceiling_time.py [--reps 5] [--out profiles/ceiling_time.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ceiling_time.json"))
    args = ap.parse_args()
    n_contigs, L, M = 8, 500_000, 60
    n = 1 << 22
    rng = np.random.default_rng(79)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), n // n_contigs)
    span = np.where(rng.random(n) < 0.5, 100, 150).astype(np.int64)
    s = (rng.random(n) * (L - span + 1)).astype(np.int64)
    e, s = (s + span - 1).astype(np.uint32), s.astype(np.uint32)
    perm = rng.permutation(n)
    s, e, ids = s[perm], e[perm], ids[perm]
    lengths = np.full(n_contigs, L, np.uint32)
    starts_1 = np.arange(0, L, 1000, dtype=np.uint32)
    offs = (np.arange(n_contigs + 1) * starts_1.size).astype(np.uint32)
    r0 = np.tile(starts_1, n_contigs)
    r1 = r0 + 899
    caps = np.full(r0.size, M, np.uint32)
    dev = torch.device("cuda", 0)
    ds, de, di = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids))
    d_masks = {k: torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev) for k in ("ceiling", "profile")}
    torch.cuda.synchronize()
    out = {"reads": n, "contigs": n_contigs, "positions": int(n_contigs * L), "M": M, "regions": int(r0.size),
           "reps": args.reps, "options": {"near_uniform": -1, "speculation": -1, "cut_points": -1}}
    with pkg.Solver(0) as solver, solver.options(near_uniform=-1, speculation=-1, cut_points=-1):
        calls = {
            "ceiling": lambda: solver.solve_ceiling_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M,
                                                           d_masks["ceiling"].data_ptr(), offs, r0, r1, caps),
            "profile": lambda: solver.solve_profile_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M,
                                                           d_masks["profile"].data_ptr(), offs, r0, r1, caps),
        }
        for call in calls.values():
            call()                                                              # warm-up: arena growth
        wall = {k: [] for k in calls}
        ms_ceiling = []
        for _ in range(args.reps):
            for name, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stats = call()
                torch.cuda.synchronize()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                if name == "ceiling":
                    ms_ceiling.append(float(stats.ms_ceiling))
        for name, call in calls.items():
            solver.set_profiling(True)
            stats = call()
            times = solver.kernel_times()
            solver.set_profiling(False)
            row = {"ms_median": round(statistics.median(wall[name]), 3), "ms_runs": [round(x, 3) for x in wall[name]],
                   "sweep_ms": round(sum(v[1] for k, v in times.items() if k.startswith("k_sweep")), 3),
                   "kept": int(np.unpackbits(d_masks[name].cpu().numpy().view(np.uint8)).sum())}
            if name == "ceiling":
                part = lambda key: round(sum(v[1] for k, v in times.items() if key in k), 4)
                row.update(ms_ceiling_median=round(statistics.median(ms_ceiling), 4), k_ceiling_need_ms=part("k_ceiling_need"),
                           depth_events_and_scan_ms=part("scan(ceiling)"), k_ceiling_check_ms=part("k_ceiling_check"),
                           k_ceiling_finish_ms=part("k_ceiling_finish"),
                           stats={k: v for k, v in stats.as_dict().items() if k != "ms_ceiling"})
            else:
                row.update(k_profile_need_ms=round(times["k_profile_need"][1], 4))
            out[name] = row
    out["ratio_ceiling_over_profile"] = round(out["ceiling"]["ms_median"] / out["profile"]["ms_median"], 4)
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
