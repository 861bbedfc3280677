"""qmcp_hip_solve_ladder_device on cfg4's reads (8 contigs x 12.5 M reads, 1 M positions each, reads of 150) in shuffled
order, coverages [100, 50, 25, 10]: the ladder's per-level device times (qmcp_hip_ladder_stats) and its end-to-end time,
and next to them, in the same process, the only route without the ladder -- solve_by_contig_device at each coverage, on
columns compacted with torch between the calls, which regroups the reads at every level.

  python lab/ladder_profile.py [--reps 5] [--out profiles/ladder_cfg4.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ladder_cfg4.json"))
    args = ap.parse_args()
    n_contigs, pairs, L, rl, cov = 8, 6_250_000, 1_000_000, 150, [100, 50, 25, 10]
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, rl, seed=12345 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
    perm = np.random.default_rng(4).permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    n = s.size
    lengths = np.full(n_contigs, L, dtype=np.uint32)
    dev = torch.device("cuda", 0)
    d_s, d_e, d_ids = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids))
    d_levels = torch.zeros(n, dtype=torch.uint8, device=dev)
    shifts = torch.arange(64, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    out = {"reads": int(n), "contigs": n_contigs, "coverages": cov, "reps": args.reps, "order": "shuffled"}
    with pkg.Solver(0) as solver:
        def ladder():
            return solver.solve_ladder_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, cov,
                                              d_levels.data_ptr())

        def chain():
            cols, alive = (d_s, d_e, d_ids), torch.arange(n, device=dev)
            levels = torch.zeros(n, dtype=torch.uint8, device=dev)
            device_ms = []
            for M in cov:
                m = cols[0].numel()
                mask = torch.zeros(pkg.mask_words(m), dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                st = solver.solve_by_contig_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), m,
                                                   lengths, M, mask.data_ptr())
                device_ms.append(float(st.ms_total))
                bits = ((mask.unsqueeze(1) >> shifts) & 1).flatten()[:m].bool()
                cols = tuple(c[bits].contiguous() for c in cols)
                alive = alive[bits]
                levels[alive] += 1
            torch.cuda.synchronize()
            return levels, device_ms

        want, _ = chain()
        ladder()
        out["ladder_equals_chain"] = bool(torch.equal(d_levels, want))
        t_ladder, t_chain, per_level, extra, chain_solves = [], [], [], [], []
        for _ in range(args.reps):   # alternating the two
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ls = ladder()
            t_ladder.append((time.perf_counter() - t0) * 1e3)
            per_level.append([float(x) for x in ls.ms_level[:len(cov)]])
            extra.append(float(ls.ms_ladder))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, ms = chain()
            t_chain.append((time.perf_counter() - t0) * 1e3)
            chain_solves.append(ms)
        med = lambda v: round(statistics.median(v), 3)
        out["n_kept"] = [int(x) for x in ls.n_kept[:len(cov)]]
        out["ladder_ms"] = {"median": med(t_ladder), "min": round(min(t_ladder), 3), "max": round(max(t_ladder), 3)}
        out["ladder_device_ms_per_level"] = [med([r[j] for r in per_level]) for j in range(len(cov))]
        out["ladder_device_ms_around_the_solves"] = med(extra)
        out["chain_ms"] = {"median": med(t_chain), "min": round(min(t_chain), 3), "max": round(max(t_chain), 3)}
        out["chain_device_ms_of_the_batches_per_level"] = [med([r[j] for r in chain_solves]) for j in range(len(cov))]
        solver.set_profiling(True)
        ladder()
        out["ladder_kernel_times_ms"] = {k: round(v[1], 4) for k, v in solver.kernel_times().items() if "ladder" in k}
        solver.set_profiling(False)
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
