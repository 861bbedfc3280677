"""qmcp_hip_solve_pairs_device on cfg4's shape as pairs (8 contigs of 1 M positions, 12.5 M reads of 150 each, every mate
starting 100 .. 499 positions behind its partner, pairs in shuffled order), M = 100 under the default stages: per-stage
device times and ms_pairs (qmcp_hip_pair_stats), the end-to-end time of the call, reads kept and mean kept depth -- and
next to them, in the same process, solve_by_contig_device + complete_pairs_device on the same input.

  python lab/pairs_profile.py [--reps 5] [--pairs 6250000] [--out profiles/pairs_cfg4.json]"""
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
    ap.add_argument("--pairs", type=int, default=6_250_000, help="pairs per contig")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_cfg4.json"))
    args = ap.parse_args()
    n_contigs, pairs, L, rl, M = 8, args.pairs, 1_000_000, 150, 100
    rng = np.random.default_rng(12345)
    s1 = rng.integers(0, L - rl - 500, size=n_contigs * pairs)
    s2 = s1 + rng.integers(100, 500, size=s1.size)
    order = rng.permutation(s1.size)                                  # pairs shuffled over the contigs, mates adjacent
    s = np.empty(2 * s1.size, np.uint32)
    s[0::2], s[1::2] = s1[order], s2[order]
    e = s + np.uint32(rl - 1)
    ids = np.repeat((order // pairs).astype(np.uint32), 2)
    n = s.size
    lengths = np.full(n_contigs, L, dtype=np.uint32)
    dev = torch.device("cuda", 0)
    d_s, d_e, d_ids = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids))
    d_mask = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev)
    d_plain = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    span = (e.astype(np.int64) - s + 1)

    def depth_of(mask_t):
        bits = pkg.mask_to_indices(mask_t.cpu().numpy().view(np.uint64), n).astype(np.int64)
        return int(bits.size), float(span[bits].sum()) / (n_contigs * L)

    out = {"reads": int(n), "contigs": n_contigs, "positions_per_contig": L, "read_length": rl, "max_coverage": M,
           "stages": "default", "reps": args.reps, "order": "pairs shuffled",
           "mean_depth_in": round(float(span.sum()) / (n_contigs * L), 3)}
    with pkg.Solver(0) as solver:
        def staged():
            return solver.solve_pairs_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, M,
                                             d_mask.data_ptr())

        def plain():
            st = solver.solve_by_contig_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, M,
                                               d_plain.data_ptr())
            solver.complete_pairs_device(d_plain.data_ptr(), n)
            torch.cuda.synchronize()
            return st

        staged()                                                      # the warm-up of both
        plain()
        t_staged, t_plain, per_stage, extra, plain_ms = [], [], [], [], []
        for _ in range(args.reps):                                    # alternating the two
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, ps = staged()
            t_staged.append((time.perf_counter() - t0) * 1e3)
            k = ps.n_stages
            per_stage.append([float(x) for x in ps.ms_stage[:k]])
            extra.append(float(ps.ms_pairs))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = plain()
            t_plain.append((time.perf_counter() - t0) * 1e3)
            plain_ms.append(float(st.ms_total))
        med = lambda v: round(statistics.median(v), 3)
        kept, depth = depth_of(d_mask)
        pkept, pdepth = depth_of(d_plain)
        out["targets"] = [int(x) for x in ps.target[:k]]
        out["n_selected"] = [int(x) for x in ps.n_selected[:k]]
        out["n_kept_after_completion"] = [int(x) for x in ps.n_kept[:k]]
        out["sweeps"] = [int(x) for x in ps.sweeps[:k]]
        out["staged_ms"] = {"median": med(t_staged), "min": round(min(t_staged), 3), "max": round(max(t_staged), 3)}
        out["staged_device_ms_per_stage"] = [med([r[j] for r in per_stage]) for j in range(k)]
        out["staged_device_ms_pairs"] = med(extra)
        out["staged_reads_kept"], out["staged_mean_kept_depth"] = kept, round(depth, 3)
        out["plain_ms"] = {"median": med(t_plain), "min": round(min(t_plain), 3), "max": round(max(t_plain), 3)}
        out["plain_device_ms_of_the_solve"] = med(plain_ms)
        out["plain_reads_kept"], out["plain_mean_kept_depth"] = pkept, round(pdepth, 3)
        solver.set_profiling(True)
        staged()
        out["staged_kernel_times_ms"] = {k_: round(v[1], 4) for k_, v in solver.kernel_times().items()
                                         if "pair" in k_ or "capped" in k_ or "k_bc_gather" in k_}
        solver.set_profiling(False)
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
