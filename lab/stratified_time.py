"""Times, on the device in one run: (a) solve_stratified_device on cfg4's reads (8 contigs x 12.5 M reads, L = 10^6,
M = 100) with a random strand column and caps (50, 50); (b) what a caller did before -- two solve_by_contig_device
calls at 50 on columns split by strand beforehand (the split is not timed); (c) the plain solve_by_contig_device at
M = 100, for scale.  Wall clock around blocking calls, alternating, median of --reps; then one profiled run of (a) and
of (b) for the per-kernel times.
    python lab/stratified_time.py [--pairs 6250000] [--reps 5] [--out profiles/stratified_time.json]"""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("genome-downsampler_amd")
    n_contigs, L, M, caps = args.contigs, args.length, 100, [50, 50]
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, args.pairs, L, seed=12345 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * args.pairs)
    rng = np.random.default_rng(4)
    perm = rng.permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    strand = rng.integers(0, 2, size=s.size).astype(np.uint32)
    n = s.size
    lengths = np.full(n_contigs, L, dtype=np.uint32)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev)
    d_s, d_e, d_ids, d_strand = up(s), up(e), up(ids), up(strand)
    split = []
    for k in (0, 1):
        on = np.flatnonzero(strand == k)
        split.append((up(s[on]), up(e[on]), up(ids[on]), on.size, torch.from_numpy(on).to(dev)))
    words = pkg.mask_words(n)
    d_mask = torch.zeros(words, dtype=torch.int64, device=dev)
    d_half = [torch.zeros(pkg.mask_words(p[3]), dtype=torch.int64, device=dev) for p in split]
    shifts = torch.arange(64, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"commit": commit or "unknown", "reads": int(n), "contigs": n_contigs, "M": M, "caps": caps, "reps": args.reps,
           "order": "shuffled"}
    with pkg.Solver(0) as solver:
        def stratified():
            return solver.solve_stratified_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), d_strand.data_ptr(), n,
                                                  lengths, caps, d_mask.data_ptr())

        def two_calls():
            for p, m, cap in zip(split, d_half, caps):
                solver.solve_by_contig_device(p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), p[3], lengths, cap,
                                              m.data_ptr())

        def plain():
            return solver.solve_by_contig_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, M,
                                                 d_mask.data_ptr())

        two_calls()
        want = torch.zeros(n, dtype=torch.bool, device=dev)
        for p, m in zip(split, d_half):
            want[p[4][((m.unsqueeze(1) >> shifts) & 1).flatten()[:p[3]].bool()]] = True
        stratified()
        got = ((d_mask.unsqueeze(1) >> shifts) & 1).flatten()[:n].bool()
        out["stratified_equals_two_calls"] = bool(torch.equal(got, want))
        out["rows"] = [r.as_dict() for r in solver.last_stratum_rows]
        plain()
        times = {"stratified": [], "two_calls": [], "plain": []}
        for _ in range(args.reps):   # alternating the three
            for name, f in (("stratified", stratified), ("two_calls", two_calls), ("plain", plain)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        for name, v in times.items():
            out[name + "_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        for name, f in (("stratified", stratified), ("two_calls", two_calls)):
            solver.set_profiling(True)
            f()
            out[name + "_kernel_times_ms"] = {k: [int(v[0]), round(v[1], 4)] for k, v in solver.kernel_times().items()}
            solver.set_profiling(False)
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
