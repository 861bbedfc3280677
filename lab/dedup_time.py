"""Times, on the device in one run, solve_dedup_device on cfg4's reads (8 contigs x 12.5 M reads, L = 10^6, M = 100,
shuffled) with strand tags, MAPQ 0..60 and --dup of the reads replaced by copies of other reads: read mode, pair mode,
and the plain solve_by_contig_device for scale.  Wall clock around blocking calls, alternating, median of --reps, and
ms_dedup (the device time of everything except the inner solve); then one profiled run of each mode for the per-kernel
times, and the device's copy rate (a 400 MB device-to-device copy) for the byte model of DESIGN 4.11.
    python lab/dedup_time.py [--pairs 6250000] [--reps 5] [--dup 0.2] [--out profiles/dedup_time.json]"""
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
    ap.add_argument("--dup", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("genome-downsampler_amd")
    n_contigs, L, M = args.contigs, args.length, 100
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, args.pairs, L, seed=12345 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * args.pairs)
    rng = np.random.default_rng(4)
    n = s.size
    tags = rng.integers(0, 2, size=n).astype(np.uint32)
    src = np.arange(n)
    copies = rng.random(n) < args.dup
    src[copies] = rng.integers(0, n, size=int(copies.sum()))
    src = src[rng.permutation(n)]
    s, e, ids, tags = s[src], e[src], ids[src], tags[src]
    q = rng.integers(0, 61, size=n).astype(np.uint32)
    lengths = np.full(n_contigs, L, dtype=np.uint32)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev)
    d_s, d_e, d_ids, d_t, d_q = up(s), up(e), up(ids), up(tags), up(q)
    words = pkg.mask_words(n)
    d_mask = torch.zeros(words, dtype=torch.int64, device=dev)
    d_dup = torch.zeros(words, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"commit": commit or "unknown", "reads": int(n), "contigs": n_contigs, "M": M, "reps": args.reps,
           "order": "shuffled", "dup_share_asked": args.dup}
    # the copy rate: 400 MB read + 400 MB written
    a = torch.empty(100_000_000, dtype=torch.int32, device=dev)
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        b.copy_(a)
    torch.cuda.synchronize()
    out["copy_GBps"] = round(5 * 2 * a.numel() * 4 / (time.perf_counter() - t0) / 1e9, 1)
    del a, b
    with pkg.Solver(0) as solver:
        def dedup(pairs):
            return solver.solve_dedup_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, M,
                                             d_mask.data_ptr(), d_tags=d_t.data_ptr(), d_qualities=d_q.data_ptr(),
                                             pairs=pairs, d_dup_mask=d_dup.data_ptr(), hist_bins=64)

        def plain():
            return solver.solve_by_contig_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, M,
                                                 d_mask.data_ptr())

        modes = (("read", lambda: dedup(False)), ("pair", lambda: dedup(True)), ("plain", plain))
        for name, f in modes:
            f()
            if name != "plain":
                out[name + "_stats"] = solver.last_dedup_stats.as_dict()
        times = {name: [] for name, _ in modes}
        ms_dedup = {"read": [], "pair": []}
        for _ in range(args.reps):   # alternating the three
            for name, f in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
                if name in ms_dedup:
                    ms_dedup[name].append(solver.last_dedup_stats.ms_dedup)
        for name, v in times.items():
            out[name + "_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        for name, v in ms_dedup.items():
            out[name + "_ms_dedup"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        for name, f in modes[:2]:
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
