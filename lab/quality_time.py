"""qmcp_hip_solve_quality_device against qmcp_hip_solve_device on the same reads: cfg4 (8 contigs x 12.5 M reads, 1 M
positions each, reads of 150, M = 100) with MAPQ uniform on 0..60, the same reads with one quality (the early exit), and
cfg3's amplicon shape (30 M reads from primer to primer on 98 amplicons, M = 200: cells of ~3 x 10^5 reads).  Reports
the device times of the plain solve and of the quality pass (median over --reps) and, with the context's per-kernel
events on, the pass's kernels.

  python lab/quality_time.py [--reps 10] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("genome-downsampler_amd")


def cfg4():
    pairs, L = 6_250_000, 1_000_000
    ss, ee = zip(*[pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, seed=12345 + c) for c in range(8)])
    offs = np.arange(9, dtype=np.uint64) * np.uint64(2 * pairs)
    return np.concatenate(ss), np.concatenate(ee), offs, np.full(8, L, np.uint32), 100


def cfg3_shape():
    rng = np.random.default_rng(8)
    a0, a1 = importlib.import_module("genome-downsampler_amd.synthetic").amplicon_panel()
    n_pairs = 15_000_000
    amp = rng.integers(0, a0.size, size=n_pairs)
    s = np.empty(2 * n_pairs, np.uint32)
    e = np.empty(2 * n_pairs, np.uint32)
    s[0::2], e[0::2] = a0[amp] + 25, a0[amp] + 174
    s[1::2], e[1::2] = a1[amp] - 174, a1[amp] - 25
    return s, e, np.array([0, s.size], np.uint64), np.array([29_903], np.uint32), 200


def measure(solver, name, s, e, q, offs, lengths, M, reps):
    dev = lambda a: torch.from_numpy(a.astype(np.int32)).to("cuda:0")
    ds, de, dq = dev(s), dev(e), dev(q)
    dm = torch.zeros(pkg.mask_words(s.size), dtype=torch.int64, device="cuda:0")
    plain, qual, total = [], [], []
    for r in range(reps + 1):
        solver.solve_device(ds.data_ptr(), de.data_ptr(), s.size, lengths, M, dm.data_ptr(), contig_read_offsets=offs)
        p = solver.last_stats.ms_total
        qs = solver.solve_quality_device(ds.data_ptr(), de.data_ptr(), dq.data_ptr(), s.size, lengths, M,
                                         dm.data_ptr(), contig_read_offsets=offs)
        if r:                                     # (the first call of a shape grows the arena)
            plain.append(p)
            qual.append(qs.ms_quality)
            total.append(solver.last_stats.ms_total + qs.ms_quality)
    solver.set_profiling(True)
    solver.solve_quality_device(ds.data_ptr(), de.data_ptr(), dq.data_ptr(), s.size, lengths, M, dm.data_ptr(),
                                contig_read_offsets=offs)
    kernels = {k: round(v[1], 4) for k, v in solver.kernel_times().items()
               if "quality" in k or k.startswith("k_qc")}
    solver.set_profiling(False)
    row = dict(case=name, n_reads=int(s.size), plain_ms=round(statistics.median(plain), 4),
               quality_pass_ms=round(statistics.median(qual), 4), quality_total_ms=round(statistics.median(total), 4),
               stats=solver.last_quality_stats.as_dict(), kernels_ms_one_call_with_events=kernels)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    with pkg.Solver(0) as solver:
        s, e, offs, lengths, M = cfg4()
        q = np.random.default_rng(60).integers(0, 61, size=s.size).astype(np.uint32)
        rows.append(measure(solver, "cfg4, MAPQ 0..60", s, e, q, offs, lengths, M, args.reps))
        rows.append(measure(solver, "cfg4, one quality", s, e, np.full(s.size, 60, np.uint32), offs, lengths, M,
                            args.reps))
        del s, e, q
        s, e, offs, lengths, M = cfg3_shape()
        q = np.random.default_rng(61).integers(0, 61, size=s.size).astype(np.uint32)
        rows.append(measure(solver, "cfg3 amplicon shape, MAPQ 0..60", s, e, q, offs, lengths, M, args.reps))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
