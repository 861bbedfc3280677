"""qmcp_hip_solve_amplicons_host next to qmcp_hip_filter_solve_by_contig_host on cfg3's shape at full size
(synthetic.amplicon_panel, synthetic.amplicon_reads): ONE genome of 29 903 bases, 98 tiled amplicons of 400 bases, 15 M
pairs (30 M reads), a tenth of the pairs straddling two amplicons, M = 200, mates completed.  Pooled mode is then one
chain over a range that holds every read, per-amplicon mode 98 short independent problems.  In one process, alternating, after a warm-up of each:
  filter_solve_by_contig     the comparison point (its code is what it was before this entry existed)
  amplicons_no_inserts       the new entry with inserts NULL, pooled, no labels, no rows: the same mask, so the difference
                             is the price of the assign kernel's extra columns
  amplicons_labels           ... with the labels copied back
  amplicons_pooled           25-base primers clipped, pooled
  amplicons_per_amplicon     25-base primers clipped, one coverage problem per amplicon
  amplicons_pooled_rows      ... pooled, with the per-amplicon rows
Reports the host-entry time of each (host clock, H2D and D2H included), ms_assign / ms_report of the entry's own stats,
the per-kernel device times of one call of each, and for k_amplicon_clip the bytes it must move over its time next to the
copy rate of the part.

  timeout -k 10 600 python lab/amplicon_clip_time.py [--pairs 15000000] [--reps 5] [--out profiles/amplicon_clip_time.json]

Run it under `timeout`, as above: one process on one MI355X, a few minutes at full size."""
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
pkg = importlib.import_module("genome-downsampler_amd")
synthetic = importlib.import_module("genome-downsampler_amd.synthetic")

COPY_TBPS = 6.29   # the measured float4 copy rate of an MI355X
M = 200
PRIMER = 25


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--pairs", type=int, default=15_000_000)
    ap_.add_argument("--reps", type=int, default=5)
    ap_.add_argument("--out", default=None)
    args = ap_.parse_args()
    n_pairs = args.pairs
    s, e, a0, a1, _ = synthetic.amplicon_reads(n_pairs)
    lengths = np.array([29_903], np.uint32)
    offs = np.array([0, a0.size], np.uint32)
    i0, i1 = a0 + PRIMER, a1 - PRIMER
    n = s.size
    ids = np.zeros(n, np.uint32)
    print(f"{n} reads drawn", file=sys.stderr, flush=True)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"commit": commit or "unknown", "reads": int(n), "references": 1, "genome": int(lengths.sum()),
           "amplicons": int(a0.size), "M": M, "primer": PRIMER, "reps": args.reps}
    tab = dict(amp_offsets=offs, amp_starts=a0, amp_ends=a1)
    with pkg.Solver(0) as solver:
        def entry(**kw):
            return lambda: solver.solve_amplicons(s, e, ids, lengths, M, offs, a0, a1, complete_pairs=True, **kw)[0]

        runs = {
            "filter_solve_by_contig": lambda: solver.filter_solve_by_contig(s, e, ids, lengths, M, complete_pairs=True,
                                                                            **tab)[0],
            "amplicons_no_inserts": entry(labels=False, rows=False),
            "amplicons_labels": entry(labels=True, rows=False),
            "amplicons_pooled": entry(insert_starts=i0, insert_ends=i1, labels=False, rows=False),
            "amplicons_per_amplicon": entry(insert_starts=i0, insert_ends=i1, per_amplicon=True, labels=False, rows=False),
            "amplicons_pooled_rows": entry(insert_starts=i0, insert_ends=i1, labels=False, rows=True),
        }
        masks = {}
        for name, fn in runs.items():   # warm-up: code objects, arena
            masks[name] = fn()
            print(f"warm-up of {name} done", file=sys.stderr, flush=True)
        out["same_mask_without_inserts"] = bool(np.array_equal(masks["filter_solve_by_contig"],
                                                               masks["amplicons_no_inserts"]))
        for name, mask in masks.items():
            out["kept_" + name] = int(np.unpackbits(mask.view(np.uint8)).sum())
        out["assign_stats_pooled"] = {k: v for k, v in solver.last_amplicons_stats.as_dict().items() if not k.startswith("ms_")}
        times = {name: [] for name in runs}
        assign, report = {name: [] for name in runs}, []
        for rep in range(args.reps):   # alternating
            print(f"repetition {rep}", file=sys.stderr, flush=True)
            for name, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
                if name != "filter_solve_by_contig":
                    assign[name].append(solver.last_amplicons_stats.ms_assign)
                if name == "amplicons_pooled_rows":
                    report.append(solver.last_amplicons_stats.ms_report)
        med = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        for name, v in times.items():
            out[name + "_host_entry_ms"] = med(v)
            if assign[name]:
                out[name + "_ms_assign"] = med(assign[name])
        out["rows_ms_report"] = med(report)
        for name, fn in runs.items():   # per-kernel device times of one call of each
            solver.set_profiling(True)
            fn()
            kt = solver.kernel_times()
            solver.set_profiling(False)
            out[name + "_kernels_ms"] = {k: round(v[1], 4) for k, v in kt.items()}
            out[name + "_device_ms"] = round(sum(v[1] for v in kt.values()), 4)
    # the assign kernel must read starts, ends and ids of every read (12 bytes) and write the three solve columns (12
    # bytes), one label per pair and one bit per pair; with rows in pooled mode three more columns.  The table (2.4 KB)
    # is staged in LDS
    for name, extra in (("amplicons_pooled", 0), ("amplicons_pooled_rows", 12)):
        need = (24 + extra) * n + 4 * n_pairs + n_pairs // 8
        ms = out[name + "_kernels_ms"].get("k_amplicon_clip")
        if ms:
            out["assign_kernel_" + name] = {"ms": ms, "bytes": int(need), "TBps": round(need / (ms * 1e-3) / 1e12, 2),
                                            "share_of_copy_rate": round(need / (ms * 1e-3) / (COPY_TBPS * 1e12), 3)}
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
