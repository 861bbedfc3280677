"""qmcp_hip_filter_solve_by_contig_host on a cfg3-sized multi-reference amplicon panel: 8 influenza-like segments
(13.6 kb), 25 amplicons each, 15 M pairs (30 M reads), a tenth of the pairs straddling two amplicons, about 1 % with
mates on two segments, M = 200, mates completed -- next to the single-reference cfg3 filter_solve (29 903 bases, 98
amplicons, 30 M reads, M = 200) on the same device.  Reports the end-to-end host-entry time of both (host clock, H2D
and D2H included), the device time of every kernel of one call (the context's per-kernel events), the device time of
the whole entry (the sum of those) and the FILTER kernel's effective bandwidth (bytes it must read / its time).

  python lab/amplicon_by_contig_profile.py [--reps 10] [--out FILE]

Run it alone for the times, under `rocprofv3 --kernel-trace --stats` for the kernel table (--reps 3 is enough)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("genome-downsampler_amd")
import amplicon_panels as ap   # noqa: E402
import workloads   # noqa: E402

COPY_TBPS = 6.29   # MI355X_MICROARCH.md: measured float4 copy
M = 200


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--reps", type=int, default=10)
    ap_.add_argument("--out", default=None)
    args = ap_.parse_args()
    refs = ap.INFLUENZA
    names = [n for n, _ in refs]
    lengths = np.array([L for _, L in refs], np.uint32)
    offs, a0, a1 = ap.panel_csr(ap.segment_panel(refs), names)
    rng = np.random.default_rng(2009)
    n_pairs = 15_000_000
    s, e, ids = ap.panel_pairs(rng, lengths, offs, a0, a1, n_pairs, straddle=0.10, cross=0.01)
    cs, ce, c0, c1, _ = workloads.amplicon_reads(n_pairs)
    n = s.size
    out = {"reads": int(n), "references": len(refs), "genome": int(lengths.sum()), "amplicons": int(a0.size), "M": M,
           "reps": args.reps, "cross_reference_pairs": int((ids[0::2] != ids[1::2]).sum())}
    with pkg.Solver(0) as solver:
        runs = {
            "filter_solve_by_contig": lambda: solver.filter_solve_by_contig(
                s, e, ids, lengths, M, amp_offsets=offs, amp_starts=a0, amp_ends=a1, complete_pairs=True),
            "filter_solve_cfg3_single_reference": lambda: solver.filter_solve(
                cs, ce, 29_903, M, amp_starts=c0, amp_ends=c1, complete_pairs=True),
        }
        for fn in runs.values():   # warm-up: code objects, arena
            fn()
        times = {name: [] for name in runs}
        for _ in range(args.reps):   # alternating the two
            for name, fn in runs.items():
                t0 = time.perf_counter()
                mask, dropped = fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
                out.setdefault("pairs_dropped_" + name, int(dropped))
                out.setdefault("kept_" + name, int(np.unpackbits(mask.view(np.uint8)).sum()))
        for name, v in times.items():
            out[name + "_host_entry_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
                                            "max": round(max(v), 3)}
        # per-kernel device times of one call of each (HIP events around each launch group)
        for name, fn in runs.items():
            solver.set_profiling(True)
            fn()
            kt = solver.kernel_times()
            solver.set_profiling(False)
            out[name + "_kernels_ms"] = {k: round(v[1], 4) for k, v in kt.items()}
            out[name + "_device_ms"] = round(sum(v[1] for v in kt.values()), 4)
    # the FILTER must read starts, ends and ids of every read (12 bytes) and write one bit per pair; the amplicon table
    # (1.6 KB) and the offsets are cache-resident
    need = 12 * n + n_pairs // 8
    ms = out["filter_solve_by_contig_kernels_ms"].get("k_amplicon_filter_by_contig")
    if ms:
        out["filter_kernel"] = {"ms": ms, "bytes": int(need), "TBps": round(need / (ms * 1e-3) / 1e12, 2),
                                "share_of_copy_rate": round(need / (ms * 1e-3) / (COPY_TBPS * 1e12), 3)}
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
