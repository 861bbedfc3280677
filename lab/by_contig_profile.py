"""qmcp_hip_solve_by_contig_device on cfg4's reads (8 contigs x 12.5 M reads, 1 M positions each, reads of 150, M = 100):
end-to-end time of the grouped solve (qmcp_hip_solve_device on reads already grouped) against the by-contig solve on the
same reads interleaved across the contigs (each contig's reads in their order) and fully shuffled; and, with the
context's per-kernel events on, the grouping and scatter-back kernels' times at 10^8 reads against the bytes they move.

  python lab/by_contig_profile.py [--reps 10] [--out FILE]

Run it alone for the times, under `rocprofv3 --kernel-trace --stats` for the kernel table (--reps 3 is enough)."""
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

COPY_TBPS = 6.29   # MI355X_MICROARCH.md: measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n_contigs, pairs, L, rl, M = 8, 6_250_000, 1_000_000, 150, 100
    ss, ee = [], []
    for c in range(n_contigs):
        s, e = pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, rl, seed=12345 + c)
        ss.append(s)
        ee.append(e)
    s, e = np.concatenate(ss), np.concatenate(ee)
    n = s.size
    offs = np.arange(n_contigs + 1, dtype=np.uint64) * (2 * pairs)
    lengths = np.full(n_contigs, L, dtype=np.uint32)
    ids_grouped = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
    rng = np.random.default_rng(4)
    ids_inter = rng.permutation(ids_grouped)
    where = np.argsort(ids_inter, kind="stable")
    s_inter, e_inter = np.empty_like(s), np.empty_like(e)
    s_inter[where], e_inter[where] = s, e
    perm = rng.permutation(n)
    s_shuf, e_shuf, ids_shuf = s[perm], e[perm], ids_grouped[perm]

    dev = torch.device("cuda", 0)
    to_dev = lambda a: torch.from_numpy(a.view(np.int32)).to(dev)
    d = {k: tuple(to_dev(x) for x in v) for k, v in
         {"grouped": (s, e, ids_grouped), "interleaved": (s_inter, e_inter, ids_inter),
          "shuffled": (s_shuf, e_shuf, ids_shuf)}.items()}
    d_mask = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    out = {"reads": int(n), "contigs": n_contigs, "M": M, "reps": args.reps}
    masks = {}
    with pkg.Solver(0) as solver:
        def grouped():
            return solver.solve_device(d["grouped"][0].data_ptr(), d["grouped"][1].data_ptr(), n, lengths, M,
                                       d_mask.data_ptr(), contig_read_offsets=offs)

        def by_contig(name):
            t = d[name]
            return solver.solve_by_contig_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, lengths, M,
                                                 d_mask.data_ptr())

        runs = {"grouped_solve_device": grouped,
                "by_contig_interleaved": lambda: by_contig("interleaved"),
                "by_contig_shuffled": lambda: by_contig("shuffled"),
                "by_contig_grouped_input": lambda: by_contig("grouped")}
        for name, fn in runs.items():
            fn()
            torch.cuda.synchronize()
            masks[name] = d_mask.cpu().numpy().view(np.uint64).copy()
        times = {name: [] for name in runs}
        for _ in range(args.reps):   # alternating the variants
            for name, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
                if name != "grouped_solve_device":
                    out.setdefault("stats_" + name, {"path": int(st.path), "n_kept": int(st.n_kept),
                                                     "device_ms_of_the_batches": round(float(st.ms_total), 3)})
        for name, v in times.items():
            out[name + "_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
                                 "max": round(max(v), 3)}
        # one bit pattern for the grouped solve and for the interleaved input mapped back
        want = np.zeros(n, dtype=bool)
        want[where] = np.unpackbits(masks["grouped_solve_device"].view(np.uint8), bitorder="little")[:n].astype(bool)
        out["interleaved_equals_grouped"] = bool(np.array_equal(
            np.unpackbits(masks["by_contig_interleaved"].view(np.uint8), bitorder="little")[:n].astype(bool), want))
        out["grouped_input_equals_grouped"] = bool(np.array_equal(masks["by_contig_grouped_input"],
                                                                  masks["grouped_solve_device"]))
        # per-kernel device times of the grouping and scatter-back (HIP events around each launch group)
        solver.set_profiling(True)
        by_contig("shuffled")
        kt = solver.kernel_times()
        solver.set_profiling(False)
    kept = int(out["stats_by_contig_shuffled"]["n_kept"])
    # bytes each stage needs at minimum: keys (ids, starts, ends in; keys out), one radix pass (keys in; hist) +
    # (keys in; {key, index} out), bounds (records in), gather ({key, index} in; starts, ends gathered; both out),
    # scatter-back (grouped mask in; per kept read its record and one 4-byte read-modify-write)
    need = {"k_bc_keys": 16 * n, "k_radix_hist_rec(by contig)": 4 * n, "k_radix_scatter_rec(by contig)": 12 * n,
            "k_bc_bounds": 8 * n, "k_bc_gather": 24 * n, "k_bc_scatter_mask": n // 8 + 16 * kept}
    stages = {}
    for name, (launches, ms) in kt.items():
        if name in need or "by contig" in name:
            b = need.get(name)
            stages[name] = {"launches": launches, "ms": round(ms, 4)}
            if b:
                stages[name]["bytes"] = int(b)
                stages[name]["GBps"] = round(b / (ms * 1e-3) / 1e9, 1) if ms > 0 else None
                stages[name]["share_of_copy_rate"] = round(b / (ms * 1e-3) / (COPY_TBPS * 1e12), 3) if ms > 0 else None
    out["grouping_and_scatter_kernels"] = stages
    out["grouping_ms"] = round(sum(v["ms"] for k, v in stages.items() if k != "k_bc_scatter_mask"), 4)
    out["scatter_back_ms"] = stages.get("k_bc_scatter_mask", {}).get("ms")
    out["all_kernel_times_ms"] = {k: round(v[1], 4) for k, v in kt.items()}
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
