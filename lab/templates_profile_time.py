"""What qmcp_hip_solve_templates_profile_device costs on lab/pairs_profile.py's input (cfg4's shape as pairs: 8 contigs
of 1 M positions, 12.5 M reads of 150 each per contig, the mate 100 .. 499 positions behind, pairs shuffled) as templates
of two, M = 100 under the default stages.  Half the positions lie in regions at M (--width positions every 2 x --width),
the cap is 0 elsewhere.  Two calls on the same reads, alternating, medians over --reps:
  templates           solve_templates_device: one cap everywhere
  templates_profile   solve_templates_profile_device under the table
Reported as measured: the whole blocking call, the per-stage device times, ms_need, ms_templates, the on-cap pass and the
need kernels under profiling, the segments kept and the mean kept depth on target (per target position) of both calls.

  python lab/templates_profile_time.py [--reps 3] [--pairs 6250000] [--width 1500] [--out profiles/templates_profile.json]"""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=6_250_000, help="pairs per contig")
    ap.add_argument("--width", type=int, default=1500, help="positions per region; one region every 2 x width")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "templates_profile.json"))
    args = ap.parse_args()
    n_contigs, pairs, L, rl, M, width = 8, args.pairs, 1_000_000, 150, 100, args.width
    rng = np.random.default_rng(12345)
    s1 = rng.integers(0, L - rl - 500, size=n_contigs * pairs)
    s2 = s1 + rng.integers(100, 500, size=s1.size)
    order = rng.permutation(s1.size)
    s = np.empty(2 * s1.size, np.uint32)
    s[0::2], s[1::2] = s1[order], s2[order]
    e = s + np.uint32(rl - 1)
    ids = np.repeat((order // pairs).astype(np.uint32), 2)
    n = s.size
    lengths = np.full(n_contigs, L, dtype=np.uint32)
    halves = (np.arange(n, dtype=np.uint32) >> 1)
    starts_1 = np.arange(0, L, 2 * width, dtype=np.uint32)
    offs = (np.arange(n_contigs + 1) * starts_1.size).astype(np.uint32)
    r0 = np.tile(starts_1, n_contigs)
    r1 = np.minimum(r0 + width - 1, L - 1).astype(np.uint32)
    caps = np.full(r0.size, M, np.uint32)
    on_target = int((r1.astype(np.int64) - r0 + 1).sum())

    def below(x):                                                      # target positions of a contig below x
        x = x.astype(np.int64)
        return (x // (2 * width)) * width + np.minimum(x % (2 * width), width)

    overlap = below(e.astype(np.int64) + 1) - below(s)                # target positions under each read
    print(f"input ready: {n} reads, {r0.size} regions, {on_target} target positions", flush=True)
    dev = torch.device("cuda", 0)
    d_s, d_e, d_ids, d_half = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids, halves))
    d_masks = [torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev) for _ in range(2)]
    torch.cuda.synchronize()

    out = {"reads": int(n), "contigs": n_contigs, "positions_per_contig": L, "read_length": rl, "max_coverage": M,
           "stages": "default", "reps": args.reps, "regions": int(r0.size), "region_width": width,
           "target_positions": on_target, "default_cap": 0}
    with pkg.Solver(0) as solver:
        def run_templates():
            st, ts = solver.solve_templates_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), d_half.data_ptr(), n,
                                                   n // 2, lengths, M, d_masks[0].data_ptr())
            return ts, None

        def run_capped():
            st, ts, qs = solver.solve_templates_profile_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(),
                                                               d_half.data_ptr(), n, n // 2, lengths, M, 0,
                                                               d_masks[1].data_ptr(), offs, r0, r1, caps)
            return ts, qs

        calls = {"templates": run_templates, "templates_profile": run_capped}
        for name, call in calls.items():
            call()
            print(f"warm-up done: {name}", flush=True)
        wall = {k: [] for k in calls}
        extra = {k: [] for k in calls}
        stage = {k: [] for k in calls}
        need = []
        last = {}
        for _ in range(args.reps):                                    # alternating the two
            for name, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ts, qs = call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                extra[name].append(float(ts.ms_templates))
                stage[name].append([float(x) for x in ts.ms_stage[:ts.n_stages]])
                if qs is not None:
                    need.append(float(qs.ms_need))
                last[name] = (ts, qs)
        med = lambda v: round(statistics.median(v), 3)
        for k_mask, name in enumerate(calls):
            ts, qs = last[name]
            k = ts.n_stages
            kept = np.unpackbits(d_masks[k_mask].cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
            row = {"whole_call_ms": med(wall[name]), "whole_call_ms_runs": [round(x, 3) for x in wall[name]],
                   "ms_templates": med(extra[name]),
                   "device_ms_per_stage": [med([r[j] for r in stage[name]]) for j in range(k)],
                   "n_selected": [int(x) for x in ts.n_selected[:k]], "n_kept": [int(x) for x in ts.n_kept[:k]],
                   "sweeps": [int(x) for x in ts.sweeps[:k]], "templates_kept": int(ts.n_templates_kept),
                   "mean_kept_depth_on_target": round(float(overlap[kept].sum()) / on_target, 2),
                   "mean_kept_depth_everywhere": round(float(kept.sum()) * rl / (n_contigs * L), 2)}
            if qs is not None:
                row.update(ms_need=med(need), segments_on_cap=int(qs.n_segments_on_cap),
                           templates_on_cap=int(qs.n_templates_on_cap), positions_in_regions=int(qs.positions_in_regions))
            solver.set_profiling(True)
            calls[name]()
            row["kernel_times_ms"] = {k_: round(v[1], 4) for k_, v in solver.kernel_times().items()
                                      if "tpl" in k_ or "need" in k_ or "sweep" in k_}
            solver.set_profiling(False)
            out[name] = row
            print(f"measured: {name}", flush=True)
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
