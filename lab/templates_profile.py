"""What the bitset completion of qmcp_hip_solve_templates_device costs, on lab/pairs_profile.py's input (cfg4's shape as
pairs: 8 contigs of 1 M positions, 12.5 M reads of 150 each per contig, the mate 100 .. 499 positions behind, pairs
shuffled), M = 100 under the default stages.  Three calls on the same reads, alternating, medians over --reps:
  pairs       solve_pairs_device: ms_pairs, the per-stage device times
  ids i / 2   solve_templates_device with template_ids[i] = i / 2: the same mask (checked), ms_templates
  random      solve_templates_device with template sizes 1 .. 6 dealt over the reads by a random permutation
and under profiling the kernels the feature adds (id check + sizes + histogram once per call; mark + spread per stage).

  python lab/templates_profile.py [--reps 3] [--pairs 6250000] [--out profiles/templates_cfg4.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "templates_cfg4.json"))
    args = ap.parse_args()
    n_contigs, pairs, L, rl, M = 8, args.pairs, 1_000_000, 150, 100
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
    sizes = rng.integers(1, 7, size=n // 2)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), n)) + 1]
    scattered = np.repeat(np.arange(sizes.size, dtype=np.uint32), sizes)[:n][rng.permutation(n)]
    n_scattered = int(scattered.max()) + 1
    print(f"input ready: {n} reads, {n_scattered} random templates", flush=True)
    dev = torch.device("cuda", 0)
    d_s, d_e, d_ids, d_half, d_scat = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids, halves, scattered))
    d_masks = [torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev) for _ in range(3)]
    torch.cuda.synchronize()

    out = {"reads": int(n), "contigs": n_contigs, "positions_per_contig": L, "read_length": rl, "max_coverage": M,
           "stages": "default", "reps": args.reps, "random_templates": n_scattered,
           "flag_bytes": {"ids i / 2": n // 2 // 8, "random": n_scattered // 8}}
    with pkg.Solver(0) as solver:
        def run_pairs():
            return solver.solve_pairs_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, M,
                                             d_masks[0].data_ptr())

        def run_templates(d_tids, n_templates, d_mask):
            return solver.solve_templates_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), d_tids.data_ptr(), n,
                                                 n_templates, lengths, M, d_mask.data_ptr())

        calls = {"pairs": run_pairs,
                 "ids i / 2": lambda: run_templates(d_half, n // 2, d_masks[1]),
                 "random": lambda: run_templates(d_scat, n_scattered, d_masks[2])}
        for name, call in calls.items():                              # the warm-up of all three
            call()
            print(f"warm-up done: {name}", flush=True)
        assert torch.equal(d_masks[0], d_masks[1]), "ids i / 2 do not give the mask of solve_pairs_device"
        wall = {k: [] for k in calls}
        extra = {k: [] for k in calls}
        stage = {k: [] for k in calls}
        last = {}
        for _ in range(args.reps):                                    # alternating the three
            for name, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, st = call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                extra[name].append(float(st.ms_pairs if name == "pairs" else st.ms_templates))
                stage[name].append([float(x) for x in st.ms_stage[:st.n_stages]])
                last[name] = st
        med = lambda v: round(statistics.median(v), 3)
        for name in calls:
            st = last[name]
            k = st.n_stages
            row = {"whole_call_ms": med(wall[name]), "ms_around_the_solves": med(extra[name]),
                   "device_ms_per_stage": [med([r[j] for r in stage[name]]) for j in range(k)],
                   "n_selected": [int(x) for x in st.n_selected[:k]], "n_kept": [int(x) for x in st.n_kept[:k]]}
            if name != "pairs":
                row.update(templates_used=int(st.n_templates_used), templates_kept=int(st.n_templates_kept),
                           max_template_size=int(st.max_template_size), size_hist=[int(x) for x in st.size_hist])
            solver.set_profiling(True)
            calls[name]()
            row["kernel_times_ms"] = {k_: round(v[1], 4) for k_, v in solver.kernel_times().items()
                                      if "tpl" in k_ or "complete_pairs" in k_}
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
