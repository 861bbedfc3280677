"""qmcp_hip_solve_replicates_device on cfg4's reads (8 contigs x 12.5 M reads, 1 M positions each, reads of 150) in
shuffled order, coverages [100] * 4: the whole call against the only route without the entry -- solve_by_contig_device
per replicate, on columns whose complement was compacted with torch in between, which regroups the reads at every
replicate --, the device time per replicate, what the call adds around the solves by kernel, and, from lab/replicates_lab
(built as its header says; skipped when the binary is not there), k_rep_split against k_ladder_compact on the
complemented mask with the bytes moved and the fraction of a plain device-to-device copy's bandwidth.

  python lab/replicates_profile.py [--reps 5] [--out profiles/replicates_cfg4.json]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replicates_cfg4.json"))
    args = ap.parse_args()
    n_contigs, pairs, L, rl, cov = 8, 6_250_000, 1_000_000, 150, [100] * 4
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, rl, seed=12345 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
    perm = np.random.default_rng(4).permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    n = s.size
    lengths = np.full(n_contigs, L, dtype=np.uint32)
    dev = torch.device("cuda", 0)
    d_s, d_e, d_ids = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids))
    d_labels = torch.zeros(n, dtype=torch.uint8, device=dev)
    shifts = torch.arange(64, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    out = {"reads": int(n), "contigs": n_contigs, "coverages": cov, "reps": args.reps, "order": "shuffled"}
    with pkg.Solver(0) as solver:
        def split(flags=0):
            return solver.solve_replicates_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, cov,
                                                  d_labels.data_ptr(), flags=flags)

        def chain():
            cols, free = (d_s, d_e, d_ids), torch.arange(n, device=dev)
            labels = torch.zeros(n, dtype=torch.uint8, device=dev)
            device_ms = []
            for r, M in enumerate(cov, start=1):
                m = cols[0].numel()
                mask = torch.zeros(pkg.mask_words(m), dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                st = solver.solve_by_contig_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), m,
                                                   lengths, M, mask.data_ptr())
                device_ms.append(float(st.ms_total))
                bits = ((mask.unsqueeze(1) >> shifts) & 1).flatten()[:m].bool()
                labels[free[bits]] = r
                cols = tuple(c[~bits].contiguous() for c in cols)
                free = free[~bits]
            torch.cuda.synchronize()
            return labels, device_ms

        want, _ = chain()
        split()
        out["replicates_equal_chain"] = bool(torch.equal(d_labels, want))
        t_split, t_chain, per_rep, extra, chain_solves = [], [], [], [], []
        for _ in range(args.reps):   # alternating the two
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rs = split()
            t_split.append((time.perf_counter() - t0) * 1e3)
            per_rep.append([float(x) for x in rs.ms_replicate[:len(cov)]])
            extra.append(float(rs.ms_split))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, ms = chain()
            t_chain.append((time.perf_counter() - t0) * 1e3)
            chain_solves.append(ms)
        med = lambda v: round(statistics.median(v), 3)
        out["n_offered"] = [int(x) for x in rs.n_offered[:len(cov)]]
        out["n_kept"] = [int(x) for x in rs.n_kept[:len(cov)]]
        out["routes_sort_passes"] = [int(r.sort_passes) for r in solver.last_replicate_solve_stats]
        out["replicates_ms"] = {"median": med(t_split), "min": round(min(t_split), 3), "max": round(max(t_split), 3)}
        out["ms_replicate"] = [med([r[j] for r in per_rep]) for j in range(len(cov))]
        out["ms_split"] = med(extra)
        out["chain_ms"] = {"median": med(t_chain), "min": round(min(t_chain), 3), "max": round(max(t_chain), 3)}
        out["chain_device_ms_of_the_batches_per_replicate"] = [med([r[j] for r in chain_solves]) for j in range(len(cov))]
        for name, flags in (("whole_pairs", pkg.REPLICATES_WHOLE_PAIRS), ("shortfall", pkg.REPLICATES_SHORTFALL)):
            split(flags)
            times = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rs = split(flags)
                times.append((time.perf_counter() - t0) * 1e3)
            out[f"replicates_ms_{name}"] = {"median": med(times), "ms_split": round(float(rs.ms_split), 3)}
        mine = ("k_rep", "replicate offsets", "k_ladder_levels(replicates)")
        for name, flags in (("plain", 0), ("whole_pairs", pkg.REPLICATES_WHOLE_PAIRS)):
            solver.set_profiling(True)
            split(flags)
            out[f"ms_split_by_kernel_{name}"] = {k: round(v[1], 4) for k, v in solver.kernel_times().items()
                                                 if k.startswith(mine)}
            solver.set_profiling(False)
    lab = os.path.join(ROOT, "lab", "replicates_lab")
    if os.path.exists(lab):
        # one replicate's step alone, at the density the call above met: taken / offered of replicate 1
        per_mille = max(1, round(1000 * out["n_kept"][0] / out["n_offered"][0]))
        run = subprocess.run([lab, str(n), str(per_mille)], capture_output=True, text=True, timeout=300)
        out["split_step_alone"] = json.loads(run.stdout) if run.returncode == 0 else {"failed": run.returncode,
                                                                                      "stderr": run.stderr[-400:]}
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
