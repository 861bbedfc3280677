"""Times, on the device in one run, solve_start_cap_device on cfg4's reads (8 contigs x 12.5 M reads of one length, L =
10^6, M = 100, shuffled, MAPQ 0..60 as priorities) and on the same reads with 1 % clipped by 1..39 bases, for K in 1, 4,
16: wall clock around blocking calls (warm-up, then alternating with the two references, median of --reps) and ms_cap
(the device time of everything except the inner solve).  The references, in the same run: solve_dedup_device in read mode
without tags on the same reads (the same sort, scan and compaction) and the plain solve_by_contig_device.  Also, per
input, cells_kept / reads kept for the plain mask (numpy) and for every K: the diversity the cap buys.
--only dedup times the dedup reference alone (set QMCP_HIP_LIB to another build of the library to time that build).
    python lab/start_cap_time.py [--pairs 6250000] [--reps 5] [--only dedup] [--out profiles/start_cap_time.json]"""
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
CAPS = (1, 4, 16)


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6_250_000, help="pairs per contig (cfg4: 6.25 M = 12.5 M reads)")
    ap.add_argument("--contigs", type=int, default=8)
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("dedup",), default=None)
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
    perm = rng.permutation(n)
    s, e, ids = s[perm], e[perm], ids[perm]
    q = rng.integers(0, 61, size=n).astype(np.uint32)
    pick = rng.random(n) < 0.01
    clip = rng.integers(1, 40, size=n).astype(np.uint32)
    front = rng.random(n) < 0.5
    s_clip = np.where(pick & front, s + clip, s).astype(np.uint32)
    e_clip = np.where(pick & ~front, e - clip, e).astype(np.uint32)
    lengths = np.full(n_contigs, L, dtype=np.uint32)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev)
    d_ids, d_q = up(ids), up(q)
    words = pkg.mask_words(n)
    d_mask = torch.zeros(words, dtype=torch.int64, device=dev)
    d_other = torch.zeros(words, dtype=torch.int64, device=dev)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"commit": commit or "unknown", "library": pkg.HIP_LIB_PATH, "reads": int(n), "contigs": n_contigs, "M": M,
           "reps": args.reps, "order": "shuffled", "spans": sorted(set((e[:1000] - s[:1000]).tolist()))}
    with pkg.Solver(0) as solver:
        for label, hs, he in (("one_length", s, e), ("clipped_1pct", s_clip, e_clip)):
            d_s, d_e = up(hs), up(he)
            torch.cuda.synchronize()

            def cap(K):
                return solver.solve_start_cap_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, M, K,
                                                     d_mask.data_ptr(), d_priorities=d_q.data_ptr(),
                                                     d_capped_mask=d_other.data_ptr(), hist_bins=64)

            def dedup():
                return solver.solve_dedup_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, M,
                                                 d_mask.data_ptr(), d_qualities=d_q.data_ptr(),
                                                 d_dup_mask=d_other.data_ptr(), hist_bins=64)

            def plain():
                return solver.solve_by_contig_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, M,
                                                     d_mask.data_ptr())

            modes = [("dedup_read", dedup)]
            if args.only is None:
                modes += [(f"cap_{K}", (lambda K=K: cap(K))) for K in CAPS] + [("plain", plain)]
            res = {}
            for name, f in modes:   # warm-up, and what does not change from run to run
                f()
                if name.startswith("cap_"):
                    st = solver.last_start_cap_stats.as_dict()
                    kept = int(solver.last_stats.n_kept)
                    res[name + "_stats"] = st
                    res[name + "_reads_kept"] = kept
                    res[name + "_cells_kept_per_read_kept"] = round(st["cells_kept"] / max(kept, 1), 4)
                elif name == "dedup_read":
                    res[name + "_stats"] = solver.last_dedup_stats.as_dict()
                elif name == "plain":
                    torch.cuda.synchronize()
                    bits = np.unpackbits(d_mask.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
                    cells = np.unique(ids[bits].astype(np.uint64) << np.uint64(32) | hs[bits].astype(np.uint64)).size
                    res["plain_reads_kept"] = int(bits.sum())
                    res["plain_cells_kept_per_read_kept"] = round(cells / max(int(bits.sum()), 1), 4)
            times = {name: [] for name, _ in modes}
            inner = {name: [] for name, _ in modes if name != "plain"}
            for _ in range(args.reps):   # alternating
                for name, f in modes:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) * 1e3)
                    if name.startswith("cap_"):
                        inner[name].append(solver.last_start_cap_stats.ms_cap)
                    elif name == "dedup_read":
                        inner[name].append(solver.last_dedup_stats.ms_dedup)
            for name, v in times.items():
                res[name + "_call_ms"] = summary(v)
            for name, v in inner.items():
                res[name + "_ms_pre_pass"] = summary(v)
            out[label] = res
            del d_s, d_e
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
