"""What fragment depth costs: 5 x 10^7 pairs of 2 x 150 shuffled over 8 contigs of 10^6 positions, fragment lengths
160 .. 400, so that roughly half the pairs overlap (10^8 segments, template ids i // 2 before the shuffle).
In one process, wall time of the blocking device calls, medians over --reps after a warm-up:
  clip        clip_templates_device
  fragments   solve_fragments_device at --coverage
  templates   solve_templates_device on the same rows (the per-segment solve the clip precedes)
  copy        a device-to-device copy that moves the bytes the clip must move: it reads four columns and writes two,
              24 bytes per segment, so the copy is of 12 bytes per segment (read + written = 24)
and, from one more profiled clip, its kernels by name.  The ratio clip : templates and the achieved GB/s of the clip
against the copy go to the JSON.

  python lab/fragment_time.py [--reps 5] [--scale 1.0] [--coverage 1000] [--out profiles/fragment_time.json]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 5 x 10^7 pairs")
    ap.add_argument("--coverage", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fragment_time.json"))
    args = ap.parse_args()
    n_contigs, L, rl = 8, 1_000_000, 150
    P = int(50_000_000 * args.scale)
    rng = np.random.default_rng(21)
    fl = rng.integers(160, 401, P, dtype=np.int64)
    fs = (rng.random(P) * (L - fl)).astype(np.int64)
    cid = rng.integers(0, n_contigs, P, dtype=np.int64)
    n = 2 * P
    perm = rng.permutation(n)
    s = np.empty(n, np.uint32)
    e = np.empty(n, np.uint32)
    s[0::2], e[0::2] = fs, fs + rl - 1
    s[1::2], e[1::2] = fs + fl - rl, fs + fl - 1
    ids = np.repeat(cid, 2).astype(np.uint32)
    tids = (np.arange(n, dtype=np.int64) // 2).astype(np.uint32)
    overlapping = int((fl < 2 * rl).sum())
    s, e, ids, tids = s[perm], e[perm], ids[perm], tids[perm]
    del perm, fl, fs, cid
    lengths = np.full(n_contigs, L, np.uint32)
    print(f"{n} segments, {overlapping} of {P} pairs overlap", flush=True)
    dev = torch.device("cuda", 0)
    cols = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids, tids)]
    outs = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)]
    mask = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev)
    src = torch.zeros(3 * n, dtype=torch.int32, device=dev)
    dst = torch.zeros(3 * n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ptr = [c.data_ptr() for c in cols]
    torch.cuda.synchronize()
    result = {"segments": n, "pairs": P, "pairs_overlapping": overlapping, "contigs": n_contigs,
              "positions": int(n_contigs * L), "coverage": args.coverage, "reps": args.reps}

    with pkg.Solver(0) as solver:
        state = {}

        def clip():
            state["fs"] = solver.clip_templates_device(*ptr, n, P, lengths, outs[0].data_ptr(), outs[1].data_ptr(),
                                                       stream=stream)

        def fragments():
            state["frag"] = solver.solve_fragments_device(*ptr, n, P, lengths, args.coverage, mask.data_ptr(), stream=stream)

        def templates():
            state["tpl"] = solver.solve_templates_device(*ptr, n, P, lengths, args.coverage, mask.data_ptr(), stream=stream)

        def copy():
            dst.copy_(src)

        def timed(call):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        ms = {}
        for name, call in (("copy", copy), ("clip", clip), ("templates", templates), ("fragments", fragments)):
            timed(call)                                                  # warm-up: the arena grows here
            runs = [timed(call) for _ in range(args.reps)]
            ms[name] = statistics.median(runs)
            result[f"ms_{name}"] = ms[name]
            result[f"ms_{name}_runs"] = runs
            print(f"{name}: median {ms[name]:.2f} ms over {runs}", flush=True)
        fs = state["fs"]
        result["fragment_stats"] = fs.as_dict()
        result["segments_kept_fragments"] = int(state["frag"][1].n_kept[state["frag"][1].n_stages - 1])
        result["segments_kept_templates"] = int(state["tpl"][1].n_kept[state["tpl"][1].n_stages - 1])
        solver.set_profiling(True)
        clip()
        torch.cuda.synchronize()
        result["clip_kernels_ms"] = {k: {"launches": v[0], "ms": v[1]} for k, v in solver.kernel_times().items()}
        solver.set_profiling(False)
    moved = 24.0 * n
    result["bytes_moved_min"] = moved
    result["gbps_clip"] = moved / (ms["clip"] * 1e-3) / 1e9
    result["gbps_copy"] = moved / (ms["copy"] * 1e-3) / 1e9
    result["ratio_clip_to_templates"] = ms["clip"] / ms["templates"]
    result["ratio_fragments_to_templates"] = ms["fragments"] / ms["templates"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if not k.endswith("_runs")}), flush=True)


if __name__ == "__main__":
    main()
