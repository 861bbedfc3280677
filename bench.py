#!/usr/bin/env python3
"""Headline benchmark of the quasi-MCP solver path: Mreads/s selected at target coverage M=100.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cfg4|cfg2] [--mode per-gpu|sharded]
                  [--dump-outputs DIR]

A step is one pass of the hot path (device-resident reads -> device keep bitmask, plus the
RCCL gather of the masks when N > 1) over one batch of libs/reads-gen-style synthetic reads.
Workload, --mode per-gpu (default, weak scaling): BASELINE.json configs[3] PER GPU -- 8 contigs x
rand_reads_uniform(seed 12345 + c, 6 250 000 pairs, L = 1 000 000, len 150), 100 M reads, M = 100;
rank r uses seeds 12345 + 8 r + c.  --mode sharded (strong scaling): ONE configs[3] for the whole
job, its 8 contigs dealt to the ranks by genome-downsampler_amd.sharding.assign_contigs, every rank
solving its share, masks gathered (padded to the largest share).  Inputs are resident in HBM when the
timed region starts.  Two solves are kept in flight per GPU (two solver contexts, the two-phase entry
qmcp_hip_solve_device_begin / _end): the selection sweep of one -- a serial chain on 8 of 256 compute
units -- runs beside the bandwidth-bound stages of the next; every solve and gather completes inside
the timed region.

For N > 1 either launch through torch.distributed.run (one rank per GPU over RCCL) or just run
`python bench.py --gpus N`: without WORLD_SIZE in the environment the script starts that launcher itself as a
child process (before torch or the GPU is touched) and exits with its code; rank 0 prints ONE JSON line.  The CPU baseline (oracle/, rank 0, N = 1 only) is a reported number, not the target.
"""
import argparse
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E peak (MI355X_MICROARCH.md: 8.0 TB/s spec)
# HBM bytes per launch from rocprofv3 PMC passes of this same command (profiles/summarize_pmc.py:
# separate FETCH_SIZE / WRITE_SIZE passes, gfx950 FETCH_SIZE x2 correction), keyed by workload
PMC_TRAFFIC_FILE = os.path.join(ROOT, "profiles", "r04_pmc_traffic_{workload}_inflight{depth}.json")

WORKLOADS = {
    # name: (contigs per GPU, pairs per contig, contig length, read length, M)
    "cfg4": (8, 6_250_000, 1_000_000, 150, 100),
    "cfg2": (1, 500_000, 30_000, 150, 100),
}


def algorithmic_bytes(n_reads, total_len, n_contigs):
    """8 B/read in, 1 bit/read out, 8 B per base of coverage array"""
    return 8.0 * n_reads + n_reads / 8.0 + 8.0 * (total_len + n_contigs)


def dump_outputs(out_dir, masks, n_reads):
    """--dump-outputs: the keep bitmask(s) the timed path's caller received from its last step, as .npy files two
    builds can be compared by, file for file (float32 / float64, well under 64 MB at any supported size):
      keep_sample.npy        float32, 1.0 where the read is kept, for a fixed seeded sample of at most 2^21 reads
                             (every read when there are fewer) -- one read drawn from each of 2^21 equal runs of indices
      keep_sample_index.npy  float64, the (ascending) read indices of that sample
      kept_per_block.npy     float32, kept reads in each run of 256 consecutive read indices, over the whole mask
                             (runs twice as long, and again, while the array would pass 16 MB: past 10^9 reads)
    masks: uint64 bitmasks, one per rank whose mask rank 0 holds, concatenated in rank order; n_reads: the reads each
    of them covers."""
    keep = np.concatenate([np.unpackbits(m.view(np.uint8), bitorder="little")[:n] for m, n in zip(masks, n_reads)])
    n, n_sample = keep.size, 1 << 21
    if n <= n_sample:
        idx = np.arange(n, dtype=np.int64)
    else:
        edges = np.arange(n_sample + 1, dtype=np.int64) * n // n_sample
        draw = np.random.default_rng(20240229).random(n_sample)
        idx = edges[:-1] + (draw * (edges[1:] - edges[:-1])).astype(np.int64)
    block = 256
    while (n + block - 1) // block * 4 > 16e6:
        block *= 2
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "keep_sample.npy"), keep[idx].astype(np.float32))
    np.save(os.path.join(out_dir, "keep_sample_index.npy"), idx.astype(np.float64))
    np.save(os.path.join(out_dir, "kept_per_block.npy"),
            np.add.reduceat(keep, np.arange(0, n, block), dtype=np.float32) if n else np.zeros(0, np.float32))


def cfg5_share(pkg, torch, dev, solver, stream):
    """One GPU's share of configs[4] (the genome-scale configuration: 24 contigs with lengths ~ GRCh38,
    10^9 reads on 1.5 * 10^9 positions, M = 50) at 1/8 scale -- 125 M reads on 187.5 M positions, coverage
    2 x M -- outside the timed region and never `value`: device-resident reads -> device keep mask, best of
    three.  Its kept set is compared with the oracle contig by contig in tests/test_gpu_full_size.py."""
    synthetic = importlib.import_module("genome-downsampler_amd.synthetic")
    s, e, offs, lengths = synthetic.wgs_contigs(int(1.5e9 / 8), int(0.5e9 / 8))
    n = int(s.size)
    d_s = torch.from_numpy(s.view(np.int32)).to(dev)
    d_e = torch.from_numpy(e.view(np.int32)).to(dev)
    s2, e2 = synthetic.clipped_mix(s, e, 0.01)
    del s, e
    d_m = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev)
    best = None
    for _ in range(3):
        st = solver.solve_device(d_s.data_ptr(), d_e.data_ptr(), n, lengths, 50, d_m.data_ptr(),
                                 contig_read_offsets=offs, stream=stream)
        if best is None or st.ms_total < best["device_ms"]:
            best = {"device_ms": round(float(st.ms_total), 3), "sweep_ms": round(float(st.ms_sweep), 3),
                    "kept": int(st.n_kept), "stretches": int(st.sweep_stretches),
                    "speculative_boundaries": int(st.spec_boundaries),
                    "boundaries_that_disagreed": int(st.spec_mismatches)}
    # the same share with 1 % of its reads clipped by 1...50 bases: the near-uniform route
    # with its sweeps in stretches; parity: tests/test_gpu_full_size.py::test_cfg5_real_share_with_clipped_reads
    d_s.copy_(torch.from_numpy(s2.view(np.int32)))
    d_e.copy_(torch.from_numpy(e2.view(np.int32)))
    del s2, e2
    clipped = None
    for _ in range(3):
        st = solver.solve_device(d_s.data_ptr(), d_e.data_ptr(), n, lengths, 50, d_m.data_ptr(),
                                 contig_read_offsets=offs, stream=stream)
        if clipped is None or st.ms_total < clipped["device_ms"]:
            clipped = {"device_ms": round(float(st.ms_total), 3), "path": int(st.path), "kept": int(st.n_kept),
                       "exceptions": int(st.near_uniform_exceptions), "exceptions_kept": int(st.near_uniform_selected),
                       "sweeps": int(st.near_uniform_rounds), "giveup": int(st.near_uniform_giveup),
                       "stretches": int(st.sweep_stretches)}
    clipped["ratio_to_one_length"] = round(clipped["device_ms"] / best["device_ms"], 2)
    best["clipped_1pct"] = clipped
    # ... and with 0.5 % of the reads LENGTHENED by 1...20 bases as well (deletions): longer reads leave the near-uniform
    # route; the mixed-span walk in speculative stretches (round 4: the rule is how deep the data is in standard
    # deviations, not that one length dominates; one chain per contig was 14.5 s).  Parity:
    # tests/test_gpu_full_size.py::test_cfg5_real_share_with_longer_reads
    e3 = synthetic.lengthened_mix(d_e.cpu().numpy().view(np.uint32), d_e.cpu().numpy().view(np.uint32), offs, lengths, 0.005)
    d_e.copy_(torch.from_numpy(e3.view(np.int32)))
    del e3
    longer = None
    for _ in range(2):
        st = solver.solve_device(d_s.data_ptr(), d_e.data_ptr(), n, lengths, 50, d_m.data_ptr(),
                                 contig_read_offsets=offs, stream=stream)
        if longer is None or st.ms_total < longer["device_ms"]:
            longer = {"device_ms": round(float(st.ms_total), 3), "path": int(st.path), "kept": int(st.n_kept),
                      "near_uniform_giveup": int(st.near_uniform_giveup), "stretches": int(st.sweep_stretches),
                      "speculative_boundaries": int(st.spec_boundaries), "boundaries_that_disagreed": int(st.spec_mismatches)}
    longer["ratio_to_one_length"] = round(longer["device_ms"] / best["device_ms"], 2)
    best["clipped_1pct_and_half_a_percent_longer"] = longer
    b_alg = algorithmic_bytes(n, int(lengths.sum()), lengths.size)
    best.update({"reads": n, "positions": int(lengths.sum()), "contigs": int(lengths.size), "max_coverage": 50,
                 "Mreads_per_s": round(n / best["device_ms"] / 1e3, 1),
                 "whole_solve_frac": round(b_alg / (best["device_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 5),
                 "note": "one solve alone on the device (HIP events), inputs resident; not the headline workload"})
    return best


def cfg5_real_share(pkg, torch, dev, solver, stream):
    """The heaviest rank's REAL share of configs[4] at full size (24 contigs, 1.5e9 positions, 1e9 reads dealt to 8
    ranks by sharding.assign_contigs): three contigs at full length -- 117.7 M, 52.0 M and 24.8 M positions, 129.7 M
    reads, M = 50 -- device-resident, one solve alone, best of three; never `value`.  Parity:
    tests/test_gpu_full_size.py::test_cfg5_real_share_of_the_heaviest_rank_at_full_length (== oracle)."""
    synthetic = importlib.import_module("genome-downsampler_amd.synthetic")
    share, owned = synthetic.cfg5_heaviest_share(8)
    s, e, offs, lengths = synthetic.wgs_contigs(int(1.5e9), int(0.5e9), only=share)
    n = int(s.size)
    d_s = torch.from_numpy(s.view(np.int32)).to(dev)
    d_e = torch.from_numpy(e.view(np.int32)).to(dev)
    s2, e2 = synthetic.clipped_mix(s, e, 0.01)
    del s, e
    d_m = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev)
    best = None
    for _ in range(3):
        st = solver.solve_device(d_s.data_ptr(), d_e.data_ptr(), n, lengths, 50, d_m.data_ptr(),
                                 contig_read_offsets=offs, stream=stream)
        if best is None or st.ms_total < best["device_ms"]:
            best = {"device_ms": round(float(st.ms_total), 3), "sweep_ms": round(float(st.ms_sweep), 3),
                    "kept": int(st.n_kept), "stretches": int(st.sweep_stretches),
                    "speculative_boundaries": int(st.spec_boundaries),
                    "boundaries_that_disagreed": int(st.spec_mismatches)}
    # the same share with 1 % of its reads clipped by 1...50 bases: the near-uniform route
    # with its sweeps in stretches; parity: tests/test_gpu_full_size.py::test_cfg5_real_share_with_clipped_reads
    d_s.copy_(torch.from_numpy(s2.view(np.int32)))
    d_e.copy_(torch.from_numpy(e2.view(np.int32)))
    del s2, e2
    clipped = None
    for _ in range(3):
        st = solver.solve_device(d_s.data_ptr(), d_e.data_ptr(), n, lengths, 50, d_m.data_ptr(),
                                 contig_read_offsets=offs, stream=stream)
        if clipped is None or st.ms_total < clipped["device_ms"]:
            clipped = {"device_ms": round(float(st.ms_total), 3), "path": int(st.path), "kept": int(st.n_kept),
                       "exceptions": int(st.near_uniform_exceptions), "exceptions_kept": int(st.near_uniform_selected),
                       "sweeps": int(st.near_uniform_rounds), "giveup": int(st.near_uniform_giveup),
                       "stretches": int(st.sweep_stretches)}
    clipped["ratio_to_one_length"] = round(clipped["device_ms"] / best["device_ms"], 2)
    best["clipped_1pct"] = clipped
    # ... and with 0.5 % of the reads LENGTHENED by 1...20 bases as well (deletions): longer reads leave the near-uniform
    # route; the mixed-span walk in speculative stretches (round 4: the rule is how deep the data is in standard
    # deviations, not that one length dominates; one chain per contig was 14.5 s).  Parity:
    # tests/test_gpu_full_size.py::test_cfg5_real_share_with_longer_reads
    e3 = synthetic.lengthened_mix(d_e.cpu().numpy().view(np.uint32), d_e.cpu().numpy().view(np.uint32), offs, lengths, 0.005)
    d_e.copy_(torch.from_numpy(e3.view(np.int32)))
    del e3
    longer = None
    for _ in range(2):
        st = solver.solve_device(d_s.data_ptr(), d_e.data_ptr(), n, lengths, 50, d_m.data_ptr(),
                                 contig_read_offsets=offs, stream=stream)
        if longer is None or st.ms_total < longer["device_ms"]:
            longer = {"device_ms": round(float(st.ms_total), 3), "path": int(st.path), "kept": int(st.n_kept),
                      "near_uniform_giveup": int(st.near_uniform_giveup), "stretches": int(st.sweep_stretches),
                      "speculative_boundaries": int(st.spec_boundaries), "boundaries_that_disagreed": int(st.spec_mismatches)}
    longer["ratio_to_one_length"] = round(longer["device_ms"] / best["device_ms"], 2)
    best["clipped_1pct_and_half_a_percent_longer"] = longer
    b_alg = algorithmic_bytes(n, int(lengths.sum()), lengths.size)
    best.update({"contigs_of_the_whole_genome": [int(c) for c in share], "reads": n,
                 "positions": int(lengths.sum()), "longest_contig": int(lengths.max()), "max_coverage": 50,
                 "reads_per_rank_of_the_assignment": [int(sum(2 * synthetic.wgs_shape(int(1.5e9), int(0.5e9))[1][c] for c in o)) for o in owned],
                 "Mreads_per_s": round(n / best["device_ms"] / 1e3, 1),
                 "whole_solve_frac": round(b_alg / (best["device_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 5),
                 "note": "one solve alone on the device (HIP events), inputs resident; not the headline workload"})
    return best


def clipped_configs(pkg, torch, dev, solver, stream, d_starts, d_ends, n_reads, lengths, offs, M, solver2=None):
    """What one read of another length costs (BamApi derives a read's span from its CIGAR, libs/bam-api/src/read.cpp:
    11-13: real BAMs are never of one length; every BASELINE config is).  cfg4 with 1 % of the reads soft-clipped by
    1...50 bases, and cfg3's shape (30 M amplicon reads, M = 200) with 15 % clipped: device ms of one solve alone on
    the mixed-span route, next to the same reads with one length.  Never `value`; parity of the routes:
    tests/test_gpu_baseline_configs.py, tests/test_gpu_parity.py."""
    synthetic = importlib.import_module("genome-downsampler_amd.synthetic")
    out = {}
    # cfg4, 1 % clipped
    s = d_starts.cpu().numpy().view(np.uint32)
    e = d_ends.cpu().numpy().view(np.uint32)
    s2, e2 = synthetic.clipped_mix(s, e, 0.01)
    d_s = torch.from_numpy(s2.view(np.int32)).to(dev)
    d_e = torch.from_numpy(e2.view(np.int32)).to(dev)
    d_m = torch.zeros(pkg.mask_words(n_reads), dtype=torch.int64, device=dev)
    ms = []
    for _ in range(3):
        st = solver.solve_device(d_s.data_ptr(), d_e.data_ptr(), n_reads, lengths, M, d_m.data_ptr(),
                                 contig_read_offsets=offs, stream=stream)
        ms.append(float(st.ms_total))
    kept_near = int(st.n_kept)
    # the same call with two solves in flight (two contexts, the two-phase entry), as the headline's timed region runs
    # cfg4: on this route _begin waits for the device several times, so little overlaps (include/qmcp_hip.h)
    pipelined_ms = None
    if solver2 is not None:
        d_m2 = torch.zeros(pkg.mask_words(n_reads), dtype=torch.int64, device=dev)
        pair, bufs = [solver, solver2], [d_m, d_m2]
        for warm in (True, False):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            steps = 2 if warm else 6
            for k in range(steps):
                sv = pair[k % 2]
                if k >= 2:
                    sv.solve_end()
                sv.solve_device_begin(d_s.data_ptr(), d_e.data_ptr(), n_reads, lengths, M, bufs[k % 2].data_ptr(),
                                      contig_read_offsets=offs, stream=stream)
            for sv in pair:
                sv.solve_end()
            torch.cuda.synchronize(dev)
            pipelined_ms = (time.perf_counter() - t0) / steps * 1e3
        del d_m2
    out["cfg4_1pct_clipped"] = {"device_ms": round(min(ms), 3), "path": int(st.path), "min_span": int(st.min_span),
                                "max_span": int(st.max_span), "stretches": int(st.sweep_stretches),
                                "kept": kept_near, "exceptions": int(st.near_uniform_exceptions),
                                "exceptions_kept": int(st.near_uniform_selected), "sweeps": int(st.near_uniform_rounds),
                                "pipelined_ms": round(pipelined_ms, 3) if pipelined_ms else None,
                                "note": "cfg4 with 1 % of the reads shortened by 1...50 bases: near-uniform route (path 3: "
                                        "the one-span sweep over the regular reads, the short ones it is seen to want "
                                        "selected and certified against the next sweep); mixed_route_device_ms is the same "
                                        "call on the mixed-span event sweep (options.near_uniform = -1), same kept set"}
    with solver.options(near_uniform=-1):
        st = solver.solve_device(d_s.data_ptr(), d_e.data_ptr(), n_reads, lengths, M, d_m.data_ptr(),
                                 contig_read_offsets=offs, stream=stream)
    out["cfg4_1pct_clipped"]["mixed_route_device_ms"] = round(float(st.ms_total), 3)
    out["cfg4_1pct_clipped"]["mixed_route_kept"] = int(st.n_kept)
    # ... and with 0.5 % of the reads LENGTHENED by 1...20 bases as well (deletions): what VERDICT round 3 asked to see at
    # <= 3 x the one-length solve and round 4 did not build -- longer reads leave the near-uniform route, and at 18.75 x M
    # the mixed-span walk is one chain per contig (lab/long_reads_lemma.py has the next step)
    e3 = synthetic.lengthened_mix(e2, e2, offs, lengths, 0.005)
    d_e.copy_(torch.from_numpy(e3.view(np.int32)))
    del e3
    st = solver.solve_device(d_s.data_ptr(), d_e.data_ptr(), n_reads, lengths, M, d_m.data_ptr(),
                             contig_read_offsets=offs, stream=stream)
    out["cfg4_1pct_clipped_and_half_a_percent_longer"] = {
        "device_ms": round(float(st.ms_total), 3), "path": int(st.path), "near_uniform_giveup": int(st.near_uniform_giveup),
        "kept": int(st.n_kept), "stretches": int(st.sweep_stretches),
        "note": "not built: reads longer than the dominant length on deep data take the mixed-span walk, one chain per contig"}
    del d_s, d_e, d_m
    # cfg3's shape: 30 M amplicon reads, one length vs 85 / 15 mix
    a, b, _, _, _ = synthetic.amplicon_reads(15_000_000)
    res = {}
    for name, (x, y) in (("one_length", (a, b)), ("clipped_tail_15pct", synthetic.clipped_mix(a, b, 0.15))):
        d_s = torch.from_numpy(x.view(np.int32)).to(dev)
        d_e = torch.from_numpy(y.view(np.int32)).to(dev)
        d_m = torch.zeros(pkg.mask_words(x.size), dtype=torch.int64, device=dev)
        ms = []
        for _ in range(3):
            st = solver.solve_device(d_s.data_ptr(), d_e.data_ptr(), x.size, np.array([29_903], np.uint32), 200,
                                     d_m.data_ptr(), stream=stream)
            ms.append(float(st.ms_total))
        res[name] = {"device_ms": round(min(ms), 3), "path": int(st.path), "kept": int(st.n_kept)}
    res["ratio"] = round(res["clipped_tail_15pct"]["device_ms"] / res["one_length"]["device_ms"], 2)
    res["note"] = "30 M amplicon reads on 29 903 bases, M = 200 (no FILTER): mixed-span route over one-length route"
    out["cfg3_clipped_tail"] = res
    del d_s, d_e, d_m
    # long SHALLOW contigs with a tail of clipped reads (a low-pass genome's shape): two contigs of 10^7 positions at
    # 1.5 x M, 1 % clipped -- the near-uniform route with its sweeps in stretches, the same reads
    # of one length, and the mixed-span walk
    L, pairs = 10_000_000, 5_000_000
    parts = [pkg.reads_gen(0, pairs, L, seed=4242 + c) for c in range(2)]
    a = np.concatenate([p[0] for p in parts]); b = np.concatenate([p[1] for p in parts])
    a2, b2 = synthetic.clipped_mix(a, b, 0.01)
    offs2 = np.arange(3, dtype=np.uint64) * np.uint64(2 * pairs)
    len2 = np.full(2, L, np.uint32)
    d_m = torch.zeros(pkg.mask_words(a.size), dtype=torch.int64, device=dev)
    res = {}
    for name, (x, y, near, reps) in (("one_length", (a, b, 0, 3)), ("clipped_1pct", (a2, b2, 0, 3)), ("clipped_1pct_mixed_route", (a2, b2, -1, 1))):
        d_s = torch.from_numpy(x.view(np.int32)).to(dev)
        d_e = torch.from_numpy(y.view(np.int32)).to(dev)
        ms = []
        with solver.options(near_uniform=near):
            for _ in range(reps):
                st = solver.solve_device(d_s.data_ptr(), d_e.data_ptr(), x.size, len2, M, d_m.data_ptr(),
                                         contig_read_offsets=offs2, stream=stream)
                ms.append(float(st.ms_total))
        res[name] = {"device_ms": round(min(ms), 3), "path": int(st.path), "kept": int(st.n_kept),
                     "stretches": int(st.sweep_stretches)}
        if name == "clipped_1pct":
            res[name].update(exceptions=int(st.near_uniform_exceptions), exceptions_kept=int(st.near_uniform_selected),
                             sweeps=int(st.near_uniform_rounds), giveup=int(st.near_uniform_giveup))
            res[name]["mask_sha1"] = hashlib.sha1(d_m.cpu().numpy().tobytes()).hexdigest()[:16]
        if name == "clipped_1pct_mixed_route":
            res["same_mask"] = res["clipped_1pct"]["mask_sha1"] == hashlib.sha1(d_m.cpu().numpy().tobytes()).hexdigest()[:16]
        del d_s, d_e
    res["ratio"] = round(res["clipped_1pct"]["device_ms"] / res["one_length"]["device_ms"], 2)
    res["note"] = "two contigs of 10^7 positions, 2 x 10^7 reads of 150 at 1.5 x M (M = 100), 1 % clipped by 1...50 bases"
    out["long_shallow_1pct_clipped"] = res
    return out


def cfg3_full(pkg, solver):
    """configs[2] at full size (15 M amplicon pairs on a 29 903-base genome, a tenth of the pairs straddling two
    amplicons, M = 200) through the fused host entry -- FILTER, pair compaction, solve, mate completion, keep
    mask over the original read indices -- outside the timed region and never `value`: wall clock of the
    call (PCIe included), best of three.  Parity: tests/test_gpu_full_size.py (== composed oracle)."""
    synthetic = importlib.import_module("genome-downsampler_amd.synthetic")
    s, e, a0, a1, straddle = synthetic.amplicon_reads(15_000_000)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        solver.filter_solve(s, e, 29_903, 200, amp_starts=a0, amp_ends=a1, complete_pairs=True)
        wall = time.perf_counter() - t0
        st = solver.last_stats
        if best is None or wall * 1e3 < best["host_call_ms"]:
            best = {"host_call_ms": round(wall * 1e3, 3), "solve_device_ms": round(float(st.ms_total), 3),
                    "reads_solved": int(st.n_reads), "kept_before_mates": int(st.n_kept),
                    "columns_sent": int(st.columns_sent)}
    best.update({"reads": int(s.size), "pairs_straddling": int(straddle.sum()), "max_coverage": 200,
                 "Mreads_per_s_host_call": round(s.size / best["host_call_ms"] / 1e3, 1),
                 "note": "host arrays in -> host keep mask out; not the headline workload"})
    return best


def cpu_baseline(pkg, workload):
    """oracle (single thread) on a bounded sample of the same workload: one contig"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py
    n_contigs, pairs, L, rl, M = WORKLOADS[workload]
    n_sample = min(n_contigs, 3)
    dt, n_done, masks = 0.0, 0, []
    for c in range(n_sample):
        s, e = pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, rl, seed=12345 + c)
        t0 = time.perf_counter()
        # the reference's two host stages: per-base coverage build (create_b_function) ...
        oracle_py.b_function(s, e, L, M)
        # ... and the selection (SimpleMaxFlow::Solve + obtain_sequence -> canonical maximum flow)
        mask = oracle_py.solve(s, e, L, M)
        dt += time.perf_counter() - t0
        n_done += s.size
        masks.append(mask)
    return {
        "value": round(n_done / dt / 1e6, 3), "unit": "Mreads/s", "cores": 1, "kind": "port",
        "sample": f"{n_sample} of {n_contigs} contigs of the workload ({n_done} reads, L={L} each, "
                  f"M={M}): per-base coverage build + canonical selection, {dt:.2f} s on one "
                  "thread; OR-Tools-backed reference binary not runnable (dependency unavailable)",
        "host_cpus": os.cpu_count(),
    }, masks


def spawn_ranks(n_ranks):
    """`python bench.py --gpus N` without a launcher: run `python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 --master-port <free port> bench.py <the same arguments>` as a child
    process, pass its output through (rank 0 prints the one JSON line) and return its exit code."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # the host driver only supports dmabuf IPC
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cfg4")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the host-entry, plugin-entry and CPU-baseline legs (counter passes: every "
                         "launch of the run is then the workload's own)")
    ap.add_argument("--mode", choices=["per-gpu", "sharded"], default="per-gpu",
                    help="N > 1: the workload per GPU (weak scaling) or one workload sharded by contig (strong)")
    ap.add_argument("--exchange", choices=["gather", "all_gather", "none"], default="gather",
                    help="N > 1: the keep masks go to rank 0 (what a caller needs: one Solution; N/8 bytes per rank over "
                         "rank 0's seven links side by side), to every rank, or nowhere (none: the solves alone, to "
                         "separate them from the exchange in a scaling run)")
    ap.add_argument("--in-flight", type=int, default=2, choices=[1, 2, 3, 4],
                    help="solves kept in flight per GPU (one solver context each; 1 = one at a time)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the keep mask(s) the last timed step produced to DIR/*.npy (see dump_outputs)")
    # rehearsal knobs (not used by the driver): run several ranks on ONE GPU over gloo to
    # exercise the N > 1 plumbing on a single-GPU box
    ap.add_argument("--dist-backend", default="nccl", help=argparse.SUPPRESS)
    ap.add_argument("--single-device", action="store_true", help=argparse.SUPPRESS)
    # one rank, but through the collective library all the same: init_process_group("nccl") and the mask gather on
    # a one-rank RCCL communicator -- the only way a one-GPU box can execute the RCCL calls of the N > 1 path
    ap.add_argument("--force-dist", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # Plain `python bench.py --gpus N`: start the N ranks ourselves, as a CHILD process and before torch or
        # the GPU is touched (a process that has initialised the GPU must never be replaced by another).
        sys.exit(spawn_ranks(args.gpus))

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with {args.gpus} ranks "
                         f"(WORLD_SIZE={world})")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    if args.single_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            import socket
            with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sock:
                sock.bind(("127.0.0.1", 0))
                os.environ.setdefault("MASTER_PORT", str(sock.getsockname()[1]))
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.dist_backend, rank=rank, world_size=world)

    pkg = importlib.import_module("genome-downsampler_amd")
    sharding = importlib.import_module("genome-downsampler_amd.sharding")
    n_contigs_job, pairs, L, rl, M = WORKLOADS[args.workload]
    sharded = args.mode == "sharded" and world > 1
    if sharded:
        # one workload for the whole job: contigs dealt by cost (reads + the longest chain of a rank)
        owned = sharding.assign_contigs([2 * pairs] * n_contigs_job, world, contig_lengths=[L] * n_contigs_job,
                                        read_length=rl, max_coverage=M)
        my_contigs = owned[rank]
        seeds = [12345 + c for c in my_contigs]
    else:
        owned = None
        my_contigs = list(range(n_contigs_job))
        seeds = [12345 + n_contigs_job * rank + c for c in my_contigs]
    n_contigs = len(my_contigs)
    ss, ee = [], []
    for sd in seeds:
        s, e = pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, rl, seed=sd)
        ss.append(s)
        ee.append(e)
    starts = np.concatenate(ss) if ss else np.zeros(0, np.uint32)
    ends = np.concatenate(ee) if ee else np.zeros(0, np.uint32)
    n_reads = starts.size
    offs = (np.arange(n_contigs + 1, dtype=np.uint64) * np.uint64(2 * pairs))
    lengths = np.full(max(n_contigs, 1), L, dtype=np.uint32)[:n_contigs] if n_contigs else np.full(1, 0, np.uint32)
    if n_contigs == 0:
        offs = np.zeros(2, np.uint64)
    # gathered masks are padded to the largest share (equal shares in per-gpu mode)
    share_reads = max(len(o) for o in owned) * 2 * pairs if sharded else n_reads
    words = pkg.mask_words(share_reads)

    d_starts = torch.from_numpy(starts.view(np.int32)).to(dev)
    d_ends = torch.from_numpy(ends.view(np.int32)).to(dev)
    # Four mask buffers in rotation: solve s writes buffer s % 4; its gather (RCCL, its own stream) is
    # started when the solve is collected one or two steps later and waited for before buffer s % 4
    # is written again.
    n_buf = max(4, args.in_flight + 2)
    d_masks = [torch.zeros(words, dtype=torch.int64, device=dev) for _ in range(n_buf)]
    d_alls = [torch.zeros(words * world, dtype=torch.int64, device=dev) for _ in range(n_buf)] \
        if use_dist else None
    depth = args.in_flight
    solvers = [pkg.Solver(local_rank) for _ in range(depth)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    gathers = [None] * n_buf        # async gather handles per mask buffer
    in_flight = [None] * depth      # per solver context: the mask buffer of its pending solve
    step_no = [0]
    last_buf = [0]

    def collect(slot):
        """wait for the solve pending on context `slot`, then start the gather of its mask"""
        b = in_flight[slot]
        if b is None:
            return
        solvers[slot].solve_end()
        in_flight[slot] = None
        last_buf[0] = b
        if use_dist and args.exchange != "none":
            # the path's one exchange: gather of the keep bitmasks (N/8 bytes per rank) over xGMI
            if args.exchange == "all_gather":
                gathers[b] = dist.all_gather_into_tensor(d_alls[b], d_masks[b], async_op=True)
            else:
                gathers[b] = dist.gather(d_masks[b], gather_list=list(d_alls[b].chunk(world)) if rank == 0 else None,
                                         dst=0, async_op=True)

    def step():
        s_no = step_no[0]
        step_no[0] += 1
        slot, b = s_no % depth, s_no % n_buf
        collect(slot)                      # this context's previous solve (depth steps ago)
        if gathers[b] is not None:         # buffer b: gathered since n_buf steps ago
            gathers[b].wait()
            gathers[b] = None
        solvers[slot].solve_device_begin(d_starts.data_ptr(), d_ends.data_ptr(), n_reads, lengths, M,
                                         d_masks[b].data_ptr(), contig_read_offsets=offs, stream=stream)
        in_flight[slot] = b

    def fence():
        for k in range(depth):
            collect((step_no[0] + k) % depth)   # oldest first
        for b in range(n_buf):
            if gathers[b] is not None:
                gathers[b].wait()
                gathers[b] = None
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def all_kernel_times():
        out = {}
        for sv in solvers:
            for name, (n, ms) in sv.kernel_times().items():
                a = out.get(name, (0, 0.0))
                out[name] = (a[0] + n, a[1] + ms)
        return out

    for _ in range(args.warmup):
        step()
    # Timed region: HIP events (recorded by the library on the stream the kernel is launched on)
    # bracket the dominant kernel -- the selection sweep -- only: every bracket costs a few
    # microseconds of device idle time, and seven of them per step are 2 % of a cfg4 solve.
    fence()
    for sv in solvers:
        sv.set_profiling(2)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    ktimes_live = all_kernel_times()
    st_live = solvers[(step_no[0] - 1) % depth].last_stats  # of the last timed solve
    if args.dump_outputs and rank == 0:
        # the last timed step's mask buffer, before the steps below write every buffer again; with an exchange, rank 0
        # holds every rank's mask (each padded to `words`)
        b = (step_no[0] - 1) % n_buf
        if use_dist and args.exchange != "none":
            masks = d_alls[b].cpu().numpy().view(np.uint64).reshape(world, words)
            sizes = [len(o) * 2 * pairs for o in owned] if sharded else [n_reads] * world
        else:
            masks, sizes = [d_masks[b].cpu().numpy().view(np.uint64)], [n_reads]
        dump_outputs(args.dump_outputs, masks, sizes)
    # Per-kernel breakdown: the same step a few more times, untimed, with every kernel bracketed.
    breakdown_steps = min(args.steps, 5)
    for sv in solvers:
        sv.set_profiling(1)
    for _ in range(breakdown_steps):
        step()
    fence()
    ktimes = all_kernel_times()
    for sv in solvers:
        sv.set_profiling(0)
    # one solve alone on the device: its latency, as opposed to the pipelined rate
    solvers[0].solve_device(d_starts.data_ptr(), d_ends.data_ptr(), n_reads, lengths, M,
                            d_masks[0].data_ptr(), contig_read_offsets=offs, stream=stream)
    alone_ms = float(solvers[0].last_stats.ms_total)
    d_mask = d_masks[0]
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # did the collective library see every rank?  (answerable from the line alone)
    rccl_info = None
    if use_dist:
        names = [None] * world
        dist.all_gather_object(names, {"rank": rank, "device": torch.cuda.get_device_name(dev),
                                       "local_rank": local_rank})
        rccl_info = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "ranks": names}
    if sharded:
        total_reads = n_contigs_job * 2 * pairs      # one workload for the whole job
    else:
        total_reads = n_reads * world
    value = total_reads * args.steps / elapsed / 1e6
    st = st_live

    out = None
    if rank == 0:
        b_alg = algorithmic_bytes(n_reads, n_contigs * L, n_contigs)
        # dominant kernel: largest summed duration per step (the solves of a pipelined run overlap, so
        # durations do not add up to the step time)
        dom_name, (dom_launches, dom_ms) = max(ktimes.items(), key=lambda kv: kv[1][1])
        dom_where = "breakdown steps after the timed region"
        if dom_name in ktimes_live:  # the dominant kernel is the one bracketed in the timed region
            dom_launches, dom_ms = ktimes_live[dom_name]
            dom_where = "timed region"
        dom_avg_ms = dom_ms / dom_launches
        achieved = b_alg / (dom_avg_ms * 1e-3) / 1e9
        step_ms = elapsed / args.steps * 1e3
        traffic, traffic_source, total_traffic = None, None, None
        try:
            # collected with the same number of solves in flight as this run (profiles/collect.sh makes one file per
            # depth); a run at another depth, or sharded, reports no traffic rather than another configuration's
            pmc_file = PMC_TRAFFIC_FILE.format(workload=args.workload, depth=depth)
            pmc = json.load(open(pmc_file)) if not sharded else {}
            traffic = pmc.get(dom_name, {}).get("hbm_bytes_per_launch")
            total_traffic = pmc.get("_total", {}).get("hbm_bytes_per_solve")
            if pmc:
                traffic_source = ("constant read from " + os.path.relpath(pmc_file, ROOT)
                                  + " (" + str(pmc.get("_source", "rocprofv3 --pmc passes, profiles/collect.sh")) + "); not measured in this run")
        except (OSError, ValueError):
            pass
        # what bounds the dominant kernel itself: the event sweep's chain wave is a serial dependency
        # chain (issue latency of one wave), the streaming kernels are HBM-bound
        latency_bound = dom_name.startswith("k_sweep")
        out = {
            "metric": "Mreads/s selected at target coverage M=100",
            "value": round(value, 2), "unit": "Mreads/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(step_ms, 4),
            "higher_is_better": True, "scaling": "strong" if sharded else "weak", "vs_baseline": None,
            # SURVEY 8(d)'s own definition, N / time of one solve() alone on the device (HIP events, nothing else in
            # flight), beside the pipelined rate above -- per GPU, rank 0's
            "value_single_solve": round(n_reads / (alone_ms * 1e-3) / 1e6, 2) if alone_ms > 0 else None,
            "single_solve_ms": round(alone_ms, 4),
            "dtype": "u32", "data": "synthetic",
            "config": {
                "workload": (f"{args.workload} sharded over {world} GPUs by contig (one workload for the job): "
                             if sharded else f"{args.workload} per GPU: ")
                            + f"{n_contigs_job} contigs x rand_reads_uniform("
                            f"{pairs} pairs, L={L}, len={rl}), {n_contigs_job * 2 * pairs} reads, M={M}; "
                            "device-resident reads -> device keep bitmask"
                            + (f"; + RCCL {args.exchange} of the keep masks" + (" at rank 0" if args.exchange == "gather" else "") + ", overlapped with the following "
                               "solves (all completed inside the timed region)"
                               if use_dist else ""),
                "multi_gpu_mode": args.mode if world > 1 else "single GPU",
                "exchange": args.exchange if use_dist else None,
                "rccl_ranks": rccl_info,
                "solves_in_flight_per_gpu": depth,
                "reads_per_gpu": int(n_reads), "contigs_per_gpu": n_contigs, "max_coverage": M,
                "path": {1: "uniform-span sweep", 2: "mixed-span event sweep", 3: "near-uniform route"}.get(st.path),
                "kept_reads_per_gpu": int(st.n_kept),
                # the selection chain's serial work (event-driven sweep): blocks that changed the kept profile cost
                # ~170 instructions of one wave each, sixteen blocks tested without a change ~60
                "sweep_blocks_changed": int(st.sweep_blocks_changed), "sweep_blocks": int(st.sweep_blocks),
            },
            "roofline": {
                "bound": "hbm", "kernel": dom_name, "achieved": round(achieved, 2),
                "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 5),
                "traffic": traffic, "traffic_source": traffic_source,
                "algorithmic_bytes_per_launch": b_alg,
                "avg_launch_ms": round(dom_avg_ms, 4), "launches": dom_launches,
                "kernel_bound": "latency (one wave's dependency chain; see kernel_own_GBps)" if latency_bound else "hbm",
                "kernel_own_GBps": (round(traffic / (dom_avg_ms * 1e-3) / 1e9, 2) if traffic else None),
                "bytes_are_of": "rank 0's share of the job" if sharded else "one GPU's whole workload",
                "whole_solve": {
                    "note": "algorithmic bytes of one solve over the time one solve takes: pipelined "
                            "(ms_per_step, two in flight) and alone on the device (HIP events)",
                    "pipelined_ms": round(step_ms, 4),
                    "achieved": round(b_alg / (step_ms * 1e-3) / 1e9, 2),
                    "frac": round(b_alg / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 5),
                    "alone_device_ms": round(alone_ms, 4),
                    "alone_frac": round(b_alg / (alone_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 5),
                    "hbm_traffic_per_solve": total_traffic,
                },
                "measured_in": dom_where,
                "kernels_ms_per_step": {k: round(ms / breakdown_steps, 4) for k, (_, ms) in
                                        sorted(ktimes.items(), key=lambda kv: -kv[1][1])},
                "kernels_measured_in": f"{breakdown_steps} extra steps after the timed region, "
                                       "every kernel bracketed (solves overlap: the sum exceeds a step)",
            },
        }
        if world == 1 and not args.no_extras:
            # T_e2e, outside the timed region and never `value`: host arrays in ->
            # host keep mask out through qmcp_hip_solve_host (pageable H2D of 8 B/read, solve, D2H of
            # the mask), best of three
            e2e = []
            for _ in range(3):
                t1 = time.perf_counter()
                solvers[0].solve(starts, ends, lengths, M, contig_read_offsets=offs)
                e2e.append(time.perf_counter() - t1)
            out["host_entry"] = {"e2e_ms": round(min(e2e) * 1e3, 3),
                                 "Mreads_per_s": round(n_reads / min(e2e) / 1e6, 1),
                                 "h2d_ms": round(float(solvers[0].last_stats.ms_h2d), 3),
                                 "d2h_ms": round(float(solvers[0].last_stats.ms_d2h), 3),
                                 "note": "PCIe-inclusive; reported beside, never as, value"}
        if world == 1 and not args.no_extras:
            # The plugin boundary itself (SURVEY section 8d T_e2e; the span src/app.cpp:132-139 brackets):
            # BamApi holding SOAPairedReads (size_t columns) -> QuasiMcpHipSolver::solve -> Solution
            # (vector<size_t>), one contig -- the reference is single-contig.  Best of three.
            best = None
            for _ in range(3):
                kept, tms = pkg.plugin_solve_timed("quasi-mcp-hip", ss[0], ee[0], L, M)
                if best is None or tms["solve_call_ms"] < best["solve_call_ms"]:
                    best = tms
            pcie_ms = 8.0 * ss[0].size / (n_reads * 8.0 / (float(solvers[0].last_stats.ms_h2d) * 1e-3)) * 1e3 \
                if float(solvers[0].last_stats.ms_h2d) > 0 else None
            best.update({"reads": int(ss[0].size), "kept": int(kept.size),
                         "Mreads_per_s": round(ss[0].size / best["solve_call_ms"] / 1e3, 1),
                         "pcie_floor_ms": round(pcie_ms, 3) if pcie_ms else None,
                         "note": "one contig of the workload through SolverManager -> Solver::solve(M, BamApi&); "
                                 "pcie_floor_ms = 8 B/read at the pageable-copy rate host_entry measured"})
            out["plugin_entry"] = best
        if world == 1 and not args.no_extras and args.workload == "cfg4":
            out["other_configs"] = {"cfg3_full_size": cfg3_full(pkg, solvers[1 % depth]),
                                    "cfg5_share_one_gpu": cfg5_share(pkg, torch, dev, solvers[0], stream),
                                    "cfg5_real_share_heaviest_rank": cfg5_real_share(pkg, torch, dev, solvers[0], stream)}
            out["other_configs"].update(clipped_configs(pkg, torch, dev, solvers[0], stream, d_starts, d_ends,
                                                        n_reads, lengths, offs, M,
                                                        solver2=solvers[1] if depth > 1 else None))
        if world == 1 and not args.no_cpu_baseline and not args.no_extras:
            base, oracle_masks = cpu_baseline(pkg, args.workload)
            out["cpu_baseline"] = base
            # parity check on EVERY sampled contig: GPU bits == oracle bits
            got_bits = np.unpackbits(d_mask.cpu().numpy().view(np.uint8), bitorder="little")
            same = True
            for k, om in enumerate(oracle_masks):
                want_bits = np.unpackbits(om.view(np.uint8), bitorder="little")[:2 * pairs]
                same = same and np.array_equal(got_bits[k * 2 * pairs:(k + 1) * 2 * pairs], want_bits)
            out["parity_vs_oracle_on_sample"] = bool(same)
            out["parity_contigs_compared"] = len(oracle_masks)
        print(json.dumps(out), flush=True)
    for sv in solvers:
        sv.close()
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
