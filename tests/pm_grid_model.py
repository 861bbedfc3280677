"""The pass-major form's range grids on the host (genome-downsampler_amd/csrc/pm_grid_plan.h, through
tests/cpp/pm_grid_plan_driver.cpp under g++ alone): the plan of a shape, the reads' starts on the grid's axis, and the
wave-slots every range comes to under the producer's padding rule (tests/pass_major_model.py: every (range, pass) slice
rounded up to whole groups of 64 slots).  Shared by tests/test_pm_grid_model.py and lab/pm_grid_slots.py."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS = 8192
NO_CONTIG = 0xFFFFFFFF


def build_driver(directory):
    exe = os.path.join(str(directory), "pm_grid_plan_driver")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "pm_grid_plan_driver.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def plan(driver, lengths, reads, shift, want):
    """-> dict: aligned, n_ranges, aligned_ranges, heaviest_global, heaviest_aligned, pos0 / live / contig (per range),
    vbase (per contig, and the axis' end)"""
    line = " ".join(str(int(v)) for v in [shift, want, len(lengths), *lengths, *reads])
    out = subprocess.run([driver], input=line + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    head = dict(kv.split("=") for kv in out[0].split())
    g = {"aligned": int(head["aligned"]), "n_ranges": int(head["n_ranges"]), "aligned_ranges": int(head["aligned_ranges"]),
         "heaviest_global": float(head["heaviest_global"]), "heaviest_aligned": float(head["heaviest_aligned"])}
    for name, row in zip(("pos0", "live", "contig", "vbase"), out[1:5]):
        g[name] = np.array(row.split(), dtype=np.int64)
    return g


def virtual_starts(local_starts, contig_of_read, lengths, vbase):
    """the producer's key before it is cut into digit and position: the contig's place on the axis + the start, clamped
    into the contig"""
    last = np.maximum(np.asarray(lengths, np.int64) - 1, 0)
    return (vbase[contig_of_read] + np.minimum(local_starts, last[contig_of_read])).astype(np.uint32)


def wave_slots_per_range(vstart, shift, n_ranges):
    """sum over the passes of ceil(records of the (range, pass) slice / 64)"""
    n = vstart.size
    d = (vstart >> shift).astype(np.int64)
    assert d.max() < n_ranges <= 256
    P = np.arange(n, dtype=np.int64) // PASS
    counts = np.bincount(P * 256 + d, minlength=256 * int(P[-1] + 1)).reshape(-1, 256)
    return ((counts + 63) // 64).sum(axis=0)[:n_ranges]
