"""Wave-slots per range of the pass-major form under both range grids (csrc/pm_grid_plan.h), on the CPU: uniform starts,
the producer's padding rule (every (range, pass) slice rounded up to whole groups of 64 slots).  The per-range kernels
take as long as their heaviest range, so the number to look at is the heaviest range over the median.
usage: python lab/pm_grid_slots.py [--lengths 1000000,...] [--passes 300] [--shift 15] [--ranges]
(default: cfg4's shape -- 8 contigs of 10^6 positions, ranges of 2^15 -- at 300 passes per contig)"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pm_grid_model as gm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default=",".join(["1000000"] * 8))
    ap.add_argument("--passes", type=int, default=300, help="passes of 8 192 reads per contig")
    ap.add_argument("--shift", type=int, default=15)
    ap.add_argument("--ranges", action="store_true", help="print every range's wave-slots")
    a = ap.parse_args()
    lengths = [int(v) for v in a.lengths.split(",")]
    reads = [a.passes * gm.PASS] * len(lengths)
    rng = np.random.default_rng(1)
    contig = np.repeat(np.arange(len(lengths)), reads)
    local = np.concatenate([rng.integers(0, max(L, 1), size=k) for L, k in zip(lengths, reads)])
    with tempfile.TemporaryDirectory() as tmp:
        driver = gm.build_driver(tmp)
        auto = gm.plan(driver, lengths, reads, a.shift, 0)
        for want, name in ((-1, "global"), (1, "aligned")):
            g = gm.plan(driver, lengths, reads, a.shift, want)
            if want > 0 and not g["aligned"]:
                print(f"aligned: {g['aligned_ranges']} ranges do not fit one partition level")
                continue
            slots = gm.wave_slots_per_range(gm.virtual_starts(local, contig, lengths, g["vbase"]), a.shift, g["n_ranges"])
            med = float(np.median(slots[slots > 0]))
            heavy = np.argsort(slots)[::-1][:8]
            print(f"{name:8s}: {g['n_ranges']} ranges, heaviest {int(slots.max())} wave-slots = {slots.max() / med:.3f} x the median "
                  f"({med:.0f}); the host's estimate {g['heaviest_' + name]:.0f}; heaviest ranges "
                  + ", ".join(f"{int(r)} (+{100 * (slots[r] / med - 1):.0f} %)" for r in heavy))
            if a.ranges:
                print("   " + " ".join(str(int(v)) for v in slots))
        print("the host takes the", "aligned" if auto["aligned"] else "global", "grid")


if __name__ == "__main__":
    main()
