"""The depth track's time against the depth report's on the same reads and mask: cfg4's 10^8 reads shuffled over its 8
contigs (8 x 10^6 positions), the mask from the plain by-contig solve, both channels, no regions.  Medians of 5 after a
warm-up of ms_track and ms_report; the per-kernel times come from qmcp_hip_set_profiling in calls of their own.  A
count-only call (runs == NULL) is timed as well: it leaves out k_track_emit and the copy of the records to the host.
    python lab/depth_track_time.py [out.json] [scale]       (scale: reads and positions divided by it; default 1)"""
import ctypes as C
import datetime
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("genome-downsampler_amd")
out = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "depth_track_time.json")
scale = int(sys.argv[2]) if len(sys.argv) > 2 else 1

REPORT_STAGES = ("k_depth_events", "k_depth_chunk_sums + k_depth_spine", "k_depth_consume")
TRACK_STAGES = ("k_depth_events", "k_depth_chunk_sums + k_depth_spine", "k_track_count + k_track_spine", "k_track_emit")

n_contigs, pairs, L, M = 8, 6_250_000 // scale, 1_000_000 // scale, 100
rng = np.random.default_rng(4)
ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, 150, seed=12345 + c) for c in range(n_contigs)))
s, e = np.concatenate(ss), np.concatenate(ee)
ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
perm = rng.permutation(s.size)
s, e, ids = s[perm], e[perm], ids[perm]
n = s.size
lengths = np.full(n_contigs, L, np.uint32)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")
ds, de, di = dev(s), dev(e), dev(ids)
d_mask = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device="cuda:0")
torch.cuda.synchronize()
solver = pkg.Solver(0)
args = (ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M)
solver.solve_by_contig_device(*args, d_mask.data_ptr())


def track():
    return solver.depth_track_device(*args, d_keep_mask=d_mask.data_ptr())[1]


def report():
    return solver.depth_report_device(*args, d_keep_mask=d_mask.data_ptr()).stats


def count_only():
    st, n_runs = pkg.TrackStats(), C.c_uint64(0)
    rc = pkg._hip.qmcp_hip_depth_track_device(solver._ctx, C.c_void_p(args[0]), C.c_void_p(args[1]), C.c_void_p(args[2]), n,
                                              pkg._p32(lengths), n_contigs, C.c_void_p(d_mask.data_ptr()), M, None, None,
                                              None, 0, 3, 0, None, 0, C.byref(n_runs), None, C.byref(st))
    assert rc == 0
    return st


def stages(fn, names):
    runs = []
    for _ in range(5):
        solver.set_profiling(True)
        fn()
        kt = solver.kernel_times()
        runs.append({k: kt[k][1] for k in names if k in kt})
    solver.set_profiling(False)
    return {k: round(statistics.median(r.get(k, 0.0) for r in runs), 4) for k in names}


first = track()
report(); count_only()
ms_track = [float(track().ms_track) for _ in range(5)]
ms_report = [float(report().ms_report) for _ in range(5)]
ms_count = [float(count_only().ms_track) for _ in range(5)]
med = statistics.median
figures = {
    "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
    "reads": n, "contigs": n_contigs, "positions": n_contigs * L, "M": M, "flags": 3, "depth_cap": 0,
    "n_runs": int(first.n_runs), "positions_in_runs": int(first.positions_in_runs), "short_positions": int(first.short_positions),
    "record_bytes": int(first.n_runs) * 24,
    "ms_track_median": round(med(ms_track), 4), "ms_track_runs": [round(x, 4) for x in ms_track],
    "ms_track_count_only_median": round(med(ms_count), 4), "ms_track_count_only_runs": [round(x, 4) for x in ms_count],
    "ms_report_median": round(med(ms_report), 4), "ms_report_runs": [round(x, 4) for x in ms_report],
    "ratio_track_over_report": round(med(ms_track) / med(ms_report), 4),
    "ratio_count_only_over_report": round(med(ms_count) / med(ms_report), 4),
    "track_stages_ms_median": stages(track, TRACK_STAGES),
    "report_stages_ms_median": stages(report, REPORT_STAGES),
}
solver.close()
print("depth_track_time " + json.dumps(figures))
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write(json.dumps(figures, indent=1) + "\n")
