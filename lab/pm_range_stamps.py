"""cfg4 (8 contigs x 12.5 M reads, M = 100), one solve alone, on a -DQMCP_PM_STAMP build of the library: where the two
per-range kernels' workgroups spend their time -- per-phase medians (and the 10th / 90th percentile) over the ranges,
in microseconds, of the LAST solve.  Read the shares, not the lengths: the stamps' waits forbid overlaps the product has.
usage: lab/build_variant.sh stamp "-DQMCP_PM_STAMP" && QMCP_HIP_LIB=lab/variants/stamp/libqmcp_hip.so python lab/pm_range_stamps.py"""
import ctypes, hashlib, importlib, os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
pkg = importlib.import_module('genome-downsampler_amd')
import torch
ss, ee = [], []
for c in range(8):
    a, b = pkg.reads_gen(0, 6_250_000, 1_000_000, seed=12345 + c); ss.append(a); ee.append(b)
S = np.concatenate(ss); E = np.concatenate(ee)
offs = np.arange(9, dtype=np.uint64) * 12_500_000
lengths = np.full(8, 1_000_000, np.uint32)
sv = pkg.Solver(0)
dS = torch.from_numpy(S.view(np.int32)).cuda(); dE = torch.from_numpy(E.view(np.int32)).cuda()
dM = torch.zeros((S.size + 63) // 64, dtype=torch.int64, device="cuda")
lib = ctypes.CDLL(pkg.HIP_LIB_PATH)
if not hasattr(lib, "qmcp_lab_pm_stamps"):
    sys.exit("this library has no stamps: build it with -DQMCP_PM_STAMP and name it in QMCP_HIP_LIB")
PHASES = {0: [("entry -> first count", 0, 1), ("counting loop", 1, 2), ("scan", 2, 3), ("boff store issued", 3, 4), ("whole", 0, 4)],
          1: [("entry -> first draw", 0, 1), ("walk loop", 1, 2), ("tail (settling)", 2, 3), ("whole", 0, 3)]}
rows = {0: {}, 1: {}}
for it in range(8):
    sv.solve_device(dS.data_ptr(), dE.data_ptr(), S.size, lengths, 100, dM.data_ptr(), contig_read_offsets=offs)
    torch.cuda.synchronize()
    if it < 3:
        continue
    st = np.zeros(2 * 256 * 8, np.uint64)
    assert lib.qmcp_lab_pm_stamps(st.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong))) == 0
    st = st.reshape(2, 256, 8).astype(np.float64)
    for k in (0, 1):
        t = st[k][st[k][:, 5] == 1]
        us_per_tick = (t[:, 7] - t[:, 6]) / 100.0 / (t[:, 4 if k == 0 else 3] - t[:, 0])  # 100 MHz clock beside the shader clock
        for name, a, b in PHASES[k]:
            rows[k].setdefault(name, []).append(np.percentile((t[:, b] - t[:, a]) * np.median(us_per_tick), [50, 10, 90]))
        rows[k].setdefault("shader clock, MHz", []).append(np.full(3, 1.0 / np.median(us_per_tick)))
        rows[k].setdefault("workgroups", []).append(np.full(3, float(len(t))))
m = dM.cpu().numpy()
print("kept %d  mask sha1 %s" % (sv.last_stats.as_dict()['n_kept'], hashlib.sha1(m.tobytes()).hexdigest()[:12]))
for k, kern in ((0, "k_pm_offsets"), (1, "k_pm_walk")):
    print(kern + "  (median over ranges: median / 10th / 90th percentile, us; mean of 5 solves)")
    for name, v in rows[k].items():
        a = np.mean(np.array(v), axis=0)
        print("   %-24s %9.2f %9.2f %9.2f" % (name, a[0], a[1], a[2]))
