"""qmcp_hip_depth_report_*: every row, histogram bin and statistic bit for bit against tests/depth_model.py (numpy, written
from the contract); tables in LDS and through L2, aligned and unaligned columns, more than 10^6 reads, two position
batches, the solvers' guarantees seen through the report, device-found errors, _device == _host, and the time of a report
against the grouping stages of the plain by-contig solve."""
import json
import os
import statistics

import numpy as np
import pytest
import torch

import depth_model as dm
import multi_reference as mr
import quality_model as qm
import target_model as tm

pytestmark = pytest.mark.gpu

NO_CONTIG = 0xFFFFFFFF
GROUPING = ("k_bc_keys", "k_radix_hist_rec(by contig)", "scan_radix_hist(by contig, 3 kernels)",
            "k_radix_scatter_rec(by contig)", "k_bc_bounds", "k_bc_gather")
DEPTH_STAGES = ("k_depth_events", "k_depth_chunk_sums + k_depth_spine", "k_depth_consume")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")


def _dev_mask(mask):
    return torch.from_numpy(np.ascontiguousarray(mask, np.uint64).view(np.int64)).to("cuda:0")


def _report_device(solver, s, e, ids, lengths, M, mask=None, offset=0, stream=0, **kw):
    """through the _device entry; offset > 0 shifts the columns off 16-byte alignment (the 32-bit load path)"""
    pad = np.zeros(offset, np.uint32)
    ds, de, di = (_dev(np.concatenate([pad, x])) for x in (s, e, ids))
    dm_ = None if mask is None else _dev_mask(mask)
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr() + 4 * offset
    return solver.depth_report_device(ptr(ds), ptr(de), ptr(di), s.size, lengths, M,
                                      d_keep_mask=0 if dm_ is None else dm_.data_ptr(), stream=stream, **kw)


def _regions_kw(regions, padding=0):
    if regions is None:
        return {}
    return dict(target_offsets=regions[0], target_starts=regions[1], target_ends=regions[2], padding=padding)


def _random_call(rng, solver, n_contigs=None):
    n_contigs = int(rng.integers(1, 41)) if n_contigs is None else n_contigs
    s, e, ids, lengths = mr.random_by_contig(rng, n_contigs, max_reads_per_contig=int(rng.choice([40, 400, 2500])),
                                             unplaced=0.05)
    lengths = lengths.copy()
    for c in range(n_contigs):                                   # empty contigs: no reads and, some of them, no positions
        if not np.any(ids == c) and rng.random() < 0.5:
            lengths[c] = 0
    M = int(rng.choice([1, 3, 20, 50]))
    return s, e, ids, lengths, M


def test_random_calls_equal_the_model(pkg, solver):
    seen = dict(zero_length=0, unplaced=0, deficit=0, regions=0)
    for seed in range(64):
        rng = np.random.default_rng(7000 + seed)
        s, e, ids, lengths, M = _random_call(rng, solver)
        n = s.size
        kind = seed % 3
        if kind == 0:
            mask = solver.solve_by_contig(s, e, ids, _solvable(lengths), M)
        elif kind == 1:
            mask = rng.integers(0, 1 << 63, size=max(pkg.mask_words(n), 1), dtype=np.uint64) * np.uint64(2) + \
                rng.integers(0, 2, size=max(pkg.mask_words(n), 1), dtype=np.uint64)
        else:
            mask = None
        regions, padding = None, 0
        if seed % 2:
            regions = tm.random_regions(rng, lengths, max_regions=6, max_len=700)
            padding = int(rng.choice([0, 0, 30]))
        n_bins = (0, 1, 64, 4096)[(seed // 2) % 4]
        kw = dict(n_bins=n_bins, **_regions_kw(regions, padding))
        want = dm.report(s, e, ids, lengths, M, keep_mask=mask, **kw)
        info = f"seed {seed}"
        dm.assert_equal(solver.depth_report(s, e, ids, lengths, M, keep_mask=mask, **kw), want, info)
        if seed % 4 < 2:
            for offset in (0, 1):
                dm.assert_equal(_report_device(solver, s, e, ids, lengths, M, mask=mask, offset=offset, **kw), want,
                                (info, offset))
        assert solver.last_depth_stats.position_batches == 1
        if kind == 0 and regions is None:
            assert want["stats"]["deficit_positions"] == 0, info
        seen["zero_length"] += int(np.any(lengths == 0))
        seen["unplaced"] += int(np.any(ids == NO_CONTIG))
        seen["deficit"] += int(want["stats"]["deficit_positions"] > 0)
        seen["regions"] += int(len(want["region_rows"]) > 0)
    assert seen["zero_length"] > 10 and seen["unplaced"] > 30 and seen["deficit"] > 10 and seen["regions"] > 20, seen


def _solvable(lengths):
    """the solvers are not asked about contigs of length 0 here: those get one position (they hold no read)"""
    return np.maximum(lengths, 1).astype(np.uint32)


def test_tables_beyond_lds(pkg, solver):
    """more contigs than k_depth_events stages in LDS (2 048), so lengths and offsets are read through L2; and far more
    merged regions than any tile holds, aligned and unaligned columns"""
    rng = np.random.default_rng(11)
    n_contigs = 2500
    lengths = rng.integers(0, 900, size=n_contigs).astype(np.uint32)
    lengths[rng.random(n_contigs) < 0.1] = 0
    live = np.flatnonzero(lengths > 0)
    n = 300_000
    ids = live[rng.integers(0, live.size, size=n)].astype(np.uint32)
    L = lengths[ids].astype(np.int64)
    span = np.minimum(rng.integers(1, 200, size=n), L)
    s = (rng.random(n) * (L - span + 1)).astype(np.int64)
    e = s + span - 1
    ids[rng.random(n) < 0.05] = NO_CONTIG
    s, e = s.astype(np.uint32), e.astype(np.uint32)
    mask = rng.integers(0, 1 << 63, size=pkg.mask_words(n), dtype=np.uint64) * np.uint64(2)
    regions = pkg.window_regions(lengths, 37)                    # ~30 000 regions, adjacent ones merge: one per contig
    gaps = (regions[0], regions[1], np.minimum(regions[2], regions[1] + 30).astype(np.uint32))   # ... and these do not
    for reg in (regions, gaps):
        kw = dict(n_bins=64, **_regions_kw(reg))
        want = dm.report(s, e, ids, lengths, 20, keep_mask=mask, **kw)
        assert len(want["region_rows"]) == (live.size if reg is regions else int(reg[1].size))
        for offset in (0, 1):
            dm.assert_equal(_report_device(solver, s, e, ids, lengths, 20, mask=mask, offset=offset, **kw), want, offset)
    dm.assert_equal(solver.depth_report(s, e, ids, lengths, 20, keep_mask=mask, n_bins=4096),
                    dm.report(s, e, ids, lengths, 20, keep_mask=mask, n_bins=4096))


@pytest.mark.parametrize("case", ["plain_mask", "targets", "windows_500"])
def test_more_than_a_million_reads(pkg, solver, case):
    rng = np.random.default_rng(21)
    n_contigs, pairs, L, M = 3, 200_000, 700_000, 30
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, 150, seed=31 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
    perm = rng.permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    ids[rng.random(s.size) < 0.02] = NO_CONTIG
    lengths = np.full(n_contigs, L, np.uint32)
    assert s.size > 1_000_000
    if case == "plain_mask":
        mask = solver.solve_by_contig(s, e, ids, lengths, M)
        kw = dict(n_bins=256)
    elif case == "targets":
        regions = tm.random_regions(rng, lengths, max_regions=40, max_len=20_000, empty=0.0)
        mask = solver.solve_targets(s, e, ids, lengths, M, *regions, padding=100)
        kw = dict(n_bins=64, **_regions_kw(regions, 100))
    else:
        mask = rng.integers(0, 1 << 63, size=pkg.mask_words(s.size), dtype=np.uint64)
        kw = dict(n_bins=4096, **_regions_kw(pkg.window_regions(lengths, 500)))
    want = dm.report(s, e, ids, lengths, M, keep_mask=mask, **kw)
    got = solver.depth_report(s, e, ids, lengths, M, keep_mask=mask, **kw)
    dm.assert_equal(got, want, case)
    if case != "windows_500":
        assert got.valid and all(r["deficit_positions"] == 0 for r in (got.region_rows if case == "targets" else got.contig_rows))
    else:
        # (adjacent windows are adjacent regions: the table merges them, one row per contig, as the contract says)
        assert got.stats.regions_in == n_contigs * (L // 500) and len(got.region_rows) == n_contigs and not got.valid


def test_two_position_batches(pkg, solver):
    """two contigs of 1.2 x 10^9 positions do not fit one batch of 2^31 - 2.  The reads live in [0, 5 000) and in
    [D, D + 5 000) of each contig; the model runs on contigs of 10 000 positions with the second zone moved next to the
    first -- the stretches of depth 0 in between change `end`, `positions` and the bins of depth 0, nothing else."""
    rng = np.random.default_rng(5)
    big, D, M, n_bins = 1_200_000_000, 1_100_000_000, 4, 32
    s, e, ids, _ = mr.random_by_contig(rng, 2, max_reads_per_contig=3000, unplaced=0.05)
    placed = ids != NO_CONTIG
    lengths_small = np.array([10_000, 10_000], np.uint32)
    span = np.minimum(e.astype(np.int64) - s, 250)
    s_small = np.where(placed, rng.integers(0, 4_700, size=s.size) + 5_000 * rng.integers(0, 2, size=s.size), 0)
    e_small = np.where(placed, s_small + span, 0)
    far = s_small >= 5_000
    s_big = np.where(far, s_small - 5_000 + D, s_small).astype(np.uint32)
    e_big = np.where(far, e_small - 5_000 + D, e_small).astype(np.uint32)
    mask = rng.integers(0, 1 << 63, size=pkg.mask_words(s.size), dtype=np.uint64)
    want = dm.report(s_small, e_small, ids, lengths_small, M, keep_mask=mask, n_bins=n_bins)
    got = solver.depth_report(s_big, e_big, ids, [big, big], M, keep_mask=mask, n_bins=n_bins)
    assert got.stats.position_batches == 2 and got.stats.scope_positions == 2 * big
    assert got.stats.reads_placed == want["stats"]["reads_placed"] and got.stats.reads_kept == want["stats"]["reads_kept"]
    assert got.stats.deficit_positions == want["stats"]["deficit_positions"] > 0
    for r, w in zip(got.contig_rows.tolist(), want["contig_rows"]):
        assert w[3] == 0 and w[5] == 0                            # (the small contigs have positions of depth 0 too)
        assert tuple(int(x) for x in r) == (w[0], 0, big - 1) + w[3:8] + (big,) + w[9:]
    extra = 2 * (big - 10_000)
    for g, w in ((got.hist_in, want["hist_in"]), (got.hist_kept, want["hist_kept"])):
        assert int(g[0]) == int(w[0]) + extra and np.array_equal(g[1:], w[1:])


def test_the_solvers_guarantees_show_in_the_report(pkg, solver):
    for seed in range(6):
        rng = np.random.default_rng(900 + seed)
        s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(2, 7)), max_reads_per_contig=2500)
        n, M = s.size, int(rng.choice([3, 20]))
        ds, de, di = _dev(s), _dev(e), _dev(ids)
        d_mask = torch.zeros(max(pkg.mask_words(n), 1), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        rep = lambda **kw: solver.depth_report_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M,
                                                      d_keep_mask=d_mask.data_ptr(), n_bins=128, **kw)
        solver.solve_by_contig_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M, d_mask.data_ptr())
        plain = rep()
        assert plain.valid and np.all(plain.contig_rows["deficit_positions"] == 0)
        assert np.all(plain.contig_rows["max_kept"] <= plain.contig_rows["max_in"])
        assert plain.stats.reads_kept == solver.last_stats.n_kept
        # the quality pass keeps the same coverage: same sums, same histograms
        q = rng.integers(0, 61, size=n).astype(np.uint32)
        qmask = solver.solve_quality_by_contig(s, e, ids, q, lengths, M)
        quality = solver.depth_report(s, e, ids, lengths, M, keep_mask=qmask, n_bins=128)
        assert np.array_equal(quality.contig_rows["sum_kept"], plain.contig_rows["sum_kept"])
        assert np.array_equal(quality.hist_in, plain.hist_in) and np.array_equal(quality.hist_kept, plain.hist_kept)
        assert quality.valid
        # on-target solves, reported with the same regions and padding
        offs, t0, t1 = tm.random_regions(rng, lengths, max_regions=5, max_len=600)
        padding = int(rng.choice([0, 25]))
        drop_deficit = 0
        for keep_off in (False, True):
            solver.solve_targets_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M, offs, t0, t1,
                                        d_mask.data_ptr(), padding=padding, keep_off_target=keep_off)
            on = rep(**_regions_kw((offs, t0, t1), padding))
            assert on.valid and on.stats.deficit_positions == 0 and np.all(on.region_rows["deficit_positions"] == 0)
            if not keep_off:
                drop_deficit += int(on.contig_rows["deficit_positions"].sum())   # (off-target positions may be short)
            if n % 2 == 0:
                solver.complete_pairs_device(d_mask.data_ptr(), n)
                torch.cuda.synchronize()
                assert rep(**_regions_kw((offs, t0, t1), padding)).valid
    # (not asserted per seed: a call whose regions cover every deep position has no off-target deficit)


def test_errors_found_on_the_device_write_nothing(pkg, solver):
    rng = np.random.default_rng(13)
    s, e, ids, lengths = mr.random_by_contig(rng, 4, max_reads_per_contig=800)
    lengths = np.maximum(lengths, 1000).astype(np.uint32)
    c = int(np.argmax(np.bincount(ids[ids != NO_CONTIG].astype(np.int64), minlength=4)))
    offs = np.zeros(5, np.uint32)
    offs[c + 1:] = 1                                             # one region, [10, 60] of the contig with the most reads
    regions = (offs, np.array([10], np.uint32), np.array([60], np.uint32))
    unkept = int(np.flatnonzero((ids == c) & (s > 100))[0])      # an off-target read whose mask bit is clear
    mask = np.full(pkg.mask_words(s.size), ~np.uint64(0), np.uint64)
    mask[unkept >> 6] &= ~(np.uint64(1) << np.uint64(unkept & 63))
    cases = []
    bad_id = ids.copy(); bad_id[unkept] = lengths.size
    cases.append((s, e, bad_id, pkg.QMCP_EINVAL, "contig id"))
    bad_end = e.copy(); bad_end[unkept] = lengths[c]
    cases.append((s, bad_end, ids, pkg.QMCP_EREAD, "start > end or end >="))
    bad_start = s.copy(); bad_start[unkept] = e[unkept] + 1
    cases.append((bad_start, e, ids, pkg.QMCP_EREAD, "start > end or end >="))
    import ctypes as C
    for cs, ce, cid, code, needle in cases:
        contig_rows = np.full(lengths.size * 80, 0xA5, np.uint8)
        region_rows = np.full(4 * 80, 0xA5, np.uint8)
        hist_in, hist_kept, n_rows = (np.full(64 * 8, 0xA5, np.uint8) for _ in range(3))
        stats = np.full(C.sizeof(pkg.DepthStats), 0xA5, np.uint8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
        rc = pkg._hip.qmcp_hip_depth_report_host(
            solver._ctx, pkg._p32(cs), pkg._p32(ce), pkg._p32(cid), s.size, pkg._p32(lengths), lengths.size, pkg._p64(mask),
            5, pkg._p32(regions[0]), pkg._p32(regions[1]), pkg._p32(regions[2]), 0, 64, vp(contig_rows), vp(region_rows),
            4, p64(n_rows), p64(hist_in), p64(hist_kept), C.cast(vp(stats), C.POINTER(pkg.DepthStats)))
        assert rc == code and needle in pkg._hip.qmcp_hip_last_error().decode()
        assert all(np.all(a == 0xA5) for a in (contig_rows, region_rows, hist_in, hist_kept, n_rows, stats))
    # the context is fine afterwards
    dm.assert_equal(solver.depth_report(s, e, ids, lengths, 5, keep_mask=mask, n_bins=64, **_regions_kw(regions)),
                    dm.report(s, e, ids, lengths, 5, keep_mask=mask, n_bins=64, **_regions_kw(regions)))


def test_device_entry_on_a_callers_stream_equals_the_host_entry(pkg, solver):
    rng = np.random.default_rng(17)
    s, e, ids, lengths = mr.random_by_contig(rng, 5, max_reads_per_contig=2500)
    M, n = 10, s.size
    regions = tm.random_regions(rng, lengths, max_regions=5, max_len=500)
    kw = dict(n_bins=100, **_regions_kw(regions, 10))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):                              # the columns and the mask are produced on that stream
        ds, de, di = (torch.from_numpy(x.view(np.int32)).to("cuda:0", non_blocking=True) for x in (s, e, ids))
        d_mask = torch.zeros(max(pkg.mask_words(n), 1), dtype=torch.int64, device="cuda:0")
        solver.solve_by_contig_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M, d_mask.data_ptr(),
                                      stream=stream.cuda_stream)
        got = solver.depth_report_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M,
                                         d_keep_mask=d_mask.data_ptr(), stream=stream.cuda_stream, **kw)
    stream.synchronize()
    mask = d_mask.cpu().numpy().view(np.uint64)[:pkg.mask_words(n)]
    host = solver.depth_report(s, e, ids, lengths, M, keep_mask=mask, **kw)
    want = dm.report(s, e, ids, lengths, M, keep_mask=mask, **kw)
    dm.assert_equal(got, want)
    dm.assert_equal(host, want)
    assert got.contig_rows.tobytes() == host.contig_rows.tobytes() and got.region_rows.tobytes() == host.region_rows.tobytes()


def _grouping_ms(times):
    return sum(ms for name, (_, ms) in times.items() if name in GROUPING)


@pytest.mark.xfail(strict=True, raises=AssertionError, reason="k_depth_events holds the gate: 2 x 10^8 scattered 64-bit global atomics run at the "
                                       "memory-side atomic rate (23.6 G/s), 8.49 ms of ms_report's 9.29 ms against "
                                       "2.81 ms for the grouping stages (DESIGN 4.8)")
def test_a_report_costs_no_more_than_the_grouping_stages_of_the_plain_solve(pkg, solver):
    """cfg4's 10^8 reads shuffled over its 8 contigs, the mask from the plain by-contig solve, n_bins = 256, without regions
    and with the 776 regions of the targets test.  Asserted: stats.ms_report (median of 5 after a warm-up) does not exceed
    the grouping stages (k_bc_keys, the radix pass, k_bc_bounds, k_bc_gather; per-kernel events, median of 5) of the plain
    qmcp_hip_solve_by_contig_device call on the same reads, measured here in the same process.
    QMCP_DEPTH_TIME_OUT=<file> keeps the figures.
    Measured on one MI355X (profiles/depth_report_time.json): ms_report 9.29 ms without regions and 9.03 ms with them
    against 2.81 ms for the grouping stages -- the gate is MISSED.  k_depth_events takes 8.49 ms of it (2 x 10^8 scattered
    64-bit atomics at 23.6 G/s, the memory-side atomic rate), the chunk sums and spine 0.02 ms, k_depth_consume 0.74 /
    0.41 ms.  The assertion stays as the gate states it; the strict xfail mark flips when a form without scattered global
    atomics meets it."""
    n_contigs, pairs, L, M = 8, 6_250_000, 1_000_000, 100
    rng = np.random.default_rng(4)
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, 150, seed=12345 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
    perm = rng.permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    n = s.size
    lengths = np.full(n_contigs, L, np.uint32)
    starts_1 = np.arange(2_000, L - 5_000, 10_300, dtype=np.uint32)
    offs = (np.arange(n_contigs + 1) * starts_1.size).astype(np.uint32)
    t0 = np.tile(starts_1, n_contigs)
    t1 = t0 + 4_999
    assert t0.size == 776
    ds, de, di = _dev(s), _dev(e), _dev(ids)
    d_mask = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    def plain():
        return solver.solve_by_contig_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M, d_mask.data_ptr())

    def report(regions):
        kw = _regions_kw((offs, t0, t1)) if regions else {}
        return solver.depth_report_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M,
                                          d_keep_mask=d_mask.data_ptr(), n_bins=256, **kw)

    plain(); plain()
    first = report(False)
    assert first.valid and first.stats.reads_placed == n and report(True).valid
    ms = {False: [], True: []}
    stages = {False: [], True: []}
    for regions in (False, True):
        for _ in range(5):
            ms[regions].append(float(report(regions).stats.ms_report))
        for _ in range(5):
            solver.set_profiling(True)
            report(regions)
            kt = solver.kernel_times()
            stages[regions].append({k: kt[k][1] for k in DEPTH_STAGES if k in kt})
    grouping, stage_runs = [], []
    for _ in range(5):
        solver.set_profiling(True)
        plain()
        kt = solver.kernel_times()
        grouping.append(_grouping_ms(kt))
        stage_runs.append({k: kt[k][1] for k in GROUPING if k in kt})
    solver.set_profiling(False)
    med = statistics.median
    positions = n_contigs * L
    need_bytes = 12 * n + n // 8 + 8 * positions + 2 * 8 * positions   # columns + mask, the memset, two reads of the events
    figures = {
        "reads": n, "contigs": n_contigs, "positions": positions, "M": M, "n_bins": 256, "regions": int(t0.size),
        "ms_report_median": round(med(ms[False]), 4), "ms_report_runs": [round(x, 4) for x in ms[False]],
        "ms_report_regions_median": round(med(ms[True]), 4), "ms_report_regions_runs": [round(x, 4) for x in ms[True]],
        "stages_ms_median": {k: round(med([r.get(k, 0.0) for r in stages[False]]), 4) for k in DEPTH_STAGES},
        "stages_regions_ms_median": {k: round(med([r.get(k, 0.0) for r in stages[True]]), 4) for k in DEPTH_STAGES},
        "grouping_ms_median": round(med(grouping), 4), "grouping_runs": [round(x, 4) for x in grouping],
        "grouping_stages_ms_median": {k: round(med([r.get(k, 0.0) for r in stage_runs]), 4) for k in GROUPING},
        "min_bytes": need_bytes, "ms_at_copy_rate_6.29TBps": round(need_bytes / 6.29e12 * 1e3, 4),
        "atomics": 2 * n,
    }
    print("depth_report_time " + json.dumps(figures))
    out = os.environ.get("QMCP_DEPTH_TIME_OUT")
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(figures, indent=1) + "\n")
    assert med(ms[False]) <= med(grouping) and med(ms[True]) <= med(grouping), figures


def _parse_tsv(path):
    lines = open(path).read().split("\n")
    assert lines[0].startswith("#kind\treference\tstart\tend\tpositions\tmean_in\tmean_kept") and lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1] if not ln.startswith("#")]
    hist = [[int(x) for x in ln.split("\t")[1:]] for ln in lines[1:-1] if ln.startswith("#hist")]
    return rows, hist


def _model_tsv_rows(want, names):
    out = []
    for kind, rows in (("contig", want["contig_rows"]), ("region", want["region_rows"])):
        for r in rows:
            pos = r[8]
            out.append([kind, names[r[0]], str(r[1]), str(r[2] + 1 if pos else r[1]), str(pos),
                        f"{(r[9] / pos if pos else 0.0):.6f}", f"{(r[10] / pos if pos else 0.0):.6f}"] +
                       [str(x) for x in (r[3], r[4], r[5], r[6], r[11], r[12], r[13])])
    return out


@pytest.mark.parametrize("with_targets", [False, True])
def test_file_flow_writes_the_report_of_the_written_file(pkg, tmp_path, with_targets):
    import bam_py
    rng = np.random.default_rng(41)
    refs = [("chr1", 6000), ("chr2", 3500), ("chrEmpty", 900), ("chrM", 1200)]
    names = [n for n, _ in refs]
    path = tmp_path / "in.bam"
    header, parsed, ref_lengths = mr.write_multi_reference_bam(path, rng, refs, 4000)
    M, padding = 8, 20
    bed = None
    regions = None
    if with_targets:
        bed = tmp_path / "targets.bed"
        bed.write_text("chr1\t100\t900\nchr1\t700\t1500\nchr1\t4000\t4400\nchr2\t0\t300\nchrM\t500\t5000\n")
        regions = pkg.targets_from_bed(bed, names)
    out, report = tmp_path / "out.bam", tmp_path / "depth.tsv"
    kw = dict(per_reference=True, targets=bed, target_padding=padding if with_targets else 0)
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, report=report, report_bins=16, **kw)
    # the report of read_bam's columns against the ids of the written file
    cols = pkg.read_bam(path, per_reference=True)
    _, orecs, _ = bam_py.parse(out)
    assert written == len(orecs) > 0
    raw_to_id = {r["raw"]: i for i, r in enumerate(parsed)}
    kept_bam_ids = np.array(sorted(raw_to_id[r["raw"]] for r in orecs), np.uint64)
    kept = np.isin(cols["bam_ids"], kept_bam_ids)
    assert int(kept.sum()) == written
    mask = qm.mask_of(kept)
    want = dm.report(cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"], M, keep_mask=mask, n_bins=16,
                     **_regions_kw(regions, padding))
    rows, hist = _parse_tsv(report)
    assert rows == _model_tsv_rows(want, names)
    assert [h[1] for h in hist] == want["hist_in"].tolist() and [h[2] for h in hist] == want["hist_kept"].tolist()
    scope = want["region_rows"] if with_targets else want["contig_rows"]
    assert all(r[12] == 0 for r in scope) and len(scope) > 0
    # without report= the output is byte for byte what it is with it, and the same as a second call's
    out2, out3 = tmp_path / "out2.bam", tmp_path / "out3.bam"
    pkg.downsample_bam("quasi-mcp-hip", path, out2, M, **kw)
    pkg.downsample_bam("quasi-mcp-hip", path, out3, M, **kw)
    assert out.read_bytes() == out2.read_bytes() == out3.read_bytes()
    with pytest.raises(ValueError, match="per_reference"):
        pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", M, report=tmp_path / "no.tsv")
    assert not (tmp_path / "no.tsv").exists()
