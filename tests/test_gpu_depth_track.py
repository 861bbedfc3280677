"""qmcp_hip_depth_track_*: the full record array and the statistics bit for bit against tests/track_model.py (numpy, from
events): random calls over every flag word, boundaries placed on thread, wave, tile, chunk and batch edges, the report's
sums seen through the track, capacity and device-found errors, the file flow, and the time against the depth report."""
import ctypes as C
import statistics

import numpy as np
import pytest
import torch

import depth_model as dm
import multi_reference as mr
import quality_model as qm
import target_model as tm
import track_model as tk

pytestmark = pytest.mark.gpu

NO_CONTIG = 0xFFFFFFFF
FLAG_WORDS = [ch | mod for mod in (0, 4, 8, 12) for ch in (1, 2, 3)]

# ms_track / ms_report on the same reads and mask, cfg4's 10^8 reads over 8 contigs (lab/depth_track_time.py on one MI355X,
# profiles/depth_track_time.json): see test_a_track_costs_what_a_report_costs
MEASURED_RATIO = 5.0614
MEASURED_ON = "2026-10-18"


def _flag_kw(flags):
    return dict(channels=tuple(n for n, b in (("in", 1), ("kept", 2)) if flags & b), short_only=bool(flags & 4),
                skip_zero=bool(flags & 8))


def _regions_kw(regions, padding=0):
    if regions is None:
        return {}
    return dict(target_offsets=regions[0], target_starts=regions[1], target_ends=regions[2], padding=padding)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")


def _track_device(solver, s, e, ids, lengths, M, mask=None, offset=0, **kw):
    """through the _device entry; offset > 0 shifts the columns off 16-byte alignment"""
    pad = np.zeros(offset, np.uint32)
    ds, de, di = (_dev(np.concatenate([pad, x])) for x in (s, e, ids))
    dm_ = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint64).view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr() + 4 * offset
    return solver.depth_track_device(ptr(ds), ptr(de), ptr(di), s.size, lengths, M,
                                     d_keep_mask=0 if dm_ is None else dm_.data_ptr(), **kw)


def _check(solver, s, e, ids, lengths, M, mask, flags, cap=0, regions=None, padding=0, info="", device=False):
    s, e, ids = (np.ascontiguousarray(x, np.uint32) for x in (s, e, ids))
    rk = _regions_kw(regions, padding)
    want = tk.track(s, e, ids, lengths, M, keep_mask=mask, flags=flags, depth_cap=cap, **rk)
    kw = dict(depth_cap=cap, **_flag_kw(flags), **rk)
    tk.assert_equal(*solver.depth_track(s, e, ids, lengths, M, keep_mask=mask, **kw), want, (info, "host"))
    if device:
        for offset in (0, 1):
            tk.assert_equal(*_track_device(solver, s, e, ids, lengths, M, mask=mask, offset=offset, **kw), want, (info, offset))
    st = solver.last_track_stats
    assert st.n_runs <= min(st.positions_in_runs, 2 * st.reads_placed + len(lengths) + st.regions_merged), info
    return want


def _random_mask(rng, pkg, n):
    return rng.integers(0, 1 << 63, size=max(pkg.mask_words(n), 1), dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, size=max(pkg.mask_words(n), 1), dtype=np.uint64)


def test_random_calls_equal_the_model(pkg, solver):
    seen = dict(zero_length=0, unplaced=0, short=0, regions=0, runs=0)
    for seed in range(48):
        rng = np.random.default_rng(8000 + seed)
        n_contigs = int(rng.integers(1, 41))
        s, e, ids, lengths = mr.random_by_contig(rng, n_contigs, max_reads_per_contig=int(rng.choice([40, 400, 2500])),
                                                 unplaced=0.05)
        lengths = lengths.copy()
        for c in range(n_contigs):
            if not np.any(ids == c) and rng.random() < 0.5:
                lengths[c] = 0
        M = int(rng.choice([1, 3, 20, 50]))
        kind = seed % 3
        if kind == 0:
            mask = solver.solve_by_contig(s, e, ids, np.maximum(lengths, 1).astype(np.uint32), M)
        elif kind == 1:
            mask = _random_mask(rng, pkg, s.size)
        else:
            mask = None
        regions, padding = None, 0
        if seed % 2:
            regions = tm.random_regions(rng, lengths, max_regions=6, max_len=700)
            padding = int(rng.choice([0, 0, 30]))
        flags, cap = FLAG_WORDS[seed % 12], (0, 1, 7)[(seed // 12 + seed) % 3]
        runs, stats = _check(solver, s, e, ids, lengths, M, mask, flags, cap, regions, padding, f"seed {seed}", device=True)
        assert solver.last_track_stats.position_batches == 1
        seen["zero_length"] += int(np.any(lengths == 0))
        seen["unplaced"] += int(np.any(ids == NO_CONTIG))
        seen["short"] += int(stats["short_positions"] > 0)
        seen["regions"] += int(stats["regions_merged"] > 0)
        seen["runs"] += len(runs)
    assert seen["zero_length"] > 8 and seen["unplaced"] > 20 and seen["short"] > 8 and seen["regions"] > 15, seen
    assert seen["runs"] > 50_000, seen


EDGES = (3, 4, 255, 256, 1023, 1024)


def _edge_cases():
    """name -> (starts, ends, ids, lengths, regions): run, contig and region boundaries on thread (3 / 4), wave (255 / 256)
    and tile (1023 / 1024) edges of the batch's axis and on its last position"""
    cases = {}
    # runs: one contig, reads that begin and end on both sides of every edge, one ending on P - 1
    L = 2100
    s = [x for x in EDGES] + [x - 2 for x in EDGES if x >= 2] + [0, 2000]
    e = [x + 1 for x in EDGES] + [x for x in EDGES if x >= 2] + [3, L - 1]
    cases["runs"] = (s, e, [0] * len(s), [L], None)
    # contigs: borders at 3, 4, 255, 256, 1023, 1024, 1025 (a contig of length 1 among them); in every contig a read that
    # ends on its last position, so its -w lands on the next contig's first word, and one that begins on its first
    lengths = [3, 1, 251, 1, 767, 1, 1, 300]
    assert np.cumsum(lengths).tolist()[:7] == [3, 4, 255, 256, 1023, 1024, 1025]
    s, e, ids = [], [], []
    for c, n in enumerate(lengths):
        s += [n - 1, 0, n // 2]
        e += [n - 1, 0, n - 1]
        ids += [c, c, c]
    cases["contigs"] = (s, e, ids, lengths, None)
    cases["contigs_tile_multiple"] = (s + [722], e + [722], ids + [8], lengths + [723], None)   # P = 1 325 + 723 = 2 x 1 024
    # regions: bounds on every edge, adjacent ones that merge, one ending on P - 1; depth changes inside and outside
    L = 2048
    r0 = [0, 4, 250, 256, 1000, 1024, 2040]
    r1 = [2, 100, 255, 300, 1023, 1030, 2047]
    rs = list(range(0, L - 60, 37)) + [L - 60]
    cases["regions"] = (rs, [x + 59 for x in rs], [0] * len(rs), [L], (np.array([0, len(r0)], np.uint32), np.array(r0, np.uint32), np.array(r1, np.uint32)))
    return cases


@pytest.mark.parametrize("case", ["runs", "contigs", "contigs_tile_multiple", "regions"])
def test_boundaries_on_thread_wave_and_tile_edges(pkg, solver, case):
    s, e, ids, lengths, regions = _edge_cases()[case]
    lengths = np.array(lengths, np.uint32)
    if case == "contigs_tile_multiple":
        assert int(lengths.sum()) % 1024 == 0                         # the run open at P - 1 is closed after the last tile
    rng = np.random.default_rng(3)
    mask = _random_mask(rng, pkg, len(s))
    for flags in FLAG_WORDS:
        for m in (None, mask):
            for cap in (0, 1):
                runs, _ = _check(solver, s, e, ids, lengths, 2, m, flags, cap, regions, 0, (case, flags, cap), device=flags == 3)
    runs, _ = _check(solver, s, e, ids, lengths, 2, None, 3, 0, regions, 0, case)
    assert runs[-1][2] == int(lengths[-1]) - 1 and runs[-1][3] > 0    # the last run ends on P - 1, inside a read


def test_staircase_no_reads_clamp_and_short_only(pkg, solver):
    L = 2500
    stairs = np.arange(L, dtype=np.uint32)
    ends = np.full(L, L - 1, np.uint32)
    ids = np.zeros(L, np.uint32)
    runs, stats = _check(solver, stairs, ends, ids, [L], 10, None, 3, 0, info="staircase", device=True)
    assert len(runs) == L == stats["positions_in_runs"] and [r[3] for r in runs] == list(range(1, L + 1))
    runs, _ = _check(solver, stairs, ends, ids, [L], 10, None, 3, 7, info="clamp")          # the deep stretch is one run
    assert len(runs) == 7 and runs[-1] == (0, 6, L - 1, 7, 7, 0)
    none = np.zeros(0, np.uint32)
    lengths = [700, 0, 1, 1024, 5]
    runs, _ = _check(solver, none, none, none, lengths, 5, None, 3, info="no reads")
    assert runs == [(0, 0, 699, 0, 0, 0), (2, 0, 0, 0, 0, 0), (3, 0, 1023, 0, 0, 0), (4, 0, 4, 0, 0, 0)]
    runs, stats = _check(solver, none, none, none, lengths, 5, None, 3 | 8, info="no reads, skip zero")
    assert runs == [] and stats["positions_in_runs"] == 0 and stats["scope_positions"] == 1730
    rng = np.random.default_rng(77)
    s, e, ids, lengths = mr.random_by_contig(rng, 6, max_reads_per_contig=2500)
    M = 10
    valid = solver.solve_by_contig(s, e, ids, lengths, M)
    runs, stats = _check(solver, s, e, ids, lengths, M, valid, 3 | 4, info="short only, valid mask")
    assert runs == [] and stats["short_positions"] == 0
    runs, stats = _check(solver, s, e, ids, lengths, M, _random_mask(rng, pkg, s.size), 2 | 4, info="short only, random mask",
                         device=True)
    assert len(runs) > 100 and all(r[5] == 1 for r in runs) and stats["short_positions"] == stats["positions_in_runs"]


def test_chunks_of_several_tiles(pkg, solver):
    """one contig of 3 x 2 048 x 1 024 + 5 positions: 6 145 tiles in chunks of 4 tiles.  Reads begin and end on chunk edges
    (multiples of 4 096), a long read spans many chunks, and so do the stretches of depth 0"""
    L = 3 * 2048 * 1024 + 5
    chunk = 4096
    rng = np.random.default_rng(19)
    n = 10_000
    s = rng.integers(0, L - 400, size=n)
    e = s + rng.integers(0, 300, size=n)
    k = rng.integers(1, L // chunk, size=300) * chunk
    s = np.concatenate([s, k, k - 150, k - 1, [chunk * 10, L - 1, 5 * chunk + 7]])
    e = np.concatenate([e, k + 99, k - 1, k, [chunk * 500 - 1, L - 1, 5 * chunk + 7]])
    ids = np.zeros(s.size, np.uint32)
    mask = _random_mask(rng, pkg, s.size)
    regions = (np.array([0, 4], np.uint32), np.array([chunk * 3, chunk * 9 + 1, chunk * 100, L - 10], np.uint32),
               np.array([chunk * 8 - 1, chunk * 12, chunk * 300 - 1, L - 1], np.uint32))
    for flags, cap, reg in ((3, 0, None), (2 | 8, 0, None), (3 | 4, 1, None), (3, 0, regions), (1 | 8, 2, regions)):
        runs, _ = _check(solver, s, e, ids, [L], 2, mask, flags, cap, reg, 0, ("chunks", flags), device=flags == 3)
        assert len(runs) > 1000
    # depth_in clamped to 1, every read kept: the long read is one run over hundreds of chunks
    runs, _ = _check(solver, s, e, ids, [L], 2, None, 1, 1, None, 0, "one run over many chunks")
    assert max(r[2] - r[1] for r in runs if r[3] == 1) >= 490 * chunk - 1


def test_two_position_batches(pkg, solver):
    rng = np.random.default_rng(5)
    big, D = 1_200_000_000, 1_100_000_000
    s, e, ids, _ = mr.random_by_contig(rng, 2, max_reads_per_contig=450, unplaced=0.05)
    assert s.size <= 998
    placed = ids != NO_CONTIG
    span = np.minimum(e.astype(np.int64) - s, 250)
    s = np.where(placed, rng.integers(0, 4_700, size=s.size) + D * rng.integers(0, 2, size=s.size), 0)
    e = np.where(placed, s + span, 0)
    # the batch edge: a read on the first contig's last position, one on the second contig's first
    s, e = np.concatenate([s, [big - 3, 0]]), np.concatenate([e, [big - 1, 2]])
    ids = np.concatenate([ids, np.array([0, 1], np.uint32)])
    mask = _random_mask(rng, pkg, s.size)
    for flags in (3, 3 | 8, 2 | 4):
        runs, stats = _check(solver, s, e, ids, [big, big], 4, mask, flags, info=("batches", flags))
        assert solver.last_track_stats.position_batches == 2
        assert [r[0] for r in runs] == sorted(r[0] for r in runs) and (flags & 4 or {r[0] for r in runs} == {0, 1})
    runs, stats = _check(solver, s, e, ids, [big, big], 4, None, 3, info="batches, no mask")
    assert stats["scope_positions"] == stats["positions_in_runs"] == 2 * big
    last0 = max(i for i, r in enumerate(runs) if r[0] == 0)
    assert runs[last0][2] == big - 1 and runs[last0][3] >= 1 and runs[last0 + 1][:2] == (1, 0) and runs[last0 + 1][3] >= 1


def test_the_track_sums_to_the_report(pkg, solver):
    for seed in range(4):
        rng = np.random.default_rng(300 + seed)
        s, e, ids, lengths = mr.random_by_contig(rng, 7, max_reads_per_contig=2500)
        M = int(rng.choice([3, 20]))
        mask = _random_mask(rng, pkg, s.size)
        regions = tm.random_regions(rng, lengths, max_regions=5, max_len=600) if seed % 2 else None
        runs, stats = solver.depth_track(s, e, ids, lengths, M, keep_mask=mask)
        report = solver.depth_report(s, e, ids, lengths, M, keep_mask=mask)
        length = runs["end"].astype(np.int64) - runs["start"] + 1
        for field, column in (("depth_in", "sum_in"), ("depth_kept", "sum_kept")):
            sums = np.zeros(lengths.size, np.int64)
            np.add.at(sums, runs["contig"], length * runs[field].astype(np.int64))
            assert np.array_equal(sums, report.contig_rows[column].astype(np.int64)), (seed, field)
        assert stats.short_positions == report.stats.deficit_positions > 0
        assert int(length[runs["flags"] == 1].sum()) == stats.short_positions
        if regions is not None:
            runs, stats = solver.depth_track(s, e, ids, lengths, M, keep_mask=mask, **_regions_kw(regions, 10))
            report = solver.depth_report(s, e, ids, lengths, M, keep_mask=mask, **_regions_kw(regions, 10))
            assert stats.short_positions == report.stats.deficit_positions
            assert stats.scope_positions == report.stats.scope_positions == stats.positions_in_runs
            length = runs["end"].astype(np.int64) - runs["start"] + 1
            assert int((length * runs["depth_kept"]).sum()) == int(report.region_rows["sum_kept"].sum())


def _raw_call(pkg, solver, s, e, ids, lengths, mask, capacity, with_runs=True, M=5, flags=3):
    s, e, ids, lengths = (np.ascontiguousarray(x, np.uint32) for x in (s, e, ids, lengths))
    runs = np.full(max(capacity, 1) * 24, 0xA5, np.uint8)
    n_runs = np.full(8, 0xA5, np.uint8)
    stats = np.full(C.sizeof(pkg.TrackStats), 0xA5, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = pkg._hip.qmcp_hip_depth_track_host(
        solver._ctx, pkg._p32(s), pkg._p32(e), pkg._p32(ids), s.size, pkg._p32(lengths), lengths.size, pkg._p64(mask), M,
        None, None, None, 0, flags, 0, vp(runs) if with_runs else None, capacity,
        n_runs.ctypes.data_as(C.POINTER(C.c_uint64)), C.cast(vp(stats), C.POINTER(pkg.TrackStats)))
    return rc, runs, n_runs, stats


def test_capacity_and_counting(pkg, solver):
    rng = np.random.default_rng(23)
    s, e, ids, lengths = mr.random_by_contig(rng, 4, max_reads_per_contig=800)
    mask = _random_mask(rng, pkg, s.size)
    want, _ = tk.track(s, e, ids, lengths, 5, keep_mask=mask)
    total = len(want)
    rc, runs, n_runs, stats = _raw_call(pkg, solver, s, e, ids, lengths, mask, 0, with_runs=False)     # runs == NULL: the count
    assert rc == pkg.QMCP_OK and int(n_runs.view(np.uint64)[0]) == total and np.all(runs == 0xA5)
    assert int(stats.view(np.uint64)[0]) == total
    rc, runs, n_runs, stats = _raw_call(pkg, solver, s, e, ids, lengths, mask, total - 1)
    assert rc == pkg.QMCP_ERANGE and f"{total} runs" in pkg._hip.qmcp_hip_last_error().decode()
    assert int(n_runs.view(np.uint64)[0]) == total and np.all(runs == 0xA5) and np.all(stats == 0xA5)
    rc, runs, n_runs, stats = _raw_call(pkg, solver, s, e, ids, lengths, mask, total)
    assert rc == pkg.QMCP_OK and int(n_runs.view(np.uint64)[0]) == total
    assert [tuple(int(x) for x in r) for r in runs.view(pkg.TRACK_RUN_DTYPE).tolist()] == want
    # the wrapper's second call at the exact count
    small, pkg.TRACK_FIRST_CAPACITY = pkg.TRACK_FIRST_CAPACITY, 10
    try:
        tk.assert_equal(*solver.depth_track(s, e, ids, lengths, 5, keep_mask=mask), tk.track(s, e, ids, lengths, 5, keep_mask=mask))
    finally:
        pkg.TRACK_FIRST_CAPACITY = small


def test_errors_found_on_the_device_write_nothing(pkg, solver):
    rng = np.random.default_rng(13)
    s, e, ids, lengths = mr.random_by_contig(rng, 4, max_reads_per_contig=800)
    lengths = np.maximum(lengths, 1000).astype(np.uint32)
    c = int(np.argmax(np.bincount(ids[ids != NO_CONTIG].astype(np.int64), minlength=4)))
    victim = int(np.flatnonzero(ids == c)[0])
    mask = np.full(pkg.mask_words(s.size), ~np.uint64(0), np.uint64)
    bad_id = ids.copy(); bad_id[victim] = lengths.size
    bad_end = e.copy(); bad_end[victim] = lengths[c]
    bad_start = s.copy(); bad_start[victim] = e[victim] + 1
    for cs, ce, cid, code, needle in ((s, e, bad_id, pkg.QMCP_EINVAL, "contig id"),
                                      (s, bad_end, ids, pkg.QMCP_EREAD, "start > end or end >="),
                                      (bad_start, e, ids, pkg.QMCP_EREAD, "start > end or end >=")):
        for capacity in (1, 1 << 16):                                # the device's error comes before the capacity
            rc, runs, n_runs, stats = _raw_call(pkg, solver, cs, ce, cid, lengths, mask, capacity)
            assert rc == code and needle in pkg._hip.qmcp_hip_last_error().decode()
            assert np.all(runs == 0xA5) and np.all(n_runs == 0xA5) and np.all(stats == 0xA5)
    _check(solver, s, e, ids, lengths, 5, mask, 3, info="the context is fine afterwards")


@pytest.mark.parametrize("mode", ["plain", "targets", "targets_and_report"])
def test_file_flow_writes_the_track_of_the_written_file(pkg, tmp_path, mode):
    import bam_py
    rng = np.random.default_rng(41)
    refs = [("chr1", 6000), ("chr2", 3500), ("chrEmpty", 900), ("chrM", 1200)]
    names = [n for n, _ in refs]
    path = tmp_path / "in.bam"
    header, parsed, ref_lengths = mr.write_multi_reference_bam(path, rng, refs, 4000)
    M, padding = 8, 20
    bed, regions = None, None
    if mode != "plain":
        bed = tmp_path / "targets.bed"
        bed.write_text("chr1\t100\t900\nchr1\t700\t1500\nchr1\t4000\t4400\nchr2\t0\t300\nchrM\t500\t5000\n")
        regions = pkg.targets_from_bed(bed, names)
    out, track, report = tmp_path / "out.bam", tmp_path / "depth.bedgraph", tmp_path / "depth.tsv"
    kw = dict(per_reference=True, targets=bed, target_padding=padding if bed else 0)
    extra = dict(report=report, report_bins=8) if mode == "targets_and_report" else {}
    cap = 0 if mode == "plain" else 6
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, track=track, track_channel="both", track_cap=cap, **extra, **kw)
    cols = pkg.read_bam(path, per_reference=True)
    _, orecs, _ = bam_py.parse(out)
    assert written == len(orecs) > 0
    raw_to_id = {r["raw"]: i for i, r in enumerate(parsed)}
    kept = np.isin(cols["bam_ids"], np.array(sorted(raw_to_id[r["raw"]] for r in orecs), np.uint64))
    want, _ = tk.track(cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"], M, keep_mask=qm.mask_of(kept),
                       depth_cap=cap, **_regions_kw(regions, padding if bed else 0))
    model = tmp_path / "model.bedgraph"
    pkg.write_bedgraph(model, np.array(want, dtype=pkg.TRACK_RUN_DTYPE), names, channel="both")
    assert track.read_text() == model.read_text()
    assert len(want) > (50 if mode == "plain" else 5)                 # (the clamp at 6 leaves few runs inside the targets)
    assert report.exists() == (mode == "targets_and_report")
    out2 = tmp_path / "out2.bam"                                      # track=None changes nothing
    pkg.downsample_bam("quasi-mcp-hip", path, out2, M, **kw)
    assert out.read_bytes() == out2.read_bytes()


def test_a_track_costs_what_a_report_costs(pkg, solver):
    """cfg4's reads at 1 / 10 of the size (10^7 reads shuffled over 8 contigs of 10^5 positions, the same depth), the
    mask from the plain by-contig solve, both channels.  Asserted: ms_track (median of 5 after a warm-up)
    is at most ms_report (the same) x MEASURED_RATIO x 1.25 -- the ratio lab/depth_track_time.py measured at full size,
    plus 25 % for run-to-run spread.
    Measured at full size on MEASURED_ON (profiles/depth_track_time.json): ms_track 47.07 ms against ms_report 9.30 ms, ratio
    5.0614.  The new kernels take 0.17 ms of it (k_track_count + k_track_spine 0.05 ms, k_track_emit 0.12 ms, against
    0.73 ms for k_depth_consume); a count-only call (runs == NULL) takes 8.66 ms, 0.93 of the report.  The rest is the
    7.36 x 10^6 records (177 MB) copied to pageable host staging inside the timed span."""
    assert MEASURED_RATIO is not None, "lab/depth_track_time.py has not been run: no ratio to hold the track to"
    n_contigs, pairs, L, M = 8, 625_000, 100_000, 100
    rng = np.random.default_rng(4)
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, 150, seed=12345 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
    perm = rng.permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    n = s.size
    lengths = np.full(n_contigs, L, np.uint32)
    ds, de, di = _dev(s), _dev(e), _dev(ids)
    d_mask = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    solver.solve_by_contig_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M, d_mask.data_ptr())
    args = (ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M)
    track = lambda: solver.depth_track_device(*args, d_keep_mask=d_mask.data_ptr())[1].ms_track
    report = lambda: solver.depth_report_device(*args, d_keep_mask=d_mask.data_ptr()).stats.ms_report
    track(); report()
    ms_track = statistics.median(float(track()) for _ in range(5))
    ms_report = statistics.median(float(report()) for _ in range(5))
    print(f"depth_track_time ms_track {ms_track:.4f} ms_report {ms_report:.4f} ratio {ms_track / ms_report:.3f} "
          f"gate {MEASURED_RATIO * 1.25:.3f}")
    assert solver.last_track_stats.short_positions == 0
    assert ms_track <= ms_report * MEASURED_RATIO * 1.25, (ms_track, ms_report, MEASURED_RATIO)
