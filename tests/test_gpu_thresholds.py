"""qmcp_hip_solve_thresholds_*: every read's smallest keeping coverage in one call.  Every expected value comes from the
CPU oracle and numpy (tests/thresholds_model.py): thresholds, counts, top, solves and nesting_violations are EQUAL to the
model's -- its violations are 0 on these inputs by tests/test_thresholds_cpu.py; nothing here asserts a literal 0."""
import time

import numpy as np
import pytest

import bam_py
import budget_model as bm
import multi_reference as mr
import thresholds_model as tm
from forcing import forced

pytestmark = pytest.mark.gpu

NO_CONTIG = mr.NO_CONTIG
NEVER = tm.NEVER


def check(want, thr, ts, counts=None, capacity=None):
    """one call's thresholds, statistics and counts against the model"""
    where = ts.as_dict()
    assert thr.dtype == np.uint16 and np.array_equal(thr, want.thresholds), where
    assert (ts.coverage_lo, ts.coverage_hi, ts.top, ts.solves) == (want.lo, want.hi, want.top, want.solves), where
    assert ts.nesting_violations == want.violations and ts.saturated == want.saturated, where
    assert ts.reads_placed == want.model.placed and ts.n_kept == want.n_kept, where
    if counts is not None:
        expected = want.counts(capacity)
        assert ts.count_entries == expected.size == counts.size and np.array_equal(counts, expected), where


# ------------------------------------------------------------------------------------------ 1: mixed spans
@pytest.fixture(scope="module")
def mixed():
    return [mr.random_by_contig(np.random.default_rng(seed), 3, 1200) for seed in range(4)]


@pytest.mark.parametrize("seed", range(4))
def test_mixed_spans_equal_the_model_and_every_mask_equals_the_device_solve(pkg, oracle, solver, mixed, seed):
    s, e, ids, lengths = mixed[seed]
    n = s.size
    hi = int(bm.depth(s, e, ids, lengths).max(initial=0)) + 7                     # beyond the largest depth: the early stop
    want = tm.Thresholds(oracle, s, e, ids, lengths, 1, hi)
    thr, ts, counts = solver.solve_thresholds(s, e, ids, lengths, hi, counts=True)
    check(want, thr, ts, counts)
    assert want.saturated == 1 and want.top < hi and ts.solves < hi               # stopped early, everything placed seen
    assert np.all(thr[ids == NO_CONTIG] == NEVER)
    assert solver.last_stats.n_kept == want.model.count(want.top)                 # the last solve
    for M in range(1, hi + 1):                                                    # on the device, every M of the range
        assert np.array_equal(pkg.threshold_mask(thr, M), solver.solve_by_contig(s, e, ids, lengths, M)), M
    # a range that starts above 1 and ends below the largest depth: a collapsed lo, NEVER above hi
    full_top = want.top
    want = tm.Thresholds(oracle, s, e, ids, lengths, 5, 12)
    thr, ts, counts = solver.solve_thresholds(s, e, ids, lengths, 12, coverage_lo=5, counts=True)
    check(want, thr, ts, counts)
    if full_top > 12:                                                             # (some read needs more than 12)
        assert want.saturated == 0 and want.top == 12 and (thr[ids != NO_CONTIG] == NEVER).any()
    assert np.array_equal(thr == 5, bm.unpack(solver.solve_by_contig(s, e, ids, lengths, 5), n))
    for M in range(5, 13):
        assert np.array_equal(pkg.threshold_mask(thr, M), solver.solve_by_contig(s, e, ids, lengths, M)), M
    # a counts array shorter than the range takes what fits
    _, _, short = solver.solve_thresholds(s, e, ids, lengths, 12, coverage_lo=5, counts=True)
    cap = 3
    table = np.zeros(cap, np.uint64)
    thr3 = np.zeros(max(n, 1), np.uint16)
    st, ts3 = pkg.Stats(), pkg.ThresholdsStats()
    lens = np.asarray(lengths, np.uint32)
    rc = pkg._hip.qmcp_hip_solve_thresholds_host(solver._ctx, pkg._p32(s), pkg._p32(e), pkg._p32(ids), n, pkg._p32(lens),
                                                 lens.size, 5, 12, 0, thr3.ctypes.data_as(pkg._u16p), pkg._p64(table), cap,
                                                 st, ts3)
    assert rc == 0
    check(want, thr3[:n], ts3, table[:ts3.count_entries], capacity=cap)
    assert ts3.count_entries == 3 and np.array_equal(table, short[:3])


# ------------------------------------------------------------------------------------------ 2: whole pairs
@pytest.mark.parametrize("seed", range(4))
def test_whole_pairs_take_the_placed_mates_minimum(pkg, oracle, solver, mixed, seed):
    s, e, ids, lengths = mixed[seed]
    n = s.size & ~1
    s, e, ids = s[:n], e[:n], ids[:n]
    placed = ids != NO_CONTIG
    assert n == 0 or (placed[0::2] != placed[1::2]).any()                         # unplaced mates among them
    hi = int(bm.depth(s, e, ids, lengths).max(initial=0)) + 1
    want = tm.Thresholds(oracle, s, e, ids, lengths, 1, hi, whole_pairs=True)
    thr, ts, counts = solver.solve_thresholds(s, e, ids, lengths, hi, flags=pkg.THRESHOLDS_WHOLE_PAIRS, counts=True)
    check(want, thr, ts, counts)
    assert np.all(thr[~placed] == NEVER)
    for M in range(1, hi + 1):                                                    # the budget entry's completion of keep_M
        assert np.array_equal(thr <= M, bm.complete_pairs(want.model.bits(M), ids)), M
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_thresholds(s[:n - 1], e[:n - 1], ids[:n - 1], lengths, hi, flags=pkg.THRESHOLDS_WHOLE_PAIRS)
    assert ex.value.code == pkg.QMCP_EINVAL and "odd" in str(ex.value)


# ------------------------------------------------------------------------------------------ 3: one span, every route
@pytest.fixture(scope="module")
def one_length(oracle):
    rng = np.random.default_rng(404)
    L, n, span = 10_000, 4_000, 100                                               # depth about 40
    s = rng.integers(0, L - span + 1, n).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    ids = np.zeros(n, np.uint32)
    want = tm.Thresholds(oracle, s, e, ids, [L], 1, 40)
    assert 30 < want.model.max_depth
    return s, e, ids, [L], want


ROUTES = [{}, {"QMCP_HIP_SWEEP": "fast"}, {"QMCP_HIP_SWEEP": "gen"}, {"QMCP_HIP_SWEEP": "ev"}, {"QMCP_HIP_CUTS": "1"},
          {"QMCP_HIP_CUTS": "0"}, {"QMCP_HIP_NO_RANK": "1"}, {"QMCP_HIP_NEAR": "0"}]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "-".join(f"{k[9:]}={v}" for k, v in r.items()) or "auto")
def test_one_read_length_under_every_forced_route(solver, one_length, route):
    s, e, ids, lengths, want = one_length
    with forced(solver, **route):
        thr, ts, counts = solver.solve_thresholds(s, e, ids, lengths, 40, counts=True)
    check(want, thr, ts, counts)


# ------------------------------------------------------------------------------------------ 4: several batches, edges
def test_several_batches(pkg, oracle, solver):
    """two empty contigs as long as one solver call allows between the others cut the call into several batches, three
    of them with reads: every coverage then runs over all of them.  The model sees the two at length 1: a contig without
    reads decides nothing.  Then one such contig in front of the only contig with reads: two batches, the second the
    one with reads -- its columns are gathered once and every coverage's solve reuses them; with several batches with
    reads every coverage gathers each of them.  Depth at most 12"""
    huge = (1 << 31) - 3
    rng = np.random.default_rng(77)
    lengths = np.array([3000, 1800, 2400, 900], np.int64)
    ids = rng.integers(0, 4, 400).astype(np.uint32)
    span = rng.integers(1, 60, ids.size)
    s = (rng.random(ids.size) * (lengths[ids] - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    ids[rng.random(ids.size) < 0.04] = NO_CONTIG
    on = ids != NO_CONTIG
    ids[on] = np.array([0, 2, 3, 5], np.uint32)[ids[on]]
    wide = np.array([lengths[0], huge, lengths[1], lengths[2], huge, lengths[3]], np.uint32)
    cases = [(s, e, ids, wide, [1, 4], 3)]
    L, n = 3000, 400
    span = rng.integers(1, 60, n)
    s = (rng.random(n) * (L - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    ids = np.where(rng.random(n) < 0.04, NO_CONTIG, 1).astype(np.uint32)
    assert 0 < np.count_nonzero(ids == NO_CONTIG) < n // 4
    cases.append((s, e, ids, np.array([huge, L], np.uint32), [0], 1))
    for s, e, ids, wide, long_ones, live in cases:
        small = wide.copy()
        small[long_ones] = 1
        assert bm.depth(s, e, ids, small).max() <= 12
        for flags in (0, pkg.THRESHOLDS_WHOLE_PAIRS):
            want = tm.Thresholds(oracle, s, e, ids, small, 1, 12, whole_pairs=bool(flags))
            solver.set_profiling(True)
            try:
                thr, ts, counts = solver.solve_thresholds(s, e, ids, wide, 12, flags=flags, counts=True)
                kt = solver.kernel_times()
            finally:
                solver.set_profiling(False)
            check(want, thr, ts, counts)
            st = solver.last_stats
            assert st.n_contigs == wide.size and st.total_length == int(wide.astype(np.int64).sum())
            assert kt["k_bc_gather"][0] == (1 if live == 1 else live * ts.solves), (live, ts.solves, kt["k_bc_gather"])
            assert kt["k_bc_scatter_mask"][0] == live * ts.solves, (live, ts.solves, kt["k_bc_scatter_mask"])


def test_edges(pkg, oracle, solver):
    none = np.zeros(0, np.uint32)
    thr, ts, counts = solver.solve_thresholds(none, none, none, [100, 50], 10, counts=True)
    want = tm.Thresholds(oracle, none, none, none, [100, 50], 1, 10)
    check(want, thr, ts, counts)
    assert thr.size == 0 and counts.size == 10 and not counts.any()
    # every read unplaced
    s, e = np.array([3, 4, 5, 6], np.uint32), np.array([9, 9, 9, 9], np.uint32)
    off = np.full(4, NO_CONTIG, np.uint32)
    for flags in (0, pkg.THRESHOLDS_WHOLE_PAIRS):
        thr, ts = solver.solve_thresholds(s, e, off, [100], 10, flags=flags)
        check(tm.Thresholds(oracle, s, e, off, [100], 1, 10, whole_pairs=bool(flags)), thr, ts)
        assert np.all(thr == NEVER)
    # contigs of length 0 and contigs without reads between others; hi == lo; an odd read count
    rng = np.random.default_rng(55)
    lengths = np.array([0, 900, 0, 400, 700, 0, 1200, 0], np.uint32)
    ids = rng.choice([1, 4, 6], 3001).astype(np.uint32)
    span = rng.integers(1, 120, ids.size)
    s = (rng.random(ids.size) * (lengths[ids] - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    ids[rng.random(ids.size) < 0.05] = NO_CONTIG
    for lo, hi in ((1, 1), (7, 7), (1, 25), (3, 10_000), (60_000, tm.NEVER - 1)):
        want = tm.Thresholds(oracle, s, e, ids, lengths, lo, hi)
        thr, ts, counts = solver.solve_thresholds(s, e, ids, lengths, hi, coverage_lo=lo, counts=True)
        check(want, thr, ts, counts)
        assert np.array_equal(pkg.threshold_mask(thr, lo), solver.solve_by_contig(s, e, ids, lengths, lo))


# ------------------------------------------------------------------------------------------ 5: the device entry
def test_device_entry_equals_the_host_entry_and_waits_for_the_callers_stream(pkg, solver, mixed):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    for seed, flags in ((1, 0), (2, pkg.THRESHOLDS_WHOLE_PAIRS)):
        s, e, ids, lengths = mixed[seed]
        n = s.size & ~1
        s, e, ids = s[:n], e[:n], ids[:n]
        want, want_ts, want_counts = solver.solve_thresholds(s, e, ids, lengths, 30, coverage_lo=2, flags=flags, counts=True)
        side = torch.cuda.Stream(device=dev)
        d_s, d_e, d_ids = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
        src = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids)]
        d_thr = torch.full((n,), 7, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(4):                     # (the columns are still being written when the call is made)
                d_s.copy_(src[2]); d_e.copy_(src[0]); d_ids.copy_(src[1])
            d_s.copy_(src[0]); d_e.copy_(src[1]); d_ids.copy_(src[2])
            ts, counts = solver.solve_thresholds_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, 30,
                                                        d_thr.data_ptr(), coverage_lo=2, flags=flags, counts=True,
                                                        stream=side.cuda_stream)
        got = d_thr.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want) and np.array_equal(counts, want_counts)
        for f in ("reads_placed", "n_kept", "nesting_violations", "coverage_lo", "coverage_hi", "top", "solves", "saturated",
                  "count_entries"):
            assert getattr(ts, f) == getattr(want_ts, f), f


# ------------------------------------------------------------------------------------------ 6: bad input
def test_a_bad_read_or_contig_id_has_the_by_contig_code_and_leaves_the_output_alone(pkg, solver):
    torch = pytest.importorskip("torch")
    s = np.array([0, 5, 9, 1], np.uint32)
    e = np.array([3, 8, 9, 2], np.uint32)
    cases = [(np.array([0, 2, 0, 0], np.uint32), [10, 10], pkg.QMCP_EINVAL),     # id 2 of 2 contigs
             (np.array([0, 1, 1, 0], np.uint32), [10, 9], pkg.QMCP_EREAD),       # end 9 on a 9-position contig
             (np.array([0, 0, 0, 0], np.uint32), [10, 1 << 31], pkg.QMCP_ERANGE)]
    dev = torch.device("cuda", 0)
    for ids, lengths, code in cases:
        with pytest.raises(pkg.QmcpError) as by_contig:
            solver.solve_by_contig(s, e, ids, lengths, 2)
        assert by_contig.value.code == code
        thr = np.full(4, 0xABCD, np.uint16)
        table = np.full(2, 0x77, np.uint64)
        lens = np.asarray(lengths, np.uint32)
        rc = pkg._hip.qmcp_hip_solve_thresholds_host(solver._ctx, pkg._p32(s), pkg._p32(e), pkg._p32(ids), 4,
                                                     pkg._p32(lens), lens.size, 1, 5, 0, thr.ctypes.data_as(pkg._u16p),
                                                     pkg._p64(table), 2, pkg.Stats(), pkg.ThresholdsStats())
        assert rc == code and np.all(thr == 0xABCD) and np.all(table == 0x77)
        d = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids)]
        d_thr = torch.full((4,), 0x1234, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        with pytest.raises(pkg.QmcpError) as ex:
            solver.solve_thresholds_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 4, lengths, 5, d_thr.data_ptr())
        assert ex.value.code == code and d_thr.cpu().tolist() == [0x1234] * 4
    # the context is whole afterwards
    thr, ts = solver.solve_thresholds(s, e, np.zeros(4, np.uint32), [10], 5)
    assert ts.saturated == 1 and ts.n_kept == 4 and thr.max() <= ts.top


# ------------------------------------------------------------------------------------------ 7: the file flow
def test_downsample_bam_thresholds_tag_every_downsample_of_the_range(pkg, oracle, solver, tmp_path):
    path = tmp_path / "in.bam"
    refs = [("chrA", 5000), ("chrB", 3000), ("chrC", 1200)]
    header, parsed, _ = mr.write_multi_reference_bam(path, np.random.default_rng(23), refs, 1500)
    cols = pkg.read_bam(path, per_reference=True)                                 # the budget flow's pairing
    s, e, ids, lengths = cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"]
    bam_ids = np.asarray(cols["bam_ids"], np.int64)
    assert s.size % 2 == 0 and s.size > 2000
    lo, hi = 2, 25
    want = tm.Thresholds(oracle, s, e, ids, lengths, lo, hi, whole_pairs=True)
    assert want.saturated == 0 and want.top == hi                                 # some reads need more than hi
    out, report = tmp_path / "out.bam", tmp_path / "thresholds.tsv"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, 1, per_reference=True, thresholds=(lo, hi),
                                 thresholds_report=report)
    oh, orecs, _ = bam_py.parse(out)
    tagged = np.flatnonzero(want.thresholds <= hi)
    order = tagged[np.argsort(bam_ids[tagged])]                                   # file order
    assert oh == header and written == len(orecs) == tagged.size == want.n_kept
    tags = []
    for rec, i in zip(orecs, order.tolist()):                                     # the record plus its five tag bytes
        raw = parsed[bam_ids[i]]["raw"]
        assert rec["raw"][4:-5] == raw[4:] and rec["raw"][-5:-2] == b"XCS", i
        assert int.from_bytes(rec["raw"][:4], "little") == int.from_bytes(raw[:4], "little") + 5
        tags.append(int.from_bytes(rec["raw"][-2:], "little"))
    tags = np.array(tags)
    assert np.array_equal(tags, want.thresholds[order]) and tags.min() == lo and tags.max() <= hi
    for M in (lo, 9, hi):                                                         # a filter on the tag is the downsample at M
        kept = bm.complete_pairs(want.model.bits(M), ids)                         # what the budget flow writes at M
        kept_ids = np.sort(bam_ids[np.flatnonzero(kept)])
        filtered = [r["raw"][:-5] for r, t in zip(orecs, tags.tolist()) if t <= M]
        assert [raw[4:] for raw in filtered] == [parsed[i]["raw"][4:] for i in kept_ids.tolist()], M
    # the report parses back to the stats and the counts
    lines = report.read_text().splitlines()
    split = lines.index("#M\treads")
    rows = dict(line.split("\t") for line in lines[:split] if not line.startswith("#"))
    assert set(rows) == {name for name, _ in pkg.ThresholdsStats._fields_} | {"records_written"}
    assert int(rows["records_written"]) == written == int(rows["n_kept"]) and int(rows["reads_placed"]) == want.model.placed
    assert (int(rows["coverage_lo"]), int(rows["coverage_hi"]), int(rows["top"]), int(rows["solves"])) == (lo, hi, want.top, want.solves)
    assert int(rows["nesting_violations"]) == want.violations and int(rows["saturated"]) == want.saturated
    table = np.array([line.split("\t") for line in lines[split + 1:]], dtype=np.uint64)
    assert np.array_equal(table[:, 0], np.arange(lo, hi + 1)) and np.array_equal(table[:, 1], want.counts())
    # hi alone means 1 .. hi, another tag; SAM text shows it
    sam = tmp_path / "out.sam"
    written2 = pkg.downsample_bam("quasi-mcp-hip", path, sam, 1, per_reference=True, thresholds=6, thresholds_tag="xd")
    want2 = tm.Thresholds(oracle, s, e, ids, lengths, 1, 6, whole_pairs=True)
    body = [line for line in sam.read_text().splitlines() if not line.startswith("@")]
    assert written2 == len(body) == want2.n_kept
    order2 = np.flatnonzero(want2.thresholds <= 6)
    order2 = order2[np.argsort(bam_ids[order2])]
    assert [line.rsplit("\t", 1)[1] for line in body] == [f"xd:i:{t}" for t in want2.thresholds[order2].tolist()]
    # an input that carries the tag already is refused before anything is written
    with pytest.raises(ValueError, match="already carries the tag XC"):
        pkg.downsample_bam("quasi-mcp-hip", out, tmp_path / "no.bam", 1, per_reference=True, thresholds=5)
    assert not (tmp_path / "no.bam").exists()


# ------------------------------------------------------------------------------------------ 8: the cost
def test_the_thresholds_call_takes_no_longer_than_the_callers_loop(pkg, solver):
    """2 M reads on 8 contigs (the ladder test's shape), thresholds 1 .. 32; median of 5 runs after a warm-up, the two
    alternating in this process, timed by the wall clock around blocking calls.  The loop is the only route without the
    entry: solve_by_contig_device per coverage -- it regroups the reads every time -- and a torch where / minimum that
    accumulates the smallest keeping coverage"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    n_contigs, pairs, L, lo, hi = 8, 125_000, 20_000, 1, 32
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, seed=500 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
    perm = np.random.default_rng(8).permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    n = s.size
    lengths = np.full(n_contigs, L, np.uint32)
    d_s, d_e, d_ids = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids))
    d_thr = torch.zeros(n, dtype=torch.int16, device=dev)
    mask = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev)
    shifts = torch.arange(64, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    found = {}

    def thresholds_call():
        found["call"] = solver.solve_thresholds_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, hi,
                                                       d_thr.data_ptr(), coverage_lo=lo, stream=stream)
        torch.cuda.synchronize()

    def callers_loop():
        acc = torch.full((n,), NEVER, dtype=torch.int32, device=dev)
        for M in range(lo, hi + 1):
            torch.cuda.synchronize()
            solver.solve_by_contig_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, M, mask.data_ptr(),
                                          stream=stream)
            kept = ((mask.unsqueeze(1) >> shifts) & 1).reshape(-1)[:n].bool()
            acc = torch.minimum(acc, torch.where(kept, M, NEVER).to(torch.int32))
        torch.cuda.synchronize()
        found["loop"] = acc

    thresholds_call()
    callers_loop()
    ts = found["call"]
    got = d_thr.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, found["loop"].cpu().numpy().astype(np.uint16))     # the same array either way
    assert ts.top == hi and ts.solves == hi - lo + 1 and ts.n_kept == int((got <= hi).sum()) > 0
    t_call, t_loop = [], []
    for _ in range(5):
        for f, times in ((thresholds_call, t_call), (callers_loop, t_loop)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times.append((time.perf_counter() - t0) * 1e3)
    t_call, t_loop = sorted(t_call)[2], sorted(t_loop)[2]
    print(f"thresholds call {t_call:.3f} ms, caller's loop {t_loop:.3f} ms; {ts.as_dict()}")
    assert t_call <= t_loop, (t_call, t_loop, ts.as_dict())
