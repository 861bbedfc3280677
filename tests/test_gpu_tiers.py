"""qmcp_hip_solve_tiers_*: the best tier first, later tiers only where the earlier ones leave the depth short.  Every mask
is compared bit for bit with the model (tests/tiers_model.py, on tests/profile_model.py), and every row and counter with
it.  The shapes are the smallest at which each path is taken: several contigs and tiers, stretches without tier 0, deep
one-length data (tier 0 on the one-length route, later tiers asked for nothing or only inside a stretch), two position
batches, 16 tiers."""
import ctypes as C

import numpy as np
import pytest

import profile_model as pm
import tiers_model as tm

pytestmark = pytest.mark.gpu


def check(solver, s, e, ids, tiers, lengths, M, n_tiers, model_on=None, batches=1):
    """one host call against the model (model_on: the same instance on short contigs) -> the kept bits"""
    got = solver.solve_tiers(s, e, ids, tiers, lengths, M, n_tiers)
    ms, me, mids, mlengths = (s, e, ids, lengths) if model_on is None else model_on
    want, rows, _ = tm.tiered(ms, me, mids, tiers, mlengths, M, n_tiers, fast=True)
    n = np.asarray(s).size
    assert got.size == (n + 63) // 64 and np.array_equal(got, pm.pack(want)), (n, M, n_tiers)
    have = tm.rows_of(solver.last_tier_rows)
    assert have.shape == rows.shape and np.array_equal(have, rows), (have, rows)
    ts, st = solver.last_tiers_stats, solver.last_stats
    assert ts.n_tiers == n_tiers and ts.tiers_used == int((rows[:, 1] > 0).sum())
    assert ts.reads_untiered == tm.untiered(tiers)
    assert st.n_kept == rows[0, 1] and st.n_reads == rows[0, 0]           # stats are tier 0's solver calls
    for t, row in enumerate(solver.last_tier_rows):
        if t == 0:                                                        # tier 0: its solver calls
            assert (1 if rows[0, 0] and M else 0) <= row.sweeps <= (batches if rows[0, 0] and M else 0)
        elif rows[t, 4] == 0:
            assert row.sweeps == 0 and row.n_kept == 0                    # nothing asked: no sweep is queued
        else:
            assert 1 <= row.sweeps <= batches
    return want


def mixed(seed, repeat, n=2000):
    rng = np.random.default_rng(600 + seed)
    lengths = np.array([300, 500], np.uint32)
    repeats = [(1, 200, 299)] if repeat else []
    s, e, ids, tiers = tm.instance(rng, lengths, n, (20, 60), [70, 20, 10], repeats)
    return s, e, ids, tiers, lengths


def test_edge_inputs(solver):
    rng = np.random.default_rng(1)
    lengths = np.array([400, 90, 300], np.uint32)
    none = np.zeros(0, np.uint32)
    kept = check(solver, none, none, none, none, lengths, 4, 3)                            # no reads
    assert kept.size == 0 and solver.last_tiers_stats.tiers_used == 0
    s, e, ids, tiers = tm.instance(rng, lengths, 500, (1, 70), [5, 3, 2])
    ids[ids == 1] = 2                                              # an empty contig (its reads fit the longer one)
    assert check(solver, s, e, ids, tiers, lengths, 4, 3).any()
    kept = check(solver, s, e, ids, np.full(500, tm.NO_TIER, np.uint32), lengths, 4, 3)   # all NO_TIER
    assert not kept.any() and solver.last_tiers_stats.reads_untiered == 500
    kept = check(solver, s, e, np.full(500, tm.NO_CONTIG, np.uint32), tiers, lengths, 4, 3)   # all NO_CONTIG
    assert not kept.any() and solver.last_stats.n_reads == 0
    gap = np.where(tiers == 1, 3, tiers).astype(np.uint32)                                 # tiers 1 and 2 of 5 have no reads
    gap[gap == 2] = 4
    kept = check(solver, s, e, ids, gap, lengths, 4, 5)
    assert kept[gap == 3].any() and solver.last_tier_rows[1].n_reads == 0 == solver.last_tier_rows[2].n_reads
    for n in (1, 63, 64, 65, 129):                                                         # the mask's word edges
        check(solver, s[:n], e[:n], ids[:n], tiers[:n], lengths, 2, 3)
    assert not check(solver, s, e, ids, tiers, lengths, 0, 3).any()                        # M = 0 keeps nothing


def test_one_tier_is_the_plain_by_contig_call(solver):
    for seed, M in ((0, 1), (1, 5), (2, 40)):
        s, e, ids, _, lengths = mixed(seed, False)
        ids[::37] = tm.NO_CONTIG
        plain = solver.solve_by_contig(s, e, ids, lengths, M)
        n_kept, n_reads, path = solver.last_stats.n_kept, solver.last_stats.n_reads, solver.last_stats.path
        got = solver.solve_tiers(s, e, ids, np.zeros(s.size, np.uint32), lengths, M, 1)
        assert np.array_equal(got, plain)
        st, row = solver.last_stats, solver.last_tier_rows[0]
        assert st.n_kept == n_kept == row.n_kept and st.n_reads == n_reads == row.n_reads and st.path == path
        assert st.n_contigs == 2 and st.total_length == 800


@pytest.mark.parametrize("cut_points", [-1, 1])
@pytest.mark.parametrize("repeat", [False, True])
def test_mixed_spans_three_tiers(solver, repeat, cut_points):
    s, e, ids, tiers, lengths = mixed(3, repeat)
    with solver.options(cut_points=cut_points):
        want = check(solver, s, e, ids, tiers, lengths, 5, 3)
    assert tm.covers(s, e, ids, tiers, lengths, 5, 3, want)
    rows = solver.last_tier_rows
    assert rows[0].n_kept > 0 and rows[0].demand == 0
    if repeat:                                                   # the stretch can only be filled from tiers 1 and 2
        assert rows[1].n_kept > 0 and rows[1].demand > 0 and rows[1].asked_positions >= 100
        later = np.flatnonzero(want & (tiers > 0) & (ids == 1))
        assert ((e[later] >= 200) & (s[later] <= 299)).sum() > later.size / 2


def deep(rng, absent):
    L, span, M = 2000, 50, 10
    n = 12 * (L - span + 1)
    s = rng.integers(0, L - span + 1, size=n).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    tiers = tm.draw_tiers(rng, n, [90, 8, 2])
    if absent:
        hit = np.flatnonzero((tiers == 0) & (s <= absent[1]) & (e >= absent[0]))
        tiers[hit] = 1 + tm.draw_tiers(rng, hit.size, [8, 2])
    return s, e, np.zeros(n, np.uint32), tiers, np.array([L], np.uint32), M


def test_deep_one_length_data(pkg, solver):
    """tier 0 alone reaches M nearly everywhere: it takes the one-length route, and a later tier whose need is zero in
    the model queues no sweep; with tier 0 absent on [800, 1000) tiers 1 and 2 are asked there only"""
    s, e, ids, tiers, lengths, M = deep(np.random.default_rng(11), None)
    want = check(solver, s, e, ids, tiers, lengths, M, 3)
    assert solver.last_stats.path == pkg.PATH_UNIFORM
    rows = solver.last_tier_rows
    assert want.sum() < s.size / 20 and rows[1].asked_positions < 200 and rows[2].asked_positions <= rows[1].asked_positions
    s, e, ids, tiers, lengths, M = deep(np.random.default_rng(12), (800, 999))
    want = check(solver, s, e, ids, tiers, lengths, M, 3)
    assert solver.last_stats.path == pkg.PATH_UNIFORM
    rows = solver.last_tier_rows
    assert rows[1].sweeps == 1 and rows[1].asked_positions >= 200 and rows[1].capped_positions > 1500
    later = np.flatnonzero(want & (tiers > 0) & (s > 60) & (e < 2000 - 60))      # (the contig's thin ends aside)
    assert later.size and ((e[later] >= 800 - 50) & (s[later] <= 999 + 50)).all()
    assert tm.covers(s, e, ids, tiers, lengths, M, 3, want)


def test_tier_0_empty_on_one_contig(solver):
    """guarantee 4: on the contig without tier-0 reads tier 1 is solved with zero credit, which is the by-contig solve of
    those reads"""
    s, e, ids, tiers, lengths = mixed(5, False)
    tiers[(ids == 0) & (tiers == 0)] = 1
    want = check(solver, s, e, ids, tiers, lengths, 5, 3)
    on = np.flatnonzero((ids == 0) & (tiers == 1))
    alone = pm.unpack(solver.solve_by_contig(s[on], e[on], ids[on], lengths, 5), on.size)
    assert np.array_equal(want[on], alone) and alone.any()


def test_sixteen_tiers(solver):
    rng = np.random.default_rng(16)
    lengths = np.array([250, 350], np.uint32)
    s, e, ids, _ = tm.instance(rng, lengths, 3200, (10, 50), [1])
    tiers = rng.permutation(np.repeat(np.arange(16, dtype=np.uint32), 200))
    check(solver, s, e, ids, tiers, lengths, 40, 16)
    assert solver.last_tiers_stats.tiers_used >= 3


def test_kept_list_grows_and_keeps_its_entries(pkg):
    """thin data, nearly every read kept: on a fresh context the kept list starts at tier 0's kept count and has to grow
    while it holds tier 0's entries; the last tier's credit reads what was moved"""
    rng = np.random.default_rng(21)
    lengths = np.array([120_000, 80_000], np.uint32)
    s, e, ids, _ = tm.instance(rng, lengths, 18_000, (5, 30), [1])
    tiers = rng.permutation(np.repeat(np.arange(3, dtype=np.uint32), 6000))
    with pkg.Solver(0) as fresh:
        want = check(fresh, s, e, ids, tiers, lengths, 3, 3)
        rows = fresh.last_tier_rows
        assert rows[0].n_kept > 5000 and rows[1].n_kept > 4096 and rows[2].n_kept > 1000
        assert rows[0].n_kept + rows[1].n_kept > max(4096, s.size // 32, rows[0].n_kept)      # the list had to grow
    assert tm.covers(s, e, ids, tiers, lengths, 3, 3, want)


def raw_host(pkg, solver, s, e, ids, tiers, lengths, M, n_tiers, mask, null_tiers=False, n_contigs=None):
    """the host entry itself, on a mask buffer the caller owns -> status code"""
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    return pkg._hip.qmcp_hip_solve_tiers_host(solver._ctx, p(s), p(e), p(ids), None if null_tiers else p(tiers), s.size,
                                              p(lengths), lengths.size if n_contigs is None else n_contigs, M, n_tiers,
                                              mask.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, None)


def test_errors_leave_the_mask_alone_and_the_context_usable(pkg, solver):
    torch = pytest.importorskip("torch")
    s = np.array([0, 5, 9, 2], np.uint32)
    e = np.array([3, 8, 9, 6], np.uint32)
    ids = np.array([0, 1, 1, 0], np.uint32)
    tiers = np.array([0, 1, 1, 0], np.uint32)
    lengths = [10, 10]
    guard = np.uint64(0xA5A5A5A5A5A5A5A5)

    def good():
        # at M = 1 every read is needed: 0-3 and 2-6 each cover positions of contig 0 alone, 5-8 and 9-9 do not overlap
        assert pm.unpack(solver.solve_tiers(s, e, ids, tiers, lengths, 1, 2), 4).all()

    assert 16 * ((1 << 20) + 1) > 1 << 24
    long_lengths = np.full((1 << 20) + 1, 10, np.uint32)
    cases = [
        (dict(), 1, 0, pkg.QMCP_EINVAL, "n_tiers"),
        (dict(), 1, 17, pkg.QMCP_ERANGE, "17"),
        (dict(lengths=long_lengths), 1, 16, pkg.QMCP_ERANGE, str(16 * ((1 << 20) + 1))),
        (dict(), 1 << 31, 2, pkg.QMCP_ERANGE, "max_coverage"),
        (dict(null_tiers=True), 1, 2, pkg.QMCP_EINVAL, "tiers"),
        (dict(n_contigs=0), 1, 2, pkg.QMCP_EINVAL, "n_contigs"),
        # found on the device: the context's mask is cleared, keep_mask_out is not written
        (dict(tiers=np.array([0, 2, 1, 0], np.uint32)), 1, 2, pkg.QMCP_EINVAL, "tier id"),
        (dict(ids=np.array([0, 2, 1, 0], np.uint32)), 1, 2, pkg.QMCP_EINVAL, "contig id"),
        (dict(lengths=[10, 9]), 1, 2, pkg.QMCP_EREAD, "read"),
    ]
    for kwargs, M, n_tiers, code, word in cases:
        args = dict(s=s, e=e, ids=ids, tiers=tiers, lengths=lengths)
        extra = {k: kwargs.pop(k) for k in ("null_tiers", "n_contigs") if k in kwargs}
        args.update(kwargs)
        mask = np.full(4, guard, np.uint64)
        rc = raw_host(pkg, solver, args["s"], args["e"], args["ids"], args["tiers"], args["lengths"], M, n_tiers, mask, **extra)
        assert rc == code, (kwargs, extra, rc)
        assert word in pkg._hip.qmcp_hip_last_error().decode(), pkg._hip.qmcp_hip_last_error()
        assert (mask == guard).all(), (kwargs, extra)
        good()
    # the device entry: a bad tier id is found on the device; the mask's own word is cleared, nothing beyond it
    dev = torch.device("cuda", 0)
    bad = np.array([0, 7, 1, 0], np.uint32)
    t = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids, bad)]
    d_mask = torch.full((4,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_tiers_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), 4, lengths, 1, 2,
                                  d_mask.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    assert ex.value.code == pkg.QMCP_EINVAL and "tier" in str(ex.value)
    got = d_mask.cpu().numpy()
    assert got[0] == 0 and (got[1:] == -0x5A5A5A5A5A5A5A5B).all()
    good()


def test_two_position_batches_sum_their_counters(solver):
    """two contigs of about 1.2e9 positions (one call takes 2^31 - 2) and a short third: every tier is two batches, whose
    counters add up; a batch of tier 1 takes from the kept list the entries on its own contigs.  Under stretches only
    (as one chain per contig the walks over 1.2e9 positions take seconds)"""
    from test_gpu_proportional import two_batch_instance
    inst, small = two_batch_instance()
    lengths = inst[3].astype(np.int64)
    assert int(lengths[:2].sum()) > (1 << 31) - 2 >= int(lengths[1:].sum())
    tiers = tm.draw_tiers(np.random.default_rng(8), inst[0].size, [6, 4])
    with solver.options(cut_points=1):
        want = check(solver, inst[0], inst[1], inst[2], tiers, inst[3], 3, 2, model_on=small, batches=2)
    rows = solver.last_tier_rows
    assert rows[0].sweeps == 2 and rows[1].sweeps == 2 and rows[1].n_kept > 0
    assert solver.last_stats.total_length == int(lengths.sum()) and solver.last_stats.n_contigs == 3
    for c in range(3):
        assert (want & (tiers == 1) & (inst[2] == c)).any()          # tier 1 fills gaps on every contig


def test_device_entry_on_a_side_stream_aligned_and_one_element_off(pkg, solver):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    guard = -0x0123456789ABCDEF
    s, e, ids, tiers, lengths = mixed(7, True)
    tiers[::53] = tm.NO_TIER
    ids[::41] = tm.NO_CONTIG
    want, rows, _ = tm.tiered(s, e, ids, tiers, lengths, 5, 3, fast=True)
    n, words = s.size, pkg.mask_words(s.size)
    side = torch.cuda.Stream(device=dev)
    for shift in (0, 1):
        with torch.cuda.stream(side):
            cols = []
            for x in (s, e, ids, tiers):
                t = torch.zeros(n + shift + 4, dtype=torch.int32, device=dev)   # (a base allocation is 256-byte aligned)
                t[shift:shift + n] = torch.from_numpy(x.view(np.int32)).to(dev, non_blocking=True)
                cols.append(t)
            d_mask = torch.full((words + 3,), guard, dtype=torch.int64, device=dev)
            ptr = [t.data_ptr() + 4 * shift for t in cols]
            assert all(p % 16 == 4 * shift for p in ptr)
            st = solver.solve_tiers_device(ptr[0], ptr[1], ptr[2], ptr[3], n, lengths, 5, 3, d_mask.data_ptr(),
                                           stream=side.cuda_stream)
        side.synchronize()
        got = d_mask.cpu().numpy()
        assert np.array_equal(got[:words].view(np.uint64), pm.pack(want)), f"shift {shift}"
        assert (got[words:] == guard).all()                                  # nothing beyond ceil(n / 64) words
        assert st.n_kept == rows[0, 1]
        assert np.array_equal(tm.rows_of(solver.last_tier_rows), rows)
        assert solver.last_tiers_stats.reads_untiered == tm.untiered(tiers)


@pytest.mark.parametrize("bands,min_mapq", [([30, 10, 0], 0), ([30, 10], 10)])
def test_file_to_file(pkg, oracle, solver, tmp_path, bands, min_mapq):
    """downsample_bam(per_reference=True, mapq_tiers=...): one ingest, one tiered solve on the reads that passed it,
    find_pairs, the write -- the written records are find_pairs of the model's mask on read_bam's columns, the depth is
    >= min(coverage, M) everywhere, the lower bands' records lie in or next to the stretch the best band cannot fill,
    and the report's lines are the model's rows, records_written and mates_added"""
    import bam_py
    path = tmp_path / "bands.bam"
    header, parsed, ref_lengths = tm.write_tiers_bam(path, np.random.default_rng(29))
    cols = pkg.read_bam(path, per_reference=True, min_mapq=min_mapq)
    n, M = cols["starts"].size, 6
    ids, lengths = cols["contig_ids"], cols["contig_lengths"]
    placed = ids != tm.NO_CONTIG
    s, e = np.where(placed, cols["starts"], 0).astype(np.uint32), np.where(placed, cols["ends"], 0).astype(np.uint32)
    tiers = pkg.tiers_from_mapq(cols["qualities"], bands)
    assert (tiers != tm.NO_TIER).all() and all((tiers == t).any() for t in range(len(bands)))
    keep, rows, _ = tm.tiered(s, e, ids, tiers, lengths, M, len(bands), fast=True)
    assert 0 < keep.sum() < placed.sum() and rows[1, 1] > 0
    out, tsv = tmp_path / "out.bam", tmp_path / "tiers.tsv"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, min_mapq=min_mapq, mapq_tiers=bands,
                                 tiers_report=tsv)
    mask = oracle.find_pairs(pm.pack(keep), n)
    final = pm.unpack(mask, n)
    kept_ids = np.sort(cols["bam_ids"][np.flatnonzero(final)].astype(np.int64))
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == kept_ids.size == len(orecs)
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]
    assert tm.covers(s, e, ids, tiers, lengths, M, len(bands), final)          # completion only adds reads
    ref, a, b = tm.LOW_STRETCH
    later = np.flatnonzero(keep & (tiers > 0) & (ids == ref) & (s > 200) & (e < lengths[ref] - 200))
    assert later.size > 10 and ((e[later] >= a - 150) & (s[later] <= b + 150)).all()
    # the report: the host's lines, and write_tiers_report's for the same rows from the Python entry
    lines = [l.split("\t") for l in open(tsv).read().splitlines() if not l.startswith("#")]
    assert [l[1] for l in lines[:len(bands)]] == [f"mapq>={q}" for q in bands]
    assert [[int(x) for x in l[2:4] + l[6:8]] for l in lines[:len(bands)]] == rows[:, [0, 1, 4, 5]].tolist()
    total = float(sum(ref_lengths))
    for l, row in zip(lines, rows):
        assert abs(float(l[4]) - row[2] / total) < 1e-5 and abs(float(l[5]) - row[3] / total) < 1e-5
    assert lines[len(bands):] == [["records_written", str(written)], ["mates_added", str(int(final.sum() - keep.sum()))]]
    solver.solve_tiers(s, e, ids, tiers, lengths, M, len(bands))
    again = tmp_path / "again.tsv"
    pkg.write_tiers_report(again, solver.last_tier_rows, [f"mapq>={q}" for q in bands], total, written,
                           int(final.sum() - keep.sum()))
    assert open(again).read() == open(tsv).read()
