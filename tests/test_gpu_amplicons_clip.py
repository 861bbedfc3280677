"""qmcp_hip_solve_amplicons_*: every unit assigned to one amplicon of its contig, its reads clipped to the insert, the
clipped reads solved pooled or per amplicon.  Keep mask, labels, rows and statistics are compared bit for bit with the
literal model on the oracle (tests/amplicon_clip_model.py), through the host entry and through the device entry."""
import ctypes as C

import numpy as np
import pytest

import amplicon_clip_model as am
import amplicon_panels as ap
import multi_reference as mr

pytestmark = pytest.mark.gpu

NO = mr.NO_CONTIG
REFS = [("seg_a", 2500), ("seg_empty", 900), ("seg_b", 1300), ("seg_c", 700)]
LENGTHS = [L for _, L in REFS]
PRIMER = 25


def tiled_tables(step=300, size=400):
    """a tiled panel over seg_a and seg_b (consecutive amplicons overlap by size - step), none on seg_empty, exactly one
    on seg_c; 25-base primers -> (offs, a0, a1, i0, i1)"""
    panel = ap.tiled_panel([REFS[0], REFS[2]], 20, size=size, step=step)
    panel["seg_c"] = [(100, 599)]
    offs, a0, a1 = ap.panel_csr(panel, [n for n, _ in REFS])
    return offs, a0, a1, a0 + PRIMER, a1 - PRIMER


def fragment_units(rng, n_units, offs, a0, a1, pairs, flush=0.4, cross=0.03, unplaced=0.03, outside=0.05):
    """units drawn from the amplicons: reads of 10 - 200 bases inside their amplicon, a share flush with one of its
    edges (so the primers are hit), some in the overlap of two amplicons, some poking one base outside, some with a mate
    on another contig or unplaced, some on the contig without amplicons -> (starts, ends, ids)"""
    per = 2 if pairs else 1
    n_amp = a0.size
    contig_of = np.repeat(np.arange(len(LENGTHS)), np.diff(offs.astype(np.int64)))
    k = rng.integers(0, n_amp, size=n_units)
    lo, hi = a0.astype(np.int64)[k], a1.astype(np.int64)[k]
    s = np.zeros((n_units, per), np.int64)
    e = np.zeros((n_units, per), np.int64)
    for m in range(per):
        span = rng.integers(10, 201, size=n_units)
        st = lo + (rng.random(n_units) * (hi - lo + 2 - span)).astype(np.int64)
        edge = rng.random(n_units)
        st = np.where(edge < flush / 2, lo, np.where(edge < flush, hi - span + 1, st))
        s[:, m], e[:, m] = st, st + span - 1
    ids = np.repeat(contig_of[k][:, None], per, axis=1).astype(np.int64)
    out = np.flatnonzero(rng.random(n_units) < outside)                    # one base outside, on either side
    left = rng.random(out.size) < 0.5
    s[out, 0] = np.where(left, np.maximum(lo[out] - 1, 0), s[out, 0])
    e[out, 0] = np.where(left, e[out, 0], np.minimum(hi[out] + 1, np.asarray(LENGTHS)[ids[out, 0]] - 1))
    s = np.minimum(s, e)
    bare = np.flatnonzero(rng.random(n_units) < 0.04)                      # the contig without amplicons
    ids[bare] = 1
    s[bare], e[bare] = 10, 120
    if pairs:
        other = np.flatnonzero(rng.random(n_units) < cross)
        ids[other, 1] = (ids[other, 0] + 2) % 4
        s[other, 1], e[other, 1] = 5, 80
    un = rng.random((n_units, per)) < unplaced
    ids[un] = NO
    return s.reshape(-1).astype(np.uint32), e.reshape(-1).astype(np.uint32), ids.reshape(-1).astype(np.uint32)


def check(solver, oracle, s, e, ids, lengths, M, offs, a0, a1, i0=None, i1=None, what="", **kw):
    """the host entry against the model: mask, labels, rows and stats -> (keep bits, stats dict)"""
    mask, lab, rows, st = solver.solve_amplicons(s, e, ids, lengths, M, offs, a0, a1, insert_starts=i0, insert_ends=i1,
                                                 **kw)
    keep_w, lab_w, rows_w, st_w = am.solve(oracle, s, e, ids, lengths, M, offs, a0, a1, i0, i1, **kw)
    assert {k: st[k] for k in am.STAT_KEYS} == st_w, f"{what}: stats"
    assert np.array_equal(lab, lab_w), f"{what}: labels"
    assert np.array_equal(mask, am.pack(keep_w)), f"{what}: keep mask"
    assert [tuple(int(x) for x in r) for r in rows.tolist()] == rows_w, f"{what}: rows"
    assert st["units"] == st["units_assigned"] + st["units_filtered"] + st["units_no_amplicon"]
    return keep_w, st


@pytest.mark.parametrize("pairs, complete", [(True, False), (True, True), (False, False)])
@pytest.mark.parametrize("per_amplicon", [False, True])
def test_modes_on_a_tiled_panel(solver, oracle, per_amplicon, pairs, complete):
    rng = np.random.default_rng(5 + 2 * per_amplicon + pairs)
    offs, a0, a1, i0, i1 = tiled_tables()
    s, e, ids = fragment_units(rng, 1500, offs, a0, a1, pairs)
    n = s.size
    sl = rng.integers(20, 200, size=n).astype(np.uint32)
    mq = rng.integers(0, 61, size=n).astype(np.uint32)
    _, st = check(solver, oracle, s, e, ids, LENGTHS, 6, offs, a0, a1, i0, i1, seq_lengths=sl, qualities=mq,
                  min_length=30, min_mapq=5, single_end=not pairs, per_amplicon=per_amplicon, complete_pairs=complete)
    assert st["units_in_several"] > 0 and st["units_no_amplicon"] > 0 and st["units_filtered"] > 0
    assert st["reads_shortened"] > 0 and st["reads_clipped_away"] > 0 and st["amplicons_unused"] == 0


@pytest.mark.parametrize("pairs", [True, False])
@pytest.mark.parametrize("n_units", [0, 1, 63, 64, 65, 129])
def test_unit_counts_at_the_ballot_word_edges(solver, oracle, n_units, pairs):
    rng = np.random.default_rng(40 + n_units)
    offs, a0, a1, i0, i1 = tiled_tables()
    s, e, ids = fragment_units(rng, n_units, offs, a0, a1, pairs)
    for per_amplicon in (False, True):
        check(solver, oracle, s, e, ids, LENGTHS, 2, offs, a0, a1, i0, i1, single_end=not pairs,
              per_amplicon=per_amplicon, complete_pairs=pairs, what=f"{n_units} units")


def test_every_kind_of_clip(solver, oracle):
    """one amplicon [100, 499] with insert [125, 474] on seg_a: reads clipped on the left, on the right, on both sides,
    to one base, and away; a pair with both mates clipped away; pairs whose clipped-away mate only comes back through
    completion.  M is above the depth, so the solve keeps exactly the reads that are still placed"""
    offs = np.array([0, 1, 1, 1, 1], np.uint32)
    a0, a1, i0, i1 = (np.array([x], np.uint32) for x in (100, 499, 125, 474))
    pairs = [((100, 200), (300, 400)),      # left clip, untouched
             ((300, 499), (200, 250)),      # right clip
             ((100, 499), (110, 480)),      # both sides, twice
             ((100, 125), (474, 499)),      # to one base each
             ((100, 124), (130, 140)),      # mate 1 away
             ((100, 110), (480, 499)),      # both away
             ((475, 499), (126, 473))]      # mate 1 away
    s = np.array([r[0] for p in pairs for r in p], np.uint32)
    e = np.array([r[1] for p in pairs for r in p], np.uint32)
    ids = np.zeros(s.size, np.uint32)
    for per_amplicon in (False, True):
        for complete in (False, True):
            keep, st = check(solver, oracle, s, e, ids, LENGTHS, 20, offs, a0, a1, i0, i1, per_amplicon=per_amplicon,
                             complete_pairs=complete)
            assert st["reads_clipped_away"] == 4 and st["reads_shortened"] == 6 and st["units_assigned"] == 7
            assert st["bases_clipped"] == 25 + 25 + 50 + (15 + 6) + 25 + 25 + 25 + 11 + 20 + 25
            away = np.zeros(14, bool)
            away[[8, 10, 11, 12]] = True
            assert keep[~away].all() and not keep[10] and not keep[11]  # both mates away: never kept
            assert keep[8] == keep[12] == complete                      # a mate clipped away returns by completion only
    # single reads: the same reads, one unit each
    _, st = check(solver, oracle, s, e, ids, LENGTHS, 20, offs, a0, a1, i0, i1, single_end=True)
    assert st["units"] == 14 and st["reads_clipped_away"] == 4


def test_assignment_rule_on_nested_and_duplicated_amplicons(solver, oracle):
    """greatest start, then smallest end, then smallest index -- with a table the caller gives unsorted"""
    offs = np.array([0, 7, 7, 7, 7], np.uint32)
    a0 = np.array([300, 0, 200, 200, 200, 0, 250], np.uint32)
    a1 = np.array([900, 2000, 800, 700, 700, 2000, 400], np.uint32)
    s = np.array([210, 210, 310, 260, 0, 5, 750, 901, 200, 700], np.uint32)
    e = np.array([300, 750, 320, 300, 9, 1999, 900, 950, 200, 700], np.uint32)     # (the last read: [700, 700])
    ids = np.zeros(s.size, np.uint32)
    _, lab, _, st = solver.solve_amplicons(s, e, ids, LENGTHS, 3, offs, a0, a1, single_end=True)
    assert lab.tolist() == [3, 2, 0, 6, 1, 1, 0, 1, 3, 0]
    assert st["units_in_several"] == 10 and st["amplicons_unused"] == 2
    check(solver, oracle, s, e, ids, LENGTHS, 3, offs, a0, a1, single_end=True)
    check(solver, oracle, s, e, ids, LENGTHS, 3, offs, a0, a1, single_end=True, per_amplicon=True)


@pytest.mark.parametrize("n_a", [2560, 2561])
def test_table_in_lds_and_in_global_memory(pkg, solver, oracle, n_a):
    """tiny amplicons of 8 bases (insert: the middle 4), step 6: at the LDS bound the table is staged, one amplicon more
    and it is read from global memory.  A second contig holds exactly one amplicon"""
    assert pkg.AMPLICON_LDS_MAX == 2560
    rng = np.random.default_rng(n_a)
    first = np.arange(n_a - 1, dtype=np.int64) * 6
    a0 = np.concatenate([first, [10]]).astype(np.uint32)
    a1 = np.concatenate([first + 7, [59]]).astype(np.uint32)
    i0, i1 = a0 + 2, a1 - 2
    lengths = np.array([int(first[-1]) + 8, 80])
    offs = np.array([0, n_a - 1, n_a], np.uint32)
    k = np.repeat(rng.integers(0, n_a, size=600), 2)                       # both mates from one amplicon
    k[:40] = n_a - 1
    s = a0.astype(np.int64)[k] + rng.integers(0, 4, size=k.size)
    e = np.minimum(s + rng.integers(0, 6, size=k.size), a1.astype(np.int64)[k] + (rng.random(k.size) < 0.1))
    ids = (k == n_a - 1).astype(np.uint32)
    e = np.maximum(np.minimum(e, lengths[ids] - 1), s)
    for per_amplicon in (False, True):
        _, st = check(solver, oracle, s.astype(np.uint32), e.astype(np.uint32), ids, lengths, 2, offs, a0, a1, i0, i1,
                      per_amplicon=per_amplicon, complete_pairs=True, what=f"{n_a} amplicons")
        assert st["amplicons"] == n_a and st["units_in_several"] > 0 and st["amplicons_unused"] > 0
        assert st["units_no_amplicon"] > 0 and st["reads_clipped_away"] > 0


@pytest.mark.parametrize("complete", [False, True])
def test_identity_1_inserts_null_pooled_is_filter_solve_by_contig(solver, complete):
    rng = np.random.default_rng(71)
    offs, a0, a1, _, _ = tiled_tables()
    s, e, ids = ap.panel_pairs(rng, LENGTHS, offs, a0, a1, 3000, read_length=150, straddle=0.1, cross=0.03, unplaced=0.02)
    sl = rng.integers(20, 200, size=s.size).astype(np.uint32)
    mq = rng.integers(0, 61, size=s.size).astype(np.uint32)
    kw = dict(seq_lengths=sl, qualities=mq, min_length=30, min_mapq=10, complete_pairs=complete)
    want, dropped = solver.filter_solve_by_contig(s, e, ids, LENGTHS, 7, offs, a0, a1, **kw)
    got, _, _, st = solver.solve_amplicons(s, e, ids, LENGTHS, 7, offs, a0, a1, **kw)
    assert np.array_equal(got, want) and want.any()
    assert st["units"] - st["units_assigned"] == dropped and st["bases_clipped"] == 0


def test_identity_2_disjoint_amplicons_both_modes_agree(solver, oracle):
    rng = np.random.default_rng(72)
    lengths = [3000, 1500]
    a0 = np.array([0, 401, 900, 1500, 100, 700], np.uint32)        # (an uncovered base between any two)
    a1 = np.array([399, 898, 1400, 2999, 600, 1499], np.uint32)
    offs = np.array([0, 4, 6], np.uint32)
    k = rng.integers(0, 6, size=2000)
    span = rng.integers(20, 150, size=(2000, 2))
    lo, hi = a0.astype(np.int64)[k][:, None], a1.astype(np.int64)[k][:, None]
    s = lo + (rng.random((2000, 2)) * (hi - lo + 2 - span)).astype(np.int64)
    e = s + span - 1
    ids = np.repeat((k >= 4).astype(np.uint32), 2)
    s, e = s.reshape(-1).astype(np.uint32), e.reshape(-1).astype(np.uint32)
    for complete in (False, True):
        pooled, lab, _, st = solver.solve_amplicons(s, e, ids, lengths, 5, offs, a0, a1, complete_pairs=complete)
        per, lab2, _, _ = solver.solve_amplicons(s, e, ids, lengths, 5, offs, a0, a1, complete_pairs=complete,
                                                 per_amplicon=True)
        assert st["units_assigned"] == 2000 and np.array_equal(lab, k) and np.array_equal(lab2, k)
        assert np.array_equal(pooled, per) and pooled.any()
    check(solver, oracle, s, e, ids, lengths, 5, offs, a0, a1, per_amplicon=True)


def test_one_amplicon_per_contig_single_end_is_solve_by_contig(solver):
    rng = np.random.default_rng(73)
    s, e, ids, lengths = mr.random_by_contig(rng, 5, max_reads_per_contig=800)
    offs = np.arange(6, dtype=np.uint32)
    a0, a1 = np.zeros(5, np.uint32), (lengths - 1).astype(np.uint32)
    want = solver.solve_by_contig(s, e, ids, lengths, 9)
    want = want[0] if isinstance(want, tuple) else want
    for per_amplicon in (False, True):
        got, lab, _, _ = solver.solve_amplicons(s, e, ids, lengths, 9, offs, a0, a1, single_end=True,
                                                per_amplicon=per_amplicon)
        assert np.array_equal(got, want) and np.array_equal(lab, ids)   # (NO_AMPLICON == NO_CONTIG for the unplaced)


def test_errors_leave_the_mask_untouched(pkg, solver, oracle):
    rng = np.random.default_rng(74)
    offs, a0, a1, i0, i1 = tiled_tables()
    s, e, ids = fragment_units(rng, 500, offs, a0, a1, True)
    n = s.size
    guard = np.uint64(0xA5A5A5A5A5A5A5A5)
    p32 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))

    def refused(code, word, s=s, e=e, ids=ids, n=n, offs=offs, a0=a0, a1=a1, i0=i0, i1=i1, flags=0, sl=None, min_length=0,
                n_contigs=len(LENGTHS)):
        mask = np.full((n + 63) // 64 + 1, guard, np.uint64)
        lab = np.full(n + 1, 7, np.uint32)
        rows = np.zeros(max(a0.size if a0 is not None else 1, 1), pkg.DEPTH_ROW_DTYPE)
        keep = [np.ascontiguousarray(x, np.uint32) for x in (s, e, ids, LENGTHS)]
        with pytest.raises(pkg.QmcpError, match=word) as ei:
            pkg._check(pkg._hip.qmcp_hip_solve_amplicons_host(
                solver._ctx, p32(keep[0]), p32(keep[1]), p32(keep[2]), p32(sl), None, n, p32(keep[3]), n_contigs, p32(offs),
                p32(a0), p32(a1), p32(i0), p32(i1), min_length, 0, 4, flags, mask.ctypes.data_as(C.POINTER(C.c_uint64)),
                p32(lab), C.c_void_p(rows.ctypes.data), None, None))
        assert ei.value.code == code
        assert (mask == guard).all() and (lab == 7).all() and not rows.view(np.uint8).any()

    bad = i0.copy()
    bad[3] = a0[3] - 1
    refused(pkg.QMCP_EINVAL, "amplicon 3", i0=bad)
    bad = i1.copy()
    bad[5] = i0[5] - 1
    refused(pkg.QMCP_EINVAL, "amplicon 5", i1=bad)
    bad = i1.copy()
    bad[0] = a1[0] + 1
    refused(pkg.QMCP_EINVAL, "amplicon 0", i1=bad)
    refused(pkg.QMCP_EINVAL, "go together", i1=None)
    refused(pkg.QMCP_EINVAL, "amp_offsets missing", offs=None)
    refused(pkg.QMCP_EINVAL, "must be even", n=n - 1)
    refused(pkg.QMCP_EINVAL, "needs pairs", flags=pkg.AMPLICONS_SINGLE_END | pkg.AMPLICONS_COMPLETE_PAIRS)
    refused(pkg.QMCP_EINVAL, "unknown flag", flags=8)
    many = np.array([0, 0, 0, 0, (1 << 24) + 1], np.uint32)            # offsets only: nothing else is looked at
    refused(pkg.QMCP_ERANGE, "2\\^24", offs=many, a0=None, a1=None, i0=None, i1=None, flags=pkg.AMPLICONS_PER_AMPLICON)
    ids2 = ids.copy()
    ids2[11] = 4
    refused(pkg.QMCP_EINVAL, "contig id", ids=ids2)
    # a bad read inside a unit the length filter drops
    q = int(np.flatnonzero(ids[0::2] == 0)[0])
    sl = np.full(n, 100, np.uint32)
    sl[2 * q] = 10
    e2 = e.copy()
    e2[2 * q + 1] = LENGTHS[0]
    refused(pkg.QMCP_EREAD, "a read has", e=e2, sl=sl, min_length=30)
    s2 = s.copy()
    s2[2 * q] = e[2 * q] + 1
    refused(pkg.QMCP_EREAD, "a read has", s=s2, sl=sl, min_length=30)
    check(solver, oracle, s, e, ids, LENGTHS, 4, offs, a0, a1, i0, i1, what="after the refusals")


def test_a_pending_solve_refuses_the_entry(pkg, solver, oracle):
    torch = pytest.importorskip("torch")
    s, e = pkg.reads_gen(pkg.KIND_UNIFORM, 20_000, 6_000, seed=7)
    d_s = torch.from_numpy(s.view(np.int32)).cuda()
    d_e = torch.from_numpy(e.view(np.int32)).cuda()
    d_mask = torch.zeros(pkg.mask_words(s.size), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    solver.solve_device_begin(d_s.data_ptr(), d_e.data_ptr(), s.size, 6_000, 10, d_mask.data_ptr())
    try:
        with pytest.raises(pkg.QmcpError, match="pending"):
            solver.solve_amplicons(s, e, np.zeros(s.size, np.uint32), [6_000], 10, [0, 1], [0], [5_999])
    finally:
        solver.solve_end()
    assert np.array_equal(d_mask.cpu().numpy().view(np.uint64), oracle.solve(s, e, 6_000, 10))


def test_device_entry_equals_the_host_entry_and_refuses_odd_alignment(pkg, solver, oracle):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(75)
    offs, a0, a1, i0, i1 = tiled_tables()
    guard = -0x5A5A5A5A5A5A5A5B
    for pairs in (True, False):
        s, e, ids = fragment_units(rng, 1000, offs, a0, a1, pairs)
        n = s.size
        words = (n + 63) // 64
        sl = rng.integers(20, 200, size=n).astype(np.uint32)
        mq = rng.integers(0, 61, size=n).astype(np.uint32)
        kw = dict(min_length=30, min_mapq=5, single_end=not pairs, per_amplicon=pairs, complete_pairs=pairs)
        keep_w, lab_w, rows_w, st_w = am.solve(oracle, s, e, ids, LENGTHS, 4, offs, a0, a1, i0, i1, seq_lengths=sl,
                                               qualities=mq, **kw)
        for shift in (0, 1):
            cols = []
            for x in (s, e, ids, sl, mq):
                t = torch.zeros(n + shift + 4, dtype=torch.int32, device=dev)   # (a base allocation is 256-byte aligned)
                t[shift:shift + n] = torch.from_numpy(x.view(np.int32)).to(dev)
                cols.append(t)
            d_mask = torch.full((words + 3,), guard, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            ptr = [t.data_ptr() + 4 * shift for t in cols]
            call = lambda: solver.solve_amplicons_device(ptr[0], ptr[1], ptr[2], n, LENGTHS, 4, d_mask.data_ptr(), offs, a0,
                                                         a1, insert_starts=i0, insert_ends=i1, d_seq_lengths=ptr[3],
                                                         d_qualities=ptr[4],
                                                         stream=torch.cuda.current_stream().cuda_stream, **kw)
            if pairs and shift:
                # the kernel reads a pair as one 8-byte word: such columns are refused, nothing is written
                with pytest.raises(pkg.QmcpError, match="8-byte aligned") as ei:
                    call()
                assert ei.value.code == pkg.QMCP_EINVAL and (d_mask.cpu().numpy() == guard).all()
                continue
            lab, rows, st = call()
            got = d_mask.cpu().numpy()
            assert np.array_equal(got[:words].view(np.uint64), am.pack(keep_w)), (pairs, shift)
            assert (got[words:] == guard).all()
            assert np.array_equal(lab, lab_w) and {k: st[k] for k in am.STAT_KEYS} == st_w
            assert [tuple(int(x) for x in r) for r in rows.tolist()] == rows_w
