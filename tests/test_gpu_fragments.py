"""Fragment depth on the device: qmcp_hip_clip_templates_* against tests/fragment_model.py's clip (both output columns and
every statistic, exactly), qmcp_hip_solve_fragments_* against template_model.staged on the model's clipped columns, the
two identities, the contrast input, the errors the device finds, and the file flow.
TILE: the segmented scan works on tiles of 1 024 sorted rows (four waves of 4 x 64), carried tile to tile by a spine."""
import ctypes as C

import numpy as np
import pytest
import torch

import bam_py
import fragment_model as fm
import profile_model as pm
import template_bams as tb
import template_model as tm
import template_profile_model as tpm

pytestmark = pytest.mark.gpu

NO_CONTIG = 0xFFFFFFFF
QMCP_EINVAL, QMCP_EREAD = -1, -2
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
TILE = 1024
SENTINEL = 0xDEADBEEF
SORT_SCAN_WORDS = ("k_frag_keys", "radix", "k_frag_tiles", "k_frag_spine", "k_frag_apply")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")


def clip_device(solver, s, e, ids, tids, n_templates, lengths):
    """the device entry on outputs prefilled with a sentinel, one guard word behind each"""
    n = s.size
    cols = [_dev(x) for x in (s, e, ids, tids)]
    outs = [torch.full((n + 1,), -2, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    fs = solver.clip_templates_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), n,
                                      n_templates, lengths, outs[0].data_ptr(), outs[1].data_ptr(),
                                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = [o.cpu().numpy().view(np.uint32) for o in outs]
    assert got[0][n] == got[1][n] == 0xFFFFFFFE                         # nothing written past the columns
    for col, src in zip(cols, (s, e, ids, tids)):                      # the inputs are not modified
        assert np.array_equal(col.cpu().numpy().view(np.uint32), np.asarray(src, np.uint32))
    return got[0][:n].copy(), got[1][:n].copy(), fs


def check_clip(solver, s, e, ids, tids, n_templates, lengths):
    """host and device entry against the model: both columns and every statistic -> the model's stats"""
    want_s, want_c, want = fm.clip(s, e, ids, tids)
    for entry in ("host", "device"):
        if entry == "host":
            got_s, got_c, fs = solver.clip_templates(s, e, ids, tids, n_templates, lengths)
        else:
            got_s, got_c, fs = clip_device(solver, s, e, ids, tids, n_templates, lengths)
        assert np.array_equal(got_s, want_s), (entry, int(np.count_nonzero(got_s != want_s)))
        assert np.array_equal(got_c, want_c), (entry, int(np.count_nonzero(got_c != want_c)))
        got = {k: int(getattr(fs, k)) for k in fm.STAT_NAMES}
        assert got == want, entry
    return want


# ------------------------------------------------------------------------------------------ 1: random calls
def test_random_calls_equal_the_model(solver):
    clipped = emptied = 0
    for seed in range(60):
        rng = np.random.default_rng(1000 + seed)
        lengths = rng.integers(200, 3001, size=int(rng.integers(1, 4))).astype(np.uint32)
        n = int(rng.integers(0, 2001))
        large = (0, 70, 300, 1500)[seed % 4]
        spare = None if seed % 3 else n + 40
        s, e, ids, tids, n_templates = fm.random_fragments(rng, n, lengths, n_templates=spare, large=large)
        want = check_clip(solver, s, e, ids, tids, n_templates, lengths)
        clipped += want["n_clipped"]
        emptied += want["n_emptied"]
    assert clipped > 2000 and emptied > 2000


# ------------------------------------------------------------------------------------------ 2: carry shapes
CARRY_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 5 * TILE]


def carry_pattern(kind, n, L):
    i = np.arange(n, dtype=np.int64)
    if kind == "span_first":            # the first segment spans the contig: every later one is emptied by the carry
        s, e = 10 + 2 * i, 14 + 2 * i
        s[0], e[0] = 0, L - 1
    elif kind == "staircase":           # start = 2 i, length 5: every segment but the first loses 3 bases
        s, e = 2 * i, 2 * i + 4
    elif kind == "disjoint":            # the identity
        s, e = 3 * i, 3 * i + 1
    else:                               # all identical: the first stays, every other one is emptied
        s, e = np.full(n, 7, np.int64), np.full(n, 30, np.int64)
    return s.astype(np.uint32), e.astype(np.uint32)


@pytest.mark.parametrize("n", CARRY_SIZES)
def test_one_template_on_one_contig_carries_across_waves_and_tiles(solver, n):
    L = 20_000
    lengths = np.array([L], np.uint32)
    ids, tids = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for kind in ("span_first", "staircase", "disjoint", "identical"):
        s, e = carry_pattern(kind, n, L)
        want = check_clip(solver, s, e, ids, tids, 1, lengths)
        assert want["max_group"] == n
        if kind == "span_first":
            assert want["n_emptied"] == n - 1 and want["n_clipped"] == 0
        elif kind == "staircase":
            assert want["n_clipped"] == n - 1 and want["bases_removed"] == 3 * (n - 1)
        elif kind == "disjoint":
            assert want["n_clipped"] == want["n_emptied"] == want["n_templates_overlapping"] == 0
        else:
            assert want["n_emptied"] == n - 1
        # the same rows in a shuffled input order: the sort brings them back, ties go by input index
        perm = np.random.default_rng(n).permutation(n)
        check_clip(solver, s[perm], e[perm], ids, tids, 1, lengths)


# ------------------------------------------------------------------------------------------ 3: heads on boundaries
@pytest.mark.parametrize("size, count", [(TILE, 3), (64, 40)])
def test_groups_whose_heads_fall_on_tile_and_wave_boundaries(solver, size, count):
    rng = np.random.default_rng(size)
    n = size * count
    lengths = np.array([200 * count + 400], np.uint32)
    tids = np.repeat(np.arange(count), size)
    s = 200 * tids + rng.integers(0, 60, n)
    e = s + rng.integers(0, 70, n)
    # the last member of every group reaches furthest: a carry that leaked into the next group would clip its head
    last = np.arange(size - 1, n, size)
    e[last] = 200 * tids[last] + 390
    perm = rng.permutation(n)
    s, e, tids = s[perm].astype(np.uint32), e[perm].astype(np.uint32), tids[perm].astype(np.uint32)
    want = check_clip(solver, s, e, np.zeros(n, np.uint32), tids, count, lengths)
    assert want["max_group"] == size and want["n_templates_overlapping"] == count


# ------------------------------------------------------------------------------------------ 4: the common shape
def test_two_to_the_sixteen_pairs_half_of_them_overlapping(solver):
    rng = np.random.default_rng(4)
    P = 1 << 16
    lengths = np.array([100_000, 100_000], np.uint32)
    fs = rng.integers(0, 100_000 - 400, P)
    fl = rng.integers(160, 401, P)
    s, e = np.empty(2 * P, np.int64), np.empty(2 * P, np.int64)
    s[0::2], e[0::2] = fs, fs + 149
    s[1::2], e[1::2] = fs + fl - 150, fs + fl - 1
    ids = np.repeat(rng.integers(0, 2, P), 2).astype(np.uint32)
    tids = (np.arange(2 * P) // 2).astype(np.uint32)
    want = check_clip(solver, s.astype(np.uint32), e.astype(np.uint32), ids, tids, P, lengths)
    assert 0.4 * P < want["n_clipped"] < 0.7 * P and want["max_group"] == 2
    assert want["n_templates_overlapping"] == want["n_clipped"] + want["n_emptied"]


# ------------------------------------------------------------------------------------------ 5: the early exit
def test_a_call_without_a_template_of_two_segments_launches_no_sort_or_scan(solver):
    rng = np.random.default_rng(5)
    lengths = np.array([3000, 2000], np.uint32)
    n = 5000
    s, e, ids, _, _ = fm.random_fragments(rng, n, lengths)
    tids = rng.permutation(n + 7)[:n].astype(np.uint32)                 # distinct ids, some unused
    solver.set_profiling(True)
    try:
        got_s, got_c, fs = solver.clip_templates(s, e, ids, tids, n + 7, lengths)
        single = solver.kernel_times()
        assert np.array_equal(got_s, s) and np.array_equal(got_c, ids)
        assert fs.n_clipped == fs.n_emptied == fs.bases_removed == 0 and fs.max_group == 1
        assert fs.n_placed == int((ids != NO_CONTIG).sum())
        assert "k_frag_check" in single
        assert not [k for k in single if any(w in k for w in SORT_SCAN_WORDS)], single
        solver.set_profiling(True)                                       # (resets the totals)
        tids[1] = tids[0]                                                # one template of two: the sort and the scan run
        check_clip(solver, s, e, ids, tids, n + 7, lengths)
        both = solver.kernel_times()
        for word in SORT_SCAN_WORDS:
            assert [k for k in both if word in k], (word, both)
    finally:
        solver.set_profiling(False)


# ------------------------------------------------------------------------------------------ 6: edges
def test_no_rows_only_unplaced_rows_and_the_highest_id(solver):
    lengths = np.array([500], np.uint32)
    z = np.zeros(0, np.uint32)
    got_s, got_c, fs = solver.clip_templates(z, z, z, z, 0, lengths)
    assert got_s.size == got_c.size == 0 and fs.n_placed == fs.max_group == 0
    assert clip_device(solver, z, z, z, z, 0, lengths)[2].n_placed == 0
    n = 300
    rng = np.random.default_rng(6)
    s = rng.integers(0, 100, n).astype(np.uint32)
    e = s + 5
    ids = np.full(n, NO_CONTIG, np.uint32)
    tids = rng.integers(0, 20, n).astype(np.uint32)
    want = check_clip(solver, s, e, ids, tids, 20, lengths)
    assert want["n_placed"] == want["max_group"] == 0
    # the highest id in use is n_templates - 1, its two overlapping segments at the two ends of the input; four bytes
    # of template id, one of contig id and four of start make the sort take two rounds of keys
    n_templates = 2**24 + 5
    lengths2 = np.array([2**24 + 400, 400], np.uint32)
    ids = rng.integers(0, 2, n).astype(np.uint32)
    tids = rng.integers(0, n_templates, n).astype(np.uint32)
    tids[:40] = tids[40:80]                                              # some templates of two
    s = (rng.integers(0, 300, n) + np.where(ids == 0, 2**24 * (tids % 2), 0)).astype(np.uint32)
    e = (s + rng.integers(0, 90, n)).astype(np.uint32)
    tids[0] = tids[n - 1] = n_templates - 1
    ids[0] = ids[n - 1] = 0
    s[0], e[0], s[n - 1], e[n - 1] = 2**24 + 10, 2**24 + 40, 2**24 + 30, 2**24 + 60
    want = check_clip(solver, s, e, ids, tids, n_templates, lengths2)
    assert want["n_clipped"] >= 1
    # ends up to the last position of the longest contig a call can have are carried as they are
    big = np.array([2**31 - 2], np.uint32)
    s = np.array([5, 2**31 - 10, 2**31 - 6], np.uint32)
    e = np.array([2**31 - 3, 2**31 - 3, 2**31 - 4], np.uint32)
    want = check_clip(solver, s, e, np.zeros(3, np.uint32), np.zeros(3, np.uint32), 1, big)
    assert want["n_emptied"] == 2


# ------------------------------------------------------------------------------------------ 7: the solve
def solve_device(pkg, solver, s, e, ids, tids, n_templates, lengths, M, stages):
    n = s.size
    words = pkg.mask_words(n)
    cols = [_dev(x) for x in (s, e, ids, tids)]
    d_mask = torch.full((words + 1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st, ts, fs = solver.solve_fragments_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(),
                                               cols[3].data_ptr(), n, n_templates, lengths, M, d_mask.data_ptr(), stages,
                                               stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_mask.cpu().numpy().view(np.uint64)
    assert out[words] == ALL_ONES
    for col, src in zip(cols, (s, e, ids, tids)):                      # the caller's columns are never modified
        assert np.array_equal(col.cpu().numpy().view(np.uint32), np.asarray(src, np.uint32))
    return out[:words].copy(), st, ts, fs


def fragment_floor_holds(s, e, ids, tids, lengths, kept, M):
    have = fm.fragment_depth(s, e, ids, tids, lengths, kept)
    full = fm.fragment_depth(s, e, ids, tids, lengths)
    return all((h >= np.minimum(f, M)).all() for h, f in zip(have, full))


@pytest.fixture(scope="module")
def solve_instance():
    rng = np.random.default_rng(70)
    lengths = np.array([900, 600], np.uint32)
    s, e, ids, tids, n_templates = fm.random_fragments(rng, 3000, lengths, large=300)
    return s, e, ids, tids, n_templates, lengths


@pytest.mark.parametrize("M", [1, 2, 3, 7, 20])
def test_solve_fragments_equals_the_staged_model_on_clipped_columns(pkg, solver, solve_instance, M):
    s, e, ids, tids, n_templates, lengths = solve_instance
    n = s.size
    _, _, clip_stats = fm.clip(s, e, ids, tids)
    for stages in (None, [M], [1, M]):
        if stages == [1, M] and M == 1:
            continue
        want, selected, kept, sets = fm.staged(s, e, ids, tids, n_templates, lengths, M, stages)
        k = len(selected)
        host = solver.solve_fragments(s, e, ids, tids, n_templates, lengths, M, stages)
        dev = solve_device(pkg, solver, s, e, ids, tids, n_templates, lengths, M, stages)
        for got, st, ts, fs in (host, dev):
            assert np.array_equal(got, want), (M, stages)
            assert ts.n_stages == k and list(ts.n_selected)[:k] == selected and list(ts.n_kept)[:k] == kept
            assert {f: int(getattr(fs, f)) for f in fm.STAT_NAMES} == clip_stats
        assert tm.whole_templates(sets[-1], tids, n_templates)
        assert fragment_floor_holds(s, e, ids, tids, lengths, sets[-1], M)


# ------------------------------------------------------------------------------------------ 8: identities
def test_rows_without_overlap_inside_a_template_give_solve_templates(pkg, solver):
    rng = np.random.default_rng(8)
    lengths = np.array([4000, 2500], np.uint32)
    s, e, ids, tids, n_templates = fm.random_fragments(rng, 4000, lengths, large=70)
    s, ids, _ = fm.clip(s, e, ids, tids)                                # disjoint inside every template now
    assert fm.clip(s, e, ids, tids)[2]["bases_removed"] == 0
    for M, stages in ((3, None), (7, [2, 4, 7])):
        want, st_t, ts_t = solver.solve_templates(s, e, ids, tids, n_templates, lengths, M, stages)
        want = want.copy()
        got, st_f, ts_f, fs = solver.solve_fragments(s, e, ids, tids, n_templates, lengths, M, stages)
        assert np.array_equal(got, want) and fs.n_clipped == fs.n_emptied == 0
        for name, _ in pkg.TemplateStats._fields_:
            if name in ("ms_stage", "ms_templates"):
                continue
            a, b = getattr(ts_f, name), getattr(ts_t, name)
            assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), name
        assert st_f.n_kept == st_t.n_kept


def test_distinct_ids_and_one_stage_give_solve_by_contig(pkg, solver):
    rng = np.random.default_rng(9)
    lengths = np.array([3000, 2000, 700], np.uint32)
    n = 5000
    s, e, ids, _, _ = fm.random_fragments(rng, n, lengths)
    tids = rng.permutation(n).astype(np.uint32)
    for M in (1, 4, 11):
        want = solver.solve_by_contig(s, e, ids, lengths, M).copy()
        got, _, _, _ = solver.solve_fragments(s, e, ids, tids, n, lengths, M, [M])
        got_d, _, _, _ = solve_device(pkg, solver, s, e, ids, tids, n, lengths, M, [M])
        assert np.array_equal(got, want) and np.array_equal(got_d, want)


# ------------------------------------------------------------------------------------------ 9: the contrast input
def test_contrast_input_solve_templates_is_short_solve_fragments_is_not(pkg, solver):
    s, e, ids, tids, n_templates, lengths, M = fm.contrast_pairs()
    n = s.size
    full = fm.fragment_depth(s, e, ids, tids, lengths)[0]
    per_segment = pm.unpack(solver.solve_templates(s, e, ids, tids, n_templates, lengths, M)[0], n)
    short = int((fm.fragment_depth(s, e, ids, tids, lengths, per_segment)[0] < np.minimum(full, M)).sum())
    got, _, ts, fs = solver.solve_fragments(s, e, ids, tids, n_templates, lengths, M)
    fragments = pm.unpack(got, n)
    short_f = int((fm.fragment_depth(s, e, ids, tids, lengths, fragments)[0] < np.minimum(full, M)).sum())
    print(f"positions short of min(fragment depth, {M}): solve_templates {short}, solve_fragments {short_f}; "
          f"segments kept {int(per_segment.sum())} / {int(fragments.sum())}")
    assert short > 0 and short_f == 0
    assert np.array_equal(got, fm.staged(s, e, ids, tids, n_templates, lengths, M)[0])
    assert fs.n_clipped > 0 and tm.whole_templates(fragments, tids, n_templates)


# ------------------------------------------------------------------------------------------ 10: device-found errors
def test_errors_found_on_the_device_leave_the_outputs_and_clear_the_mask(pkg, solver):
    """argument errors the library must refuse; the bad row sits inside an overlapping group, where a clip that ran first
    would have emptied it"""
    n = 2 * TILE + 5
    lengths = np.array([5000, 100], np.uint32)
    s = np.full(n, 100, np.uint32)
    e = np.full(n, 400, np.uint32)                                        # one group, all identical: all but one emptied
    ids, tids = np.zeros(n, np.uint32), np.full(n, 3, np.uint32)
    cases = []
    bad = tids.copy(); bad[n - 2] = 4
    cases.append((s, e, ids, bad, QMCP_EINVAL, "template id"))
    bad = ids.copy(); bad[TILE + 1] = 2
    cases.append((s, e, bad, tids, QMCP_EINVAL, "contig id"))
    bs, be = s.copy(), e.copy(); bs[n - 1], be[n - 1] = 300, 200           # start > end, inside [100, 400]
    cases.append((bs, be, ids, tids, QMCP_EREAD, "start > end"))
    be = e.copy(); be[7] = 5000                                           # end >= the contig's length
    cases.append((s, be, ids, tids, QMCP_EREAD, "start > end"))
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    for cs, ce, ci, ct, code, word in cases:
        cs, ce, ci, ct = (np.ascontiguousarray(x, np.uint32) for x in (cs, ce, ci, ct))
        # clip, host entry: the outputs keep their sentinel
        out_s, out_c = np.full(n, SENTINEL, np.uint32), np.full(n, SENTINEL, np.uint32)
        rc = pkg._hip.qmcp_hip_clip_templates_host(solver._ctx, u32(cs), u32(ce), u32(ci), u32(ct), n, 4, u32(lengths), 2,
                                                   u32(out_s), u32(out_c), None)
        msg = pkg._hip.qmcp_hip_last_error().decode()
        assert rc == code and word in msg, (rc, msg)
        assert (out_s == SENTINEL).all() and (out_c == SENTINEL).all()
        # clip, device entry
        cols = [_dev(x) for x in (cs, ce, ci, ct)]
        outs = [torch.full((n,), -2, dtype=torch.int32, device="cuda:0") for _ in range(2)]
        d_mask = torch.full((pkg.mask_words(n) + 1,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(pkg.QmcpError) as err:
            solver.clip_templates_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), n,
                                         4, lengths, outs[0].data_ptr(), outs[1].data_ptr())
        assert err.value.code == code and word in str(err.value)
        torch.cuda.synchronize()
        assert all((o.cpu().numpy() == -2).all() for o in outs)
        # the solve: the same code and message, the device mask cleared, the host mask not written
        with pytest.raises(pkg.QmcpError) as err:
            solver.solve_fragments_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(),
                                          n, 4, lengths, 3, d_mask.data_ptr())
        assert err.value.code == code and word in str(err.value)
        torch.cuda.synchronize()
        out = d_mask.cpu().numpy()
        assert (out[:-1] == 0).all() and out[-1] == -1
        with pytest.raises(pkg.QmcpError) as err:
            solver.solve_fragments(cs, ce, ci, ct, 4, lengths, 3)
        assert err.value.code == code and word in str(err.value)
    # the context is still good
    check_clip(solver, s, e, ids, tids, 4, lengths)


def test_clip_outputs_must_not_overlap_the_inputs(pkg, solver):
    n = 100
    cols = [_dev(np.arange(n) % 7) for _ in range(4)]
    out = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(pkg.QmcpError) as err:
        solver.clip_templates_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), n, 7,
                                     [50], cols[0].data_ptr(), out.data_ptr())
    assert err.value.code == QMCP_EINVAL and "overlaps" in str(err.value)


# ------------------------------------------------------------------------------------------ 11: behind a user stream
def test_device_entries_are_ordered_after_a_stream_that_still_writes_the_columns(pkg, solver):
    rng = np.random.default_rng(11)
    lengths = np.array([2500, 1500], np.uint32)
    n = 6000
    s, e, ids, tids, n_templates = fm.random_fragments(rng, n, lengths, large=300)
    want_s, want_c, _ = fm.clip(s, e, ids, tids)
    want_mask = fm.staged(s, e, ids, tids, n_templates, lengths, 4)[0]
    dev = "cuda:0"
    side = torch.cuda.Stream(device=dev)
    src = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids, tids)]
    cols = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4)]
    outs = [torch.full((n,), -2, dtype=torch.int32, device=dev) for _ in range(2)]
    d_mask = torch.full((pkg.mask_words(n),), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):                                              # (the columns are still being written)
            for k in range(4):
                cols[k].copy_(src[(k + 1) % 4])
        for k in range(4):
            cols[k].copy_(src[k])
        solver.clip_templates_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), n,
                                     n_templates, lengths, outs[0].data_ptr(), outs[1].data_ptr(), stream=side.cuda_stream)
        solver.solve_fragments_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), n,
                                      n_templates, lengths, 4, d_mask.data_ptr(), stream=side.cuda_stream)
    assert np.array_equal(outs[0].cpu().numpy().view(np.uint32), want_s)
    assert np.array_equal(outs[1].cpu().numpy().view(np.uint32), want_c)
    assert np.array_equal(d_mask.cpu().numpy().view(np.uint64), want_mask)


# ------------------------------------------------------------------------------------------ 12: under a cap table
def test_solve_templates_profile_with_fragment_depth_runs_on_the_clipped_columns(pkg, solver):
    rng = np.random.default_rng(12)
    lengths = np.array([1500, 900], np.uint32)
    n, M, default_cap = 3000, 6, 2
    s, e, ids, tids, n_templates = fm.random_fragments(rng, n, lengths, large=70)
    offs = np.array([0, 2, 3], np.uint32)
    r0, r1 = np.array([100, 700, 50], np.uint32), np.array([400, 1200, 600], np.uint32)
    caps = np.array([6, 3, 0], np.uint32)
    cs, cc, clip_stats = fm.clip(s, e, ids, tids)
    want = tpm.staged(cs, e, cc, tids, n_templates, lengths, M, default_cap, offs, r0, r1, caps)[0]
    got, _, _, _ = solver.solve_templates_profile(s, e, ids, tids, n_templates, lengths, M, default_cap, offs, r0, r1, caps,
                                                  fragment_depth=True)
    assert np.array_equal(got, want)
    assert {f: int(getattr(solver.last_fragment_stats, f)) for f in fm.STAT_NAMES} == clip_stats
    # the device form, with the two columns it clips into
    cols = [_dev(x) for x in (s, e, ids, tids)]
    outs = [torch.zeros(n, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    d_mask = torch.full((pkg.mask_words(n),), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    solver.solve_templates_profile_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), n,
                                          n_templates, lengths, M, default_cap, d_mask.data_ptr(), offs, r0, r1, caps,
                                          fragment_depth=True, d_clipped_starts=outs[0].data_ptr(),
                                          d_clipped_contig_ids=outs[1].data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_mask.cpu().numpy().view(np.uint64), want)


# ------------------------------------------------------------------------------------------ 13: the file flow
def overlapping_pair_records(rng, refs, n_pairs):
    """2 x 150 pairs with fragment lengths 160 .. 400 on their reference: roughly half of them overlap"""
    out = []
    for i in range(n_pairs):
        ref = int(rng.integers(0, len(refs)))
        fl = int(rng.integers(160, 401))
        pos = int(rng.integers(0, refs[ref][1] - fl))
        mapq = int(rng.integers(0, 61))
        out.append(tb.record(f"p{i}", 0x41, ref, pos, mapq, [(150, "M")]))
        out.append(tb.record(f"p{i}", 0x81, ref, pos + fl - 150, mapq, [(150, "M")]))
    return [out[i] for i in rng.permutation(len(out))]


def check_fragment_file_flow(pkg, tmp_path, name, refs, records, M, stages=None, table=None):
    """a record is written iff its template is kept by the model on the independently parsed segments; the report's
    values are the model's"""
    path = tmp_path / f"{name}.bam"
    bam_py.write_bam(path, refs, records)
    header, parsed, _ = bam_py.parse(path)
    segs = tb.expected_segments(records)
    lengths = np.array([L for _, L in refs], np.uint32)
    s, e, ids, tids, nt = segs["starts"], segs["ends"], segs["contig_ids"], segs["template_ids"], segs["n_templates"]
    cs, cc, clip_stats = fm.clip(s, e, ids, tids)
    kw = {}
    if table is None:
        _, _, _, sets = tm.staged(cs, e, cc, tids, nt, lengths, M, stages)
    else:
        graph = tmp_path / f"{name}.bedgraph"
        graph.write_text("".join(f"{refs[c][0]}\t{a}\t{b + 1}\t{cap}\n" for c, a, b, cap in table))
        offs = np.cumsum([0] + [sum(1 for row in table if row[0] == c) for c in range(len(refs))]).astype(np.uint32)
        r0, r1, caps = (np.array([row[k] for row in table], np.uint32) for k in (1, 2, 3))
        _, _, _, sets = tpm.staged(cs, e, cc, tids, nt, lengths, M, M, offs, r0, r1, caps, stages)
        kw["template_profile"] = graph
    kept_records = np.unique(np.asarray(segs["segment_records"], np.int64)[sets[-1]])
    out, report = tmp_path / f"{name}.out.bam", tmp_path / f"{name}.fragments.tsv"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, template_aware=True,
                                 template_stages=stages, fragment_depth=True, fragment_report=report, **kw)
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == kept_records.size == len(orecs) > 0
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_records.tolist()]
    rows = dict(line.split("\t", 1) for line in report.read_text().splitlines() if "\t" in line and line[0] != "#")
    names = {"n_placed": "segments_placed", "n_clipped": "segments_clipped", "n_emptied": "segments_emptied",
             "bases_in": "bases_in", "bases_removed": "bases_removed", "n_templates_overlapping": "templates_overlapping",
             "max_group": "max_group"}
    assert {k: int(rows[v]) for k, v in names.items()} == clip_stats
    assert int(rows["records_written"]) == written and float(rows["ms_clip"]) >= 0
    if table is None:
        assert fragment_floor_holds(s, e, ids, tids, lengths, sets[-1], M)
    return clip_stats, written


def test_downsample_bam_with_fragment_depth_writes_the_models_templates(pkg, solver, tmp_path):
    refs = [("chrA", 3000), ("chrB", 1800)]
    pairs = overlapping_pair_records(np.random.default_rng(13), refs, 900)
    stats, written = check_fragment_file_flow(pkg, tmp_path, "pairs", refs, pairs, 8)
    assert stats["n_clipped"] > 300 and stats["max_group"] == 2
    per_segment = pkg.downsample_bam("quasi-mcp-hip", tmp_path / "pairs.bam", tmp_path / "per_segment.bam", 8,
                                     per_reference=True, template_aware=True)
    assert written > per_segment                                         # more molecules are needed for 8 x of fragments
    check_fragment_file_flow(pkg, tmp_path, "pairs3", refs, pairs, 8, stages=[2, 5, 8])
    table = [(0, 100, 900, 3), (0, 1500, 2200, 8), (1, 0, 700, 0)]
    check_fragment_file_flow(pkg, tmp_path, "pairs_caps", refs, pairs, 8, table=table)
    refs3 = [("chrA", 5000), ("chrB", 3000), ("chrC", 800)]
    mixed = tb.mixed_records(np.random.default_rng(11), refs3, 700)
    check_fragment_file_flow(pkg, tmp_path, "mixed", refs3, mixed, 6)
