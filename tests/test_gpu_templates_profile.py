"""qmcp_hip_solve_templates_profile_*: whole templates under a cap per region.  Every mask and every per-stage count is
compared bit for bit with tests/template_profile_model.py through both the host and the device entry, on an output
pre-filled with ones; the four identities with qmcp_hip_solve_templates_* and qmcp_hip_solve_profile_*; the on-cap counts
with the model; the file flow with the records of the model's kept templates."""
import ctypes as C
import functools
import json
import os
import statistics
import time

import numpy as np
import pytest
import torch

import bam_py
import profile_model as pm
import template_bams as tb
import template_model as tm
import template_profile_model as tpm

pytestmark = pytest.mark.gpu

NO_CONTIG = 0xFFFFFFFF
QMCP_EINVAL, QMCP_ERANGE = -1, -3
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
STAGE_FIELDS = ("target", "n_selected", "n_kept", "capped_positions", "demand", "sweeps")
# the whole call under caps that are all M against qmcp_hip_solve_templates_device on the same input: the
# ratio measured on one MI355X (1.0085), the run-to-run spread of that run (2.1 % + 0.9 %), and 3 % for what
# DESIGN 6 records between boxes
COST_MARGIN = 1.07


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")


def u32(a):
    return None if a is None else np.ascontiguousarray(a, np.uint32)


def solve_device(pkg, solver, inst, M, default_cap, table, stages):
    """the device entry on a mask buffer filled with ones, one guard word behind it"""
    s, e, ids, tids, n_templates, lengths = inst
    n = s.size
    words = pkg.mask_words(n)
    cols = [_dev(x) for x in (s, e, ids, tids)]
    d_mask = torch.full((words + 1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st, ts, qs = solver.solve_templates_profile_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(),
                                                       cols[3].data_ptr(), n, n_templates, lengths, M, default_cap,
                                                       d_mask.data_ptr(), *table, stages=stages,
                                                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_mask.cpu().numpy().view(np.uint64)
    assert out[words] == ALL_ONES                                        # nothing written past the mask
    if n % 64:
        assert int(out[words - 1]) >> (n % 64) == 0                      # no bit at or beyond n_reads
    return out[:words].copy(), st, ts, qs


def solve_host_prefilled(pkg, solver, inst, M, default_cap, table, stages):
    """the host entry through the C ABI, keep_mask_out filled with 0xFF"""
    s, e, ids, tids, n_templates, lengths = inst
    n = s.size
    words = pkg.mask_words(n)
    cols = [u32(x) for x in (s, e, ids, tids, lengths)]
    tab = [u32(x) for x in table]
    tg = None if stages is None else np.asarray(stages, np.uint32)
    out = np.full(words + 1, ALL_ONES, np.uint64)
    st, ts, qs = pkg.Stats(), pkg.TemplateStats(), pkg.TemplateProfileStats()
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    rc = pkg._hip.qmcp_hip_solve_templates_profile_host(
        solver._ctx, p(cols[0]), p(cols[1]), p(cols[2]), p(cols[3]), n, n_templates, p(cols[4]), cols[4].size, p(tab[0]),
        p(tab[1]), p(tab[2]), p(tab[3]), default_cap, 0, M, p(tg), 0 if tg is None else tg.size,
        out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(st), C.byref(ts), C.byref(qs))
    assert rc == 0, pkg._hip.qmcp_hip_last_error()
    assert out[words] == ALL_ONES
    if n % 64:
        assert int(out[words - 1]) >> (n % 64) == 0
    return out[:words].copy(), st, ts, qs


NO_TABLE = (None, None, None, None)


def check_both_entries(pkg, solver, inst, M, default_cap, table, stages, model_inst=None, model_table=None, batches=None):
    """host and device entry against the model: mask, per-stage counts, template counts, on-cap counts -> the host call's
    stats and the model's (selected, kept, sets).  model_inst / model_table: a translated copy the model can walk"""
    s, e, ids, tids, n_templates, lengths = inst
    n = s.size
    ms, me, mids, _, _, mlengths = model_inst or inst
    mtab = model_table or table
    counters = []
    want, selected, kept, sets = tpm.staged(ms, me, mids, tids, n_templates, mlengths, M, default_cap, *mtab, stages=stages,
                                            counters=counters, batches=batches)
    caps = pm.cap_arrays(mlengths, default_cap, *mtab)
    assert tpm.covers(ms, me, mids, caps, sets[-1]) and tm.whole_templates(sets[-1], tids, n_templates)
    seg_on, tpl_on = tpm.on_cap(ms, me, mids, tids, caps)
    hist, used, largest = tm.template_counts(tids, n_templates)
    out = None
    for entry in ("host", "device"):
        solve = solve_host_prefilled if entry == "host" else solve_device
        got, st, ts, qs = solve(pkg, solver, inst, M, default_cap, table, stages)
        diff = int(np.count_nonzero(pm.unpack(got ^ want, n))) if n else 0
        assert np.array_equal(got, want), (entry, M, default_cap, stages, diff)
        k = len(selected)
        assert ts.n_stages == k and list(ts.target)[:k] == (tm.default_stages(M) if stages is None else list(stages))
        assert list(ts.n_selected)[:k] == selected and list(ts.n_kept)[:k] == kept, (entry, M, default_cap, stages)
        assert st.n_kept == selected[0] and ts.sweeps[0] == 0
        assert list(zip(list(ts.capped_positions)[:k], list(ts.demand)[:k])) == counters, (entry, M, default_cap, stages)
        assert all(list(getattr(ts, f))[k:] == [0] * (16 - k) for f in STAGE_FIELDS)
        assert list(ts.size_hist) == hist and ts.n_templates_used == used and ts.max_template_size == largest
        assert ts.n_templates_kept == tm.kept_templates(sets[-1], tids)
        for j in range(1, k):
            assert (ts.sweeps[j] >= 1) == (ts.demand[j] > 0) == (selected[j] > 0), (entry, j, ts.as_dict())
        assert (qs.n_segments_on_cap, qs.n_templates_on_cap) == (seg_on, tpl_on), (entry, qs.as_dict())
        if table[0] is not None and model_table is None:
            rows = [pm.clipped_regions(int(L), table[1][a:b], table[2][a:b], table[3][a:b])
                    for L, a, b in zip(lengths, table[0][:-1], table[0][1:])]
            assert qs.regions_in == int(table[0][-1]) and qs.regions_used == sum(len(r) for r in rows)
            assert qs.positions_in_regions == sum(b - a + 1 for r in rows for a, b, _ in r)
        out = out or (st, ts, qs)
    got, _, _, _ = solver.solve_templates_profile(s, e, ids, tids, n_templates, lengths, M, default_cap, *table, stages=stages)
    assert np.array_equal(got, want)
    return out, (selected, kept, sets)


# ------------------------------------------------------------------------------------------ instances
def segments(seed, n, M, n_contigs=3, unplaced=0.05, empty=None):
    """n segments of spans 20 .. 200 on contigs of 500 .. 5 000 positions, depth about 2 .. 8 x M where n allows it (the
    contigs shrink towards 500 positions, then the spans towards 20), some unplaced, shuffled; contig `empty` (of 700
    positions) gets no segment"""
    rng = np.random.default_rng(seed)
    depth = float(rng.uniform(2, 8)) * M
    hi = 200
    per = n * (20 + hi) / 2 / depth / n_contigs
    while per > 5000 and hi > 40:
        hi -= 20
        per = n * (20 + hi) / 2 / depth / n_contigs
    lengths = np.clip(rng.uniform(0.7, 1.3, size=n_contigs) * per, 500, 5000).astype(np.uint32)
    ids = rng.integers(0, n_contigs, size=n).astype(np.uint32)
    span = rng.integers(20, hi + 1, size=n)
    s = (rng.random(n) * (lengths[ids].astype(np.int64) - span + 1)).astype(np.int64)
    e = s + span - 1
    if empty is not None:
        lengths = np.insert(lengths, empty, 700).astype(np.uint32)
        ids[ids >= empty] += 1
    ids[rng.random(n) < unplaced] = NO_CONTIG
    return s.astype(np.uint32), e.astype(np.uint32), ids, lengths


SIZES = [0, 1, 63, 64, 65, 4097, 20_000]
THREE = {1: [1], 3: [1, 2, 3], 10: [2, 5, 10]}


@pytest.mark.parametrize("dc", [0, 1, 2])
@pytest.mark.parametrize("M", [1, 3, 10])
@pytest.mark.parametrize("n", SIZES)
def test_random_calls_equal_the_model(pkg, solver, n, M, dc):
    """template sizes 1 .. 6 and one template of 1 000 segments (where n allows) dealt through a permutation, three or
    four contigs with one that holds no segment, unplaced segments; random regions with caps 0 .. 2 M, a cap-0 run of at
    least 150 positions per contig, regions that reach beyond their contig; default_cap = dc x M; the default schedule,
    the one stage [M] and three stages"""
    seed = 1000 + 21 * n + 3 * M + dc
    s, e, ids, lengths = segments(seed, n, M, n_contigs=2 + (n + M) % 2, empty=1)
    tids, n_templates = tm.random_templates(np.random.default_rng(seed), n, large=1000 if n >= 4097 else 0)
    table = pm.random_regions(np.random.default_rng(seed + 1), lengths, 2 * M, zero_run=150)
    if table[3].size:
        table[3][0] = 2 * M                                              # a cap above M, beside the cap-0 runs
    inst = (s, e, ids, tids, n_templates, lengths)
    assert not (ids == 1).any() and (table[3] == 0).any()
    later = 0
    for stages in (None, [M], THREE[M]):
        (st, ts, qs), (selected, _, _) = check_both_entries(pkg, solver, inst, M, dc * M, table, stages)
        later += sum(selected[1:])
    if n >= 4097 and M > 1:
        assert later > 0                                                 # the later stages had something to select


# ------------------------------------------------------------------------------------------ ltot % 4, region borders
@pytest.mark.parametrize("tail", [0, 1, 2, 3])
def test_need_tails_region_borders_and_a_contig_of_one_position(pkg, solver, tail):
    """the batch's axis has ltot % 4 = tail; contig 0 has one position (with segments on it); regions begin and end at
    every p % 4 of the axis, the last one on the axis' last position: the groups of four that k_tpl_profile_need takes
    whole end before it"""
    rng = np.random.default_rng(300 + tail)
    L1 = 119 + tail
    lengths = np.array([1, L1], np.uint32)
    assert int(lengths.sum()) % 4 == tail
    regs = [(3, 3, 2), (8, 10, 1), (13, 17, 0), (22, 23, 5), (27, 32, 3), (40, 40, 0), (41, 43, 4), (50, 55, 2),
            (57, 60, 6), (66, 72, 1), (L1 - 3, L1 + 10, 3)]
    glob = [(a + 1, min(b, L1 - 1) + 1) for a, b, _ in regs]             # contig 1 begins at position 1 of the axis
    assert {a % 4 for a, _ in glob} == {b % 4 for _, b in glob} == {0, 1, 2, 3}
    r0, r1, caps = (np.array(x, np.uint32) for x in zip(*regs))
    table = (np.array([0, 0, len(regs)], np.uint32), r0, r1, caps)
    n = 500
    ids = np.ones(n, np.uint32)
    ids[:30] = 0
    span = rng.integers(1, 25, size=n)
    s = (rng.random(n) * (L1 - span + 1)).astype(np.int64)
    s[30:50] = L1 - span[30:50]                                          # segments that end on the axis' last position
    e = s + span - 1
    s[:30], e[:30] = 0, 0
    tids, n_templates = tm.random_templates(rng, n, max_size=3)
    inst = (s.astype(np.uint32), e.astype(np.uint32), ids, tids, n_templates, lengths)
    for M, dc, stages in ((4, 4, None), (6, 2, [2, 3, 6]), (3, 0, None)):
        (_, ts, _), _ = check_both_entries(pkg, solver, inst, M, dc, table, stages)
        assert sum(ts.sweeps[1:ts.n_stages]) >= 1


# ------------------------------------------------------------------------------------------ region-table forms
def short_region_instance(n_regions, pitch, width, seed):
    """n_regions regions of `width` positions every `pitch` on one contig, caps 0 .. 8 cycling, default_cap 4; segments
    of spans 20 .. 120 about 20 deep, templates of 1 .. 6"""
    rng = np.random.default_rng(seed)
    L = n_regions * pitch + 50
    r0 = np.arange(n_regions, dtype=np.int64) * pitch + 1
    r1 = r0 + width - 1
    caps = (np.arange(n_regions) * 7) % 9
    n = int(20 * L / 70)
    span = rng.integers(20, 121, size=n)
    s = (rng.random(n) * (L - span + 1)).astype(np.int64)
    tids, n_templates = tm.random_templates(rng, n)
    inst = (s.astype(np.uint32), (s + span - 1).astype(np.uint32), np.zeros(n, np.uint32), tids, n_templates,
            np.array([L], np.uint32))
    return inst, (np.array([0, n_regions], np.uint32), r0.astype(np.uint32), r1.astype(np.uint32), caps.astype(np.uint32))


@pytest.mark.parametrize("n_regions, pitch, width", [(4095, 3, 1), (4096, 3, 1), (4097, 3, 1), (10_000, 4, 2)])
def test_region_table_in_lds_at_its_limit_and_in_l2_in_a_later_stage(pkg, solver, n_regions, pitch, width):
    """4 095 .. 4 097 one-position regions: the LDS form of k_tpl_profile_need at its limit and the L2 form just past it;
    10 000 short regions.  Stage 2 has candidates and demand, so the kernel under test builds a need that is swept"""
    inst, table = short_region_instance(n_regions, pitch, width, n_regions)
    (_, ts, qs), (selected, _, _) = check_both_entries(pkg, solver, inst, 4, 4, table, None)
    assert ts.n_stages == 2 and ts.sweeps[1] > 0 and selected[1] > 0 and ts.demand[1] > 0
    assert qs.regions_used == n_regions


# ------------------------------------------------------------------------------------------ credit and cap edges
def test_saturated_credit_queues_no_sweep(pkg, solver):
    """templates of two identical segments at M = 2 under caps 2 and 1: stage 1 at c_1 = 1 keeps one segment per demand,
    its twin doubles the depth, so wherever a segment is left the credit has reached c_2 <= 2 -- stage 2 finds
    candidates, asks for nothing and queues no sweep"""
    rng = np.random.default_rng(5)
    lengths = np.array([3000, 2000], np.uint32)
    n_t = 1500
    ids = np.repeat(rng.integers(0, 2, size=n_t), 2).astype(np.uint32)
    span = np.repeat(rng.integers(1, 120, size=n_t), 2)
    s = np.repeat(rng.random(n_t), 2)
    s = (s * (lengths[ids].astype(np.int64) - span + 1)).astype(np.int64)
    tids = (np.arange(2 * n_t) // 2).astype(np.uint32)
    inst = (s.astype(np.uint32), (s + span - 1).astype(np.uint32), ids, tids, n_t, lengths)
    table = (np.array([0, 2, 3], np.uint32), np.array([100, 2000, 0], np.uint32), np.array([900, 2500, 1999], np.uint32),
             np.array([1, 2, 1], np.uint32))
    (st, ts, qs), (selected, kept, _) = check_both_entries(pkg, solver, inst, 2, 2, table, None)
    assert ts.n_stages == 2 and list(ts.target)[:2] == [1, 2]
    assert kept[0] < s.size                                              # candidates are left ...
    assert ts.n_selected[1] == 0 and ts.n_kept[1] == ts.n_kept[0] == 2 * ts.n_selected[0]
    assert ts.demand[1] == 0 and ts.sweeps[1] == 0                       # ... and nothing is asked of them


def test_caps_that_are_all_zero_keep_nothing(pkg, solver):
    """default_cap 0 and regions at 0: every batch is skipped in every stage; and with one positive region on one
    contig, only the templates that reach it come out"""
    s, e, ids, lengths = segments(41, 4097, 3)
    tids, n_templates = tm.random_templates(np.random.default_rng(41), 4097, large=1000)
    inst = (s, e, ids, tids, n_templates, lengths)
    zero = (np.array([0, 1, 1, 2], np.uint32), np.array([10, 0], np.uint32), np.array([400, 99], np.uint32),
            np.array([0, 0], np.uint32))
    for table in (NO_TABLE, zero):
        (st, ts, qs), (selected, kept, _) = check_both_entries(pkg, solver, inst, 3, 0, table, None)
        assert kept == [0, 0] and ts.n_templates_kept == 0 and qs.n_segments_on_cap == qs.n_templates_on_cap == 0
        assert list(ts.sweeps)[:2] == [0, 0] and list(ts.demand)[:2] == [0, 0]
    one = (zero[0], zero[1], zero[2], np.array([0, 2], np.uint32))
    (st, ts, qs), (selected, kept, sets) = check_both_entries(pkg, solver, inst, 3, 0, one, [1, 2, 3])
    assert 0 < kept[-1] < 4097 and 0 < qs.n_segments_on_cap < int((ids == 2).sum())


def test_a_cap_of_2_to_the_31_minus_1_and_a_ceiling_that_matters(pkg, solver):
    """a cap of 2^31 - 1 beside the cut bit (its stage caps are computed in 64 bits: (2^31 - 1) x T does not fit 32), and
    caps 1, 3, 5, 7 under M = 4 with stages [1, 4] and [3, 4]: ceil(cap / 4) and ceil(3 cap / 4) are no multiples"""
    s, e, ids, lengths = segments(43, 4097, 4)
    tids, n_templates = tm.random_templates(np.random.default_rng(43), 4097, max_size=2)
    inst = (s, e, ids, tids, n_templates, lengths)
    L0 = int(lengths[0])
    table = (np.array([0, 5, 5, 5], np.uint32), np.array([0, 100, 200, 300, 400], np.uint32),
             np.array([99, 199, 299, 399, L0 + 5], np.uint32), np.array([1, 3, 5, 7, 2**31 - 1], np.uint32))
    assert [int(tpm.stage_cap(c, 1, 4)) for c in (1, 3, 5, 7, 2**31 - 1)] == [1, 1, 2, 2, 2**29]
    assert [int(tpm.stage_cap(c, 3, 4)) for c in (1, 3, 5, 7)] == [1, 3, 4, 6]
    for stages in ([1, 4], [3, 4], None):
        (st, ts, qs), (selected, _, _) = check_both_entries(pkg, solver, inst, 4, 6, table, stages)
        assert selected[1] > 0


# ------------------------------------------------------------------------------------------ two position batches
TWO_BATCH_LENGTHS = [1_200_000_000, 1_150_000_123, 5_000]


def island_segments(seed, lengths, max_span, per_island=40):
    """segments of spans 1 .. max_span in islands at both ends of every contig and around a multiple of 64 inside it,
    shuffled over the input"""
    rng = np.random.default_rng(seed)
    ss, ee, ii = [], [], []
    for c, L in enumerate(lengths):
        for a in (0, 64 * int(rng.integers(L // 256, L // 128)), L - 1):
            span = np.minimum(rng.integers(1, max_span + 1, size=per_island), L)
            span[0], span[1] = min(max_span, L), 1
            s = np.clip(a - rng.integers(0, span) + rng.integers(-2, 3, size=per_island), 0, L - span)
            ss.append(s); ee.append(s + span - 1); ii.append(np.full(per_island, c))
    s, e, ids = (np.concatenate(x) for x in (ss, ee, ii))
    perm = rng.permutation(s.size)
    return u32(s[perm]), u32(e[perm]), u32(ids[perm]), u32(lengths)


@functools.lru_cache(maxsize=None)
def two_batch_instance():
    s, e, ids, lengths = island_segments(83, TWO_BATCH_LENGTHS, 300)
    rng = np.random.default_rng(84)
    tids, n_templates = tm.random_templates(rng, s.size, max_size=4)
    # regions over the islands of contigs 1 and 2 (the second batch): caps 0 .. 8, and a long cap-0 run between islands
    L1 = TWO_BATCH_LENGTHS[1]
    mid = int(np.median(s[(ids == 1) & (s > 1000) & (s < L1 - 1000)]))    # inside the island in the middle of contig 1
    regs1 = [(0, 120, 2), (121, 250, 0), (251, 400, 7), (1000, mid - 1000, 0), (mid - 50, mid + 60, 3),
             (L1 - 300, L1 - 150, 8), (L1 - 149, L1 + 50, 1)]
    regs2 = [(0, 99, 0), (100, 2000, 6), (4000, 4999, 1)]
    rows = regs1 + regs2
    table = (u32([0, 0, len(regs1), len(rows)]), u32([r[0] for r in rows]), u32([r[1] for r in rows]), u32([r[2] for r in rows]))
    moved = pm.compact(s, e, ids, lengths, *table)
    return (s, e, ids, tids, n_templates, lengths), table, (moved[0], moved[1], moved[2], tids, n_templates, moved[3]), moved[4:]


def test_two_position_batches_with_regions_in_the_second_and_templates_across_both(pkg, solver):
    """two contigs of about 1.2e9 positions (one call takes 2^31 - 2) and a short third: contig 0 is a batch of its own
    without regions (the plain route in stage 1), the regions lie in the second batch, and most templates have segments
    in both.  Under cut_points = 1 (stretches): one chain per contig would walk 1.2e9 positions"""
    inst, table, model_inst, model_table = two_batch_instance()
    s, e, ids, tids, n_templates, lengths = inst
    L = lengths.astype(np.int64)
    assert int(L[:2].sum()) > (1 << 31) - 2 >= int(L[1:].sum())
    batch_of = (ids != 0).astype(np.int64)
    first = np.full(n_templates, -1)
    first[tids[::-1]] = batch_of[::-1]
    assert int(np.count_nonzero(batch_of != first[tids])) > 50
    with solver.options(cut_points=1):
        (st, ts, qs), (selected, kept, _) = check_both_entries(pkg, solver, inst, 5, 5, table, None, model_inst, model_table,
                                                               batches=[[0], [1, 2]])
    assert st.total_length == int(L.sum()) and st.n_contigs == 3
    assert ts.sweeps[1] == 2 and ts.n_selected[1] > 0
    assert qs.regions_in == qs.regions_used == int(table[0][-1])


# ------------------------------------------------------------------------------------------ on-cap counts
def test_on_cap_counts_at_region_borders_and_over_10_000_zero_regions(pkg, solver):
    """segments that end one position before a positive region, that begin at its last position, that begin one behind
    it; a long segment over 10 000 cap-0 regions (default_cap 0: not on cap) and the same under default_cap 1 (on cap
    between the regions); a long segment that reaches the one positive region behind them"""
    n_zero = 10_000
    L = 4 * n_zero + 2000
    r0 = np.concatenate([np.arange(n_zero) * 4 + 1, [4 * n_zero + 100, 4 * n_zero + 500]])
    r1 = np.concatenate([np.arange(n_zero) * 4 + 2, [4 * n_zero + 199, 4 * n_zero + 500]])
    caps = np.concatenate([np.zeros(n_zero, np.int64), [3, 2]])
    P0, P1, Q = 4 * n_zero + 100, 4 * n_zero + 199, 4 * n_zero + 500
    rows = [(P0 - 40, P0 - 1), (P0 - 40, P0), (P1, P1 + 30), (P1 + 1, P1 + 30), (Q, Q), (Q - 1, Q - 1), (Q + 1, Q + 9),
            (0, 4 * n_zero - 1), (0, 4 * n_zero - 1), (5, P0 - 1), (5, P0), (0, 0), (1, 2), (3, 4), (L - 1, L - 1)]
    rng = np.random.default_rng(9)
    extra = 400
    xs = rng.integers(P0 - 150, Q + 50, size=extra)
    xe = np.minimum(xs + rng.integers(0, 60, size=extra), L - 1)
    s = np.concatenate([[a for a, _ in rows], xs])
    e = np.concatenate([[b for _, b in rows], xe])
    n = s.size
    ids = np.zeros(n, np.uint32)
    ids[-5:] = NO_CONTIG                                                 # unplaced segments are never on cap
    tids, n_templates = tm.random_templates(rng, n, n_templates=n + 33, max_size=3)
    inst = (u32(s), u32(e), ids, tids, n_templates, np.array([L, 50], np.uint32))
    table = (u32([0, r0.size, r0.size]), u32(r0), u32(r1), u32(caps))
    caps0 = pm.cap_arrays(inst[5], 0, *table)
    seg0, _ = tpm.on_cap(inst[0], inst[1], ids, tids, caps0)
    seg1, _ = tpm.on_cap(inst[0], inst[1], ids, tids, pm.cap_arrays(inst[5], 1, *table))
    assert seg1 > seg0 + 8                                               # the long segments and the ones at 0, 3 .. 4, L - 1
    for dc in (0, 1):
        (_, ts, qs), _ = check_both_entries(pkg, solver, inst, 3, dc, table, None)
        assert qs.n_segments_on_cap == (seg0, seg1)[dc] and qs.regions_used == n_zero + 2


# ------------------------------------------------------------------------------------------ the identities
def identity_instance(M, n=4097):
    s, e, ids, lengths = segments(500 + M, n, M, empty=2)
    tids, n_templates = tm.random_templates(np.random.default_rng(500 + M), n, large=1000)
    return s, e, ids, tids, n_templates, lengths


@pytest.mark.parametrize("M", [1, 3, 10])
def test_identity_1_no_region_and_default_cap_m_is_solve_templates_with_every_stat(pkg, solver, M):
    inst = identity_instance(M)
    s, e, ids, tids, n_templates, lengths = inst
    beyond = (np.array([0, 1, 1, 1, 2], np.uint32), lengths[[0, 3]], lengths[[0, 3]] + 7, np.array([0, 9], np.uint32))
    for stages in (None, [M], THREE[M]):
        want, st_t, ts_t = solver.solve_templates(s, e, ids, tids, n_templates, lengths, M, stages)
        want = want.copy()
        for table in (NO_TABLE, beyond):                                # regions that begin beyond their contig are not used
            for solve in (solve_host_prefilled, solve_device):
                got, st, ts, qs = solve(pkg, solver, inst, M, M, table, stages)
                assert np.array_equal(got, want), (M, stages)
                for name, _ in pkg.TemplateStats._fields_:
                    a, b = getattr(ts, name), getattr(ts_t, name)
                    if not name.startswith("ms_") and name != "reserved":
                        assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), (name, M, stages)
                assert (st.n_kept, st.n_reads, st.path, st.sort_passes) == (st_t.n_kept, st_t.n_reads, st_t.path, st_t.sort_passes)
                assert qs.regions_used == 0 and qs.regions_in == (0 if table[0] is None else 2)
                assert qs.n_segments_on_cap == int((ids != NO_CONTIG).sum())
                assert qs.n_templates_on_cap == np.unique(tids[ids != NO_CONTIG]).size


@pytest.mark.parametrize("M, n", [(1, 65), (3, 4097), (10, 20_000)])
def test_identity_2_distinct_ids_and_one_stage_give_the_mask_of_solve_profile(pkg, solver, M, n):
    s, e, ids, lengths = segments(600 + n, n, M)
    tids = np.random.default_rng(n).permutation(n).astype(np.uint32)
    table = pm.random_regions(np.random.default_rng(n + 1), lengths, 2 * M, zero_run=100)
    for dc in (0, M, 2 * M):
        want = solver.solve_profile(s, e, ids, lengths, dc, *table).copy()
        kept = solver.last_stats.n_kept
        for solve in (solve_host_prefilled, solve_device):
            got, st, ts, qs = solve(pkg, solver, (s, e, ids, tids, n, lengths), M, dc, table, [M])
            assert np.array_equal(got, want), (M, dc)
            assert ts.n_selected[0] == ts.n_kept[0] == ts.n_templates_kept == kept == st.n_kept


@pytest.mark.parametrize("M", [1, 3, 10])
def test_identity_3_caps_all_m_with_regions_give_the_mask_of_solve_templates(pkg, solver, M):
    inst = identity_instance(M)
    s, e, ids, tids, n_templates, lengths = inst
    offs, r0, r1, caps = pm.random_regions(np.random.default_rng(M), lengths, 5)
    assert offs[-1] > 0
    table = (offs, r0, r1, np.full(r0.size, M, np.uint32))
    for stages in (None, [M], THREE[M]):
        want, _, ts_t = solver.solve_templates(s, e, ids, tids, n_templates, lengths, M, stages)
        want = want.copy()
        for solve in (solve_host_prefilled, solve_device):
            got, st, ts, qs = solve(pkg, solver, inst, M, M, table, stages)
            assert np.array_equal(got, want), (M, stages)
            assert qs.regions_used > 0
            for f in STAGE_FIELDS:                                       # need[] is the same array: so are its counters
                assert list(getattr(ts, f)) == list(getattr(ts_t, f)), (f, M, stages)


@pytest.mark.parametrize("M", [3, 10])
def test_identity_4_one_stage_is_solve_profile_and_the_template_completion(pkg, solver, M):
    inst = identity_instance(M)
    s, e, ids, tids, n_templates, lengths = inst
    n = s.size
    table = pm.random_regions(np.random.default_rng(M + 7), lengths, 2 * M, zero_run=100)
    for dc in (0, M, 2 * M):
        plain = pm.unpack(solver.solve_profile(s, e, ids, lengths, dc, *table), n)
        got, st, ts, qs = solver.solve_templates_profile(s, e, ids, tids, n_templates, lengths, M, dc, *table, stages=[M])
        assert np.array_equal(pm.unpack(got, n), tm.complete(plain, tids, n_templates))
        assert ts.n_selected[0] == int(plain.sum())


# ------------------------------------------------------------------------------------------ errors
def test_errors_and_a_bad_id_with_the_mask_cleared(pkg, solver):
    n = 4097
    s, e, ids, lengths = segments(5, n, 3)
    tids, n_templates = tm.random_templates(np.random.default_rng(5), n)
    table = pm.random_regions(np.random.default_rng(6), lengths, 6)
    go = lambda **kw: solver.solve_templates_profile(s, e, ids, tids, n_templates, lengths,
                                                     **{"max_coverage": 3, "default_cap": 3, "region_offsets": table[0],
                                                        "region_starts": table[1], "region_ends": table[2],
                                                        "region_caps": table[3], **kw})
    overlap = dict(region_offsets=u32([0, 2, 2, 2]), region_starts=u32([10, 20]), region_ends=u32([20, 30]),
                   region_caps=u32([1, 1]))
    cases = [(dict(stages=[2, 2, 3]), QMCP_EINVAL, "stages[1]"), (dict(stages=[1, 2]), QMCP_EINVAL, "max_coverage"),
             (dict(max_coverage=0), QMCP_EINVAL, "max_coverage"), (dict(flags=1), QMCP_EINVAL, "flag"),
             (overlap, QMCP_EINVAL, "region table"), (dict(default_cap=2**31), QMCP_ERANGE, "default_cap"),
             (dict(overlap, region_ends=u32([15, 30]), region_caps=u32([1, 2**31])), QMCP_ERANGE, "cap"),
             (dict(overlap, region_offsets=u32([1, 2, 2, 2])), QMCP_EINVAL, "region table")]
    for kw, code, word in cases:
        with pytest.raises(pkg.QmcpError) as err:
            go(**kw)
        assert err.value.code == code and word in str(err.value), (kw, str(err.value))
    for where in (0, 2048, n - 1):
        bad = tids.copy()
        bad[where] = n_templates
        with pytest.raises(pkg.QmcpError) as err:
            solver.solve_templates_profile(s, e, ids, bad, n_templates, lengths, 3, 3, *table)
        assert err.value.code == QMCP_EINVAL and "template id" in str(err.value)
        cols = [_dev(x) for x in (s, e, ids, bad)]
        d_mask = torch.full((pkg.mask_words(n) + 1,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(pkg.QmcpError) as err:
            solver.solve_templates_profile_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(),
                                                  cols[3].data_ptr(), n, n_templates, lengths, 3, 3, d_mask.data_ptr(), *table)
        assert err.value.code == QMCP_EINVAL
        torch.cuda.synchronize()
        out = d_mask.cpu().numpy()
        assert (out[:-1] == 0).all() and out[-1] == -1                   # cleared, and nothing behind it touched
    check_both_entries(pkg, solver, (s, e, ids, tids, n_templates, lengths), 3, 3, table, None)   # the context is still good


# ------------------------------------------------------------------------------------------ the file flow
def check_file_flow(pkg, solver, tmp_path, name, refs, records, M, table_of, stages=None, **keywords):
    """downsample_bam(template_aware=True, template_targets= | template_profile=) writes exactly the records of the
    model's kept templates, in file order; table_of(lengths) -> (default_cap, offs, r0, r1, caps) restates the file's
    table for the model"""
    path = tmp_path / f"{name}.bam"
    bam_py.write_bam(path, refs, records)
    header, parsed, _ = bam_py.parse(path)
    segs = tb.expected_segments(records)
    lengths = np.array([L for _, L in refs], np.uint32)
    default_cap, *table = table_of(lengths)
    cols = (segs["starts"], segs["ends"], segs["contig_ids"], segs["template_ids"], segs["n_templates"], lengths)
    want, _, kept, sets = tpm.staged(*cols, M, default_cap, *table, stages=stages)
    caps = pm.cap_arrays(lengths, default_cap, *table)
    assert tpm.covers(cols[0], cols[1], cols[2], caps, sets[-1])
    kept_records = np.unique(np.asarray(segs["segment_records"], np.int64)[sets[-1]])
    out, report = tmp_path / f"{name}.out.bam", tmp_path / f"{name}.tsv"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, template_aware=True,
                                 template_stages=stages, template_report=report, **keywords)
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == kept_records.size == len(orecs) > 0
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_records.tolist()]
    assert pkg.check_bam(out)[0]
    rows = dict(line.split("\t", 1) for line in report.read_text().splitlines() if "\t" in line)
    seg_on, tpl_on = tpm.on_cap(cols[0], cols[1], cols[2], cols[3], caps)
    assert int(rows["templates_kept"]) == tm.kept_templates(sets[-1], segs["template_ids"])
    assert int(rows["segments_kept"]) == kept[-1]
    assert (int(rows["segments_on_cap"]), int(rows["templates_on_cap"])) == (seg_on, tpl_on)
    clipped = [pm.clipped_regions(int(L), table[1][a:b], table[2][a:b], table[3][a:b])
               for L, a, b in zip(lengths, table[0][:-1], table[0][1:])]
    assert int(rows["regions_in"]) == int(table[0][-1]) and int(rows["regions_used"]) == sum(len(r) for r in clipped)
    assert int(rows["positions_in_regions"]) == sum(b - a + 1 for r in clipped for a, b, _ in r)
    return segs, sets[-1], written


def mixed_file(rng, refs):
    """template_bams.mixed_records (pairs, spliced reads, split reads, secondaries, unmapped mates) plus a spliced read
    whose intron spans a target border and a split read whose supplementary lies off target"""
    records = tb.mixed_records(rng, refs, 700)
    # chrA's targets end at 2 599: the first block lies on target, the intron spans the border, the second block is off
    records.insert(len(records) // 3, tb.record("border", 0, 0, 2500, 60, [(80, "M"), (300, "N"), (60, "M")]))
    # the primary on chrA's first target, the supplementary on chrC, which has no target
    records.insert(len(records) // 2, tb.record("split", 0, 0, 300, 60, [(70, "M"), (60, "S")]))
    records.insert(2 * len(records) // 3, tb.record("split", 0x800, 2, 100, 60, [(40, "H"), (50, "M")]))
    sizes = np.bincount(tb.expected_segments(records)["template_ids"])
    assert sizes.max() >= 4 and (sizes == 1).any()
    return records


def test_downsample_bam_with_template_targets_and_with_template_profile(pkg, solver, tmp_path):
    refs = [("chrA", 5000), ("chrB", 3000), ("chrC", 800)]
    records = mixed_file(np.random.default_rng(11), refs)
    names = [r for r, _ in refs]
    M = 6
    bed = tmp_path / "targets.bed"
    bed.write_text("chrA\t200\t1500\nchrA\t1400\t2600\nchrB\t100\t900\nchrA\t4000\t4400\n")

    def targets_table(padding):
        def table_of(lengths):
            t = pkg.targets_from_bed(bed, names)
            return (0, *tpm.targets_as_regions(*t, lengths, padding, M))
        return table_of

    for padding, stages in ((0, None), (25, [1, 2, 6])):
        segs, kept, written = check_file_flow(pkg, solver, tmp_path, f"targets{padding}", refs, records, M,
                                              targets_table(padding), stages, template_targets=bed,
                                              template_target_padding=padding)
        assert 0 < written < len(records) and (segs["contig_ids"] == NO_CONTIG).any()
        # whole templates came out: kept segments lie off target too, none of them selected there
        caps = pm.cap_arrays([L for _, L in refs], 0, *targets_table(padding)([L for _, L in refs])[1:])
        off = [i for i in np.flatnonzero(kept).tolist() if segs["contig_ids"][i] != NO_CONTIG
               and not caps[segs["contig_ids"][i]][segs["starts"][i]:segs["ends"][i] + 1].any()]
        assert len(off) > 0
    graph = tmp_path / "caps.bedgraph"
    graph.write_text("chrA\t0\t1000\t2\nchrA\t1000\t1800\t0\nchrA\t2500\t3500\t9\nchrB\t500\t700\t12\nchrC\t0\t800\t1\n")

    def profile_table(lengths):
        return (M, *pkg.profile_from_bedgraph(graph, names))

    for stages in (None, [6]):
        segs, kept, written = check_file_flow(pkg, solver, tmp_path, "profile", refs, records, M, profile_table, stages,
                                              template_profile=graph)
        assert 0 < written < len(records)
    # a stage list that does not end at max_coverage is the library's to refuse
    with pytest.raises(ValueError):
        pkg.downsample_bam("quasi-mcp-hip", tmp_path / "profile.bam", tmp_path / "no.bam", M, per_reference=True,
                           template_aware=True, template_profile=graph, template_stages=[3, 5])
    assert not (tmp_path / "no.bam").exists()


# ------------------------------------------------------------------------------------------ cost
def test_the_call_under_caps_costs_little_more_than_solve_templates(pkg, solver):
    """2^20 segments of two spans (100 and 150) as templates of two on 4 contigs, shuffled; near_uniform = -1,
    speculation = -1 and cut_points = -1, so that stage 1 of qmcp_hip_solve_templates_device takes the sort-based mixed
    route as one chain per contig, as the capped route does.  2 000 regions all at M, default_cap = M.  Wall time of the
    whole blocking device call, medians of 5 after a warm-up, alternating; the masks are compared (identity 3).
    QMCP_TEMPLATES_PROFILE_TIME_OUT=<file> keeps the figures."""
    n_contigs, L, M = 4, 250_000, 60
    n = 1 << 20
    rng = np.random.default_rng(79)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), n // n_contigs)
    span = np.where(rng.random(n) < 0.5, 100, 150).astype(np.int64)
    s = (rng.random(n) * (L - span + 1)).astype(np.int64)
    e, s = (s + span - 1).astype(np.uint32), s.astype(np.uint32)
    perm = rng.permutation(n)
    s, e, ids = s[perm], e[perm], ids[perm]
    tids = (np.arange(n) // 2).astype(np.uint32)
    lengths = np.full(n_contigs, L, np.uint32)
    starts_1 = np.arange(0, L, 500, dtype=np.uint32)
    offs = (np.arange(n_contigs + 1) * starts_1.size).astype(np.uint32)
    r0 = np.tile(starts_1, n_contigs)
    r1 = r0 + 399
    caps = np.full(r0.size, M, np.uint32)
    ds, de, di, dt = _dev(s), _dev(e), _dev(ids), _dev(tids)
    d_plain = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device="cuda:0")
    d_caps = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    plain = lambda: solver.solve_templates_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), dt.data_ptr(), n, n // 2,
                                                  lengths, M, d_plain.data_ptr())
    capped = lambda: solver.solve_templates_profile_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), dt.data_ptr(), n,
                                                           n // 2, lengths, M, M, d_caps.data_ptr(), offs, r0, r1, caps)
    with solver.options(near_uniform=-1, speculation=-1, cut_points=-1):
        plain(); capped()                                                        # warm-up: arena growth
        t_plain, t_caps, ms_need, ms_stage = [], [], [], []
        for _ in range(5):
            t_plain.append(timed(plain))
            assert solver.last_stats.path == 2 and solver.last_stats.spec_boundaries == 0
            plain_stage = list(solver.last_template_stats.ms_stage)[:2]
            t_caps.append(timed(capped))
            ms_need.append(float(solver.last_template_profile_stats.ms_need))
            ms_stage.append(list(solver.last_template_stats.ms_stage)[:2])
    assert torch.equal(d_plain, d_caps)
    assert solver.last_template_stats.sweeps[1] >= 1 and solver.last_template_profile_stats.n_segments_on_cap == n
    a, b = statistics.median(t_plain), statistics.median(t_caps)
    figures = {"segments": n, "contigs": n_contigs, "positions": int(n_contigs * L), "M": M, "regions": int(r0.size),
               "templates_ms_median": round(a, 3), "templates_ms_runs": [round(x, 3) for x in t_plain],
               "templates_profile_ms_median": round(b, 3), "templates_profile_ms_runs": [round(x, 3) for x in t_caps],
               "templates_stage_ms_last_run": [round(x, 3) for x in plain_stage],
               "templates_profile_stage_ms_last_run": [round(x, 3) for x in ms_stage[-1]],
               "ms_need_median": round(statistics.median(ms_need), 4), "ratio": round(b / a, 4), "margin": COST_MARGIN}
    print("templates_profile_time " + json.dumps(figures))
    out = os.environ.get("QMCP_TEMPLATES_PROFILE_TIME_OUT")
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(figures, indent=1) + "\n")
    assert b <= COST_MARGIN * a, figures
