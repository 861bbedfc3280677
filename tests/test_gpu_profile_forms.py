"""qmcp_hip_solve_profile_*: every capped sweep form and both region-table paths, pinned.  test_gpu_profile.py reaches the
forms below by luck or not at all; here a case is the smallest shape that still selects its form, every mask is compared
bit for bit with profile_model.fast_expected_mask (the rule from sorted events, tied to the first model in
test_profile_cpu.py), `demand` and `capped_positions` with profile_model.demand_and_capped -- on long axes through
profile_model.compact, the translation helper -- and every case runs under cut_points = -1 (one chain per contig) and
cut_points = 1 (stretches; the two-batch case under stretches only, see there).  profile_model.form_of restates from the
call's statistics which kernel form the launchers picked; test_census_every_form_was_taken, the last test of the file,
asserts that every form named in it was taken by a case that passed, so a case cannot slide to another form and keep
passing.  (The census counts what ran in this process: it fails when cases are deselected.)

Reads on long axes sit in a few islands, so that the model and the one-chain walk stay quick; the islands straddle
multiples of 64, multiples of the stretch window, contig borders and the last position of the axis."""
import functools

import numpy as np
import pytest
import torch

import profile_model as pm

pytestmark = pytest.mark.gpu

NO_CONTIG = 0xFFFFFFFF
CAP_MAX = (1 << 31) - 1
FORMS, NEED_FORMS, PASSES = {}, {}, {}       # what ran: form -> the cases that took it


def _dev(a, shift=0):
    t = torch.zeros(a.size + shift + 4, dtype=torch.int32, device="cuda:0")      # (a base allocation is 256-byte aligned)
    t[shift:shift + a.size] = torch.from_numpy(np.array(a, np.uint32).view(np.int32)).to("cuda:0")
    return t


# ------------------------------------------------------------------------------------------ instances
def island_instance(seed, lengths, max_span, island_contigs=None, per_island=40, max_cap=6, default=3):
    """reads of spans 1..max_span (both ends of that range present) in islands of `per_island` reads around anchors:
    per contig in island_contigs (default: all) its first and last position and a multiple of 64 inside it, and two
    multiples of the stretch window of cut_points = 1; regions with caps 0..max_cap whose edges fall around the same
    anchors, one on every such contig's first and one on its last position; 3 % of the reads unplaced"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    n_contigs = lengths.size
    first = np.concatenate([[0], np.cumsum(lengths)])
    ltot = int(first[-1])
    anchors = {c: set() for c in (range(n_contigs) if island_contigs is None else island_contigs)}
    for c in anchors:
        L = int(lengths[c])
        anchors[c] |= {0, L - 1, 64 * int(rng.integers(L // 256, L // 128))}
    windows = pm.stretch_windows(ltot, max_span, n_contigs)
    if windows:
        win = -(-ltot // windows)
        for w in (windows // 3, (2 * windows) // 3 + 1):
            c = int(np.searchsorted(first, w * win, side="right")) - 1
            if w * win < ltot:
                anchors.setdefault(c, {0, int(lengths[c]) - 1}).add(w * win - int(first[c]))
    ss, ee, ii = [], [], []
    offs, r0, r1, caps = [0], [], [], []
    pinned = False
    for c in range(n_contigs):
        L = int(lengths[c])
        edges = {0, L}
        for a in sorted(anchors.get(c, ())):
            span = np.minimum(rng.integers(1, max_span + 1, size=per_island), L)
            if not pinned:
                span[0], span[1], pinned = min(max_span, L), 1, True
            s = np.clip(a - rng.integers(0, span) + rng.integers(-2, 3, size=per_island), 0, L - span)
            ss.append(s); ee.append(s + span - 1); ii.append(np.full(per_island, c))
            edges |= {int(x) for x in np.clip(a + rng.integers(-max_span, max_span + 1, size=4), 0, L)} | {a, min(a + 1, L)}
        if c in anchors:
            edges = sorted(edges)
            if len(edges) % 2:
                del edges[1]
            rows = [(a, b - 1, int(rng.integers(0, max_cap + 1))) for a, b in zip(edges[0::2], edges[1::2])]
            for k in rng.permutation(len(rows)).tolist():                         # the order is free
                r0.append(rows[k][0]); r1.append(rows[k][1]); caps.append(rows[k][2])
        offs.append(len(r0))
    s, e, ids = (np.concatenate(x) for x in (ss, ee, ii))
    perm = rng.permutation(s.size)
    s, e, ids = s[perm].astype(np.uint32), e[perm].astype(np.uint32), ids[perm].astype(np.uint32)
    ids[(rng.random(ids.size) < 0.03) & (perm > 1)] = NO_CONTIG                   # (the two pinned spans stay placed)
    u = lambda x: np.asarray(x, np.uint32)
    return s, e, ids, u(lengths), default, u(offs), u(r0), u(r1), u(caps)


def scattered_instance(seed, lengths, max_span, n, max_regions=3, max_cap=6, default=3, unplaced=0.03, idle=0.0):
    """n reads of spans 1..max_span (clipped to their contig; both ends of the range present when contig 0 is long
    enough) anywhere on short contigs -- none on contigs of length 0 nor on a share `idle` of the others --, regions as
    profile_model.random_regions draws them"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.uint32)
    live = np.flatnonzero((lengths > 0) & (rng.random(lengths.size) >= idle))
    live = np.union1d(live, [0])
    ids = live[rng.integers(0, live.size, size=n)].astype(np.uint32)
    ids[:2] = 0
    Ls = lengths[ids].astype(np.int64)
    span = np.minimum(rng.integers(1, max_span + 1, size=n), Ls)
    span[0], span[1] = min(max_span, int(lengths[0])), 1
    s = (rng.random(n) * (Ls - span + 1)).astype(np.int64)
    e = s + span - 1
    perm = rng.permutation(n)
    s, e, ids = s[perm].astype(np.uint32), e[perm].astype(np.uint32), ids[perm]
    ids[(rng.random(n) < unplaced) & (perm > 1)] = NO_CONTIG                      # (the two pinned spans stay placed)
    offs, r0, r1, caps = pm.random_regions(rng, lengths, max_cap, max_regions=max_regions)
    if r0.size == 0:
        offs = np.concatenate([[0], np.full(lengths.size, 1)]).astype(np.uint32)
        r0, r1, caps = np.array([0], np.uint32), np.array([int(lengths[0]) - 1], np.uint32), np.array([2], np.uint32)
    return s, e, ids, lengths, default, offs, r0, r1, caps


def table_instance(seed, lengths, rows_per_contig, max_span, n, default=3):
    """n reads of spans 1..max_span on contigs whose region tables are given as (start, end) rows; caps 0..5, about a
    quarter of them 0; the rows of a contig in random order"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.uint32)
    ids = rng.integers(0, lengths.size, size=n).astype(np.uint32)
    Ls = lengths[ids].astype(np.int64)
    span = np.minimum(rng.integers(1, max_span + 1, size=n), Ls)
    s = (rng.random(n) * (Ls - span + 1)).astype(np.int64)
    e = s + span - 1
    offs, r0, r1 = [0], [], []
    for rows in rows_per_contig:
        rows = np.asarray(rows, np.int64).reshape(-1, 2)[rng.permutation(len(rows))]
        r0.append(rows[:, 0]); r1.append(rows[:, 1])
        offs.append(offs[-1] + len(rows))
    r0, r1 = np.concatenate(r0).astype(np.uint32), np.concatenate(r1).astype(np.uint32)
    caps = np.where(rng.random(r0.size) < 0.25, 0, rng.integers(1, 6, size=r0.size)).astype(np.uint32)
    return s.astype(np.uint32), e.astype(np.uint32), ids, lengths, default, np.asarray(offs, np.uint32), r0, r1, caps


def every_position_a_region(lengths):
    return [np.stack([np.arange(L), np.arange(L)], axis=1) for L in lengths]


def short_regions_with_gaps(seed, n_regions):
    """regions of 1..3 positions with gaps of 0..2 before each; returns the rows and the length they need"""
    rng = np.random.default_rng(seed)
    size, gap = rng.integers(1, 4, size=n_regions), rng.integers(0, 3, size=n_regions)
    end = np.cumsum(size + gap) - 1
    return np.stack([end - size + 1, end], axis=1), int(end[-1]) + 1


def wide_register_lengths(max_span):
    """three contigs whose positions, with spans 1..max_span, just need 33 key bits: span_bits is the width of
    max_span - 1 (9 bits from 257 on, but 6 at 64, 7 at 128 and 8 at 192), so the axis is just above 2^23 positions for
    the two longest bounds and 2^26, 2^25 and 2^24 for the others"""
    ltot = (1 << (32 - int(max_span - 1).bit_length())) + 77
    a, b = (3 * ltot) // 8 + 1, (5 * ltot) // 16
    return [a, b, ltot - a - b]


def _ten_thousand_regions():
    rows_a, len_a = short_regions_with_gaps(41, 5000)
    rows_b, len_b = short_regions_with_gaps(42, 5000)
    return table_instance(43, [len_a + 7, len_b], [rows_a, rows_b], 100, 4000)   # (a contig border behind a default-cap tail)


def _contig_lengths(seed, n_contigs, lo, hi, zero=0):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(lo, hi + 1, size=n_contigs)
    lengths[0] = hi
    if zero:
        lengths[rng.choice(np.arange(1, n_contigs), size=zero, replace=False)] = 0
    return lengths


# name -> (builder, model through profile_model.compact, the forms the case is there for)
CASES = {}
for _b, _span in ((2, 64), (3, 128), (4, 192), (6, 320), (8, 448)):
    # 33 key bits (a 1-base read is present), 5 passes; 3 chains, or 3 + windows workgroups
    CASES[f"wide keys, register form B={_b}"] = (
        functools.partial(island_instance, 100 + _b, wide_register_lengths(_span), _span), True,
        {-1: ("k64", "reg", _b, 4), 1: ("k64", "reg", _b, 1)})
    # the same forms on 32-bit records; 64 contigs are the most that get four loader waves
    CASES[f"records, 64 contigs, B={_b}"] = (
        functools.partial(scattered_instance, 200 + _b, _contig_lengths(300 + _b, 64, 500, 700), _span, 3000), False,
        {-1: ("rec", "reg", _b, 4)})
    CASES[f"records, 65 contigs, B={_b}"] = (
        functools.partial(scattered_instance, 400 + _b, _contig_lengths(500 + _b, 65, 500, 700), _span, 3000), False,
        {-1: ("rec", "reg", _b, 1), 1: ("rec", "reg", _b, 1)})
CASES.update({
    # B = 3 and B = 6 pinned by the longest span alone, with windows under cut_points = 1
    "records, longest span 128": (functools.partial(island_instance, 601, [20_000, 20_011, 19_990], 128), False,
                                  {-1: ("rec", "reg", 3, 4), 1: ("rec", "reg", 3, 4)}),
    "records, longest span 320": (functools.partial(island_instance, 602, [20_000, 20_011, 19_990], 320), False,
                                  {-1: ("rec", "reg", 6, 4), 1: ("rec", "reg", 6, 4)}),
    # 2^19 + 5 positions (20 bits) and spans 1..8 192 (13): 33 bits
    "wide keys, plain walk, rings in LDS": (
        functools.partial(island_instance, 603, [200_000, 200_000, (1 << 19) + 5 - 400_000], 8192), True,
        {-1: ("k64", "plain", "lds"), 1: ("k64", "plain", "lds")}),
    # 2^18 + 5 positions (19 bits) and spans 1..20 000 (15): 34 bits
    "wide keys, plain walk, rings in global memory": (
        functools.partial(island_instance, 604, [100_000, 100_000, (1 << 18) + 5 - 200_000], 20_000), True,
        {-1: ("k64", "plain", "global"), 1: ("k64", "plain", "global")}),
    # 2^25 + 168 positions (26 bits) and spans 1..20 000: 41 bits, six passes -- the sorted keys end in the other buffer.
    # 200 contigs keep a chain short; the islands are in six of them
    "wide keys, six passes": (
        functools.partial(island_instance, 605, [167_773] * 200, 20_000, island_contigs=(0, 1, 77, 130, 198, 199),
                          per_island=25), True,
        {-1: ("k64", "plain", "global"), 1: ("k64", "plain", "global")}),
    "records, plain walk, rings in LDS": (functools.partial(island_instance, 606, [30_000, 30_001], 600), False,
                                          {-1: ("rec", "plain", "lds"), 1: ("rec", "plain", "lds")}),
    "records, plain walk, rings in global memory": (
        functools.partial(island_instance, 607, [60_000, 50_001], 20_000, per_island=25), False,
        {-1: ("rec", "plain", "global"), 1: ("rec", "plain", "global")}),
    "255 contigs": (functools.partial(scattered_instance, 608, _contig_lengths(618, 255, 60, 140), 40, 4000), False, {}),
    "256 contigs": (functools.partial(scattered_instance, 609, _contig_lengths(619, 256, 60, 140), 40, 4000), False, {}),
    "300 contigs": (functools.partial(scattered_instance, 610, _contig_lengths(620, 300, 60, 140, zero=9), 40, 4000,
                                      idle=0.1), False, {}),
    "contigs of 1..40 positions": (
        functools.partial(scattered_instance, 611, _contig_lengths(621, 150, 1, 40), 40, 2500, max_regions=2,
                          unplaced=0.05, idle=0.2), False, {}),
    "10 000 short regions": (_ten_thousand_regions, False, {}),
})
for _L in (4095, 4096, 4097, 4098, 4099):                          # 4 096: the most regions LDS takes; every ltot % 4
    CASES[f"every position a region, {_L} positions"] = (
        functools.partial(table_instance, 700 + _L, [_L], every_position_a_region([_L]), 30, 2000), False, {})
CASES["every position a region, two contigs of 2 050"] = (                       # the border falls inside a group of four
    functools.partial(table_instance, 612, [2050, 2050], every_position_a_region([2050, 2050]), 30, 2000), False, {})


@functools.lru_cache(maxsize=None)
def instance(name):
    """the case's arrays, its mask and its two counters by the model -- computed once, shared, left unchanged"""
    build, through_compact, _ = CASES[name]
    s, e, ids, lengths, default, offs, r0, r1, caps = inst = build()
    if through_compact:
        c = pm.compact(s, e, ids, lengths, offs, r0, r1, caps)
        model = c[:4] + (default,) + c[4:]
    else:
        model = inst
    want = pm.fast_expected_mask(*model)
    counters = pm.demand_and_capped(*model)
    for a in inst + (want,):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inst, want, counters


def solve_and_check(solver, name, cut_points, record=True):
    inst, want, counters = instance(name)
    lengths = inst[3]
    with solver.options(cut_points=cut_points):
        got = solver.solve_profile(*inst)
    st, ps = solver.last_stats, solver.last_profile_stats
    assert np.array_equal(got, want), (name, cut_points, int(np.count_nonzero(pm.unpack(got ^ want, inst[0].size))))
    assert (int(ps.demand), int(ps.capped_positions)) == counters, (name, cut_points)
    assert st.path == 2 and st.spec_boundaries == 0 and st.n_kept == int(pm.unpack(want, inst[0].size).sum())
    form = pm.form_of(st, lengths.size, cut_points)
    if record:
        FORMS.setdefault(form, []).append((name, cut_points))
        NEED_FORMS.setdefault(pm.need_form(int(ps.regions_used)), []).append(name)
        PASSES.setdefault(int(st.sort_passes), []).append(name)
    return st, ps, form


# ------------------------------------------------------------------------------------------ 1. the forms
@pytest.mark.parametrize("cut_points", [-1, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_the_model(solver, name, cut_points):
    st, ps, form = solve_and_check(solver, name, cut_points)
    expected = CASES[name][2]
    if cut_points in expected:
        assert form == expected[cut_points], (name, form, st.as_dict())
    inst = instance(name)[0]
    lengths = inst[3]
    assert st.max_span == int((inst[1].astype(np.int64) - inst[0] + 1)[inst[2] != NO_CONTIG].max())
    if lengths.size >= 256:                                  # no windows: k_profile_cuts keeps fewer than 256 contig starts
        assert st.sweep_stretches == int(np.count_nonzero(lengths)), (name, cut_points)
    if name.startswith("wide keys"):
        assert st.sort_passes == (6 if "six passes" in name else 5) and st.min_span == 1
    if name.startswith("every position a region"):
        assert ps.regions_used == ps.regions_in == int(lengths.sum()) == ps.positions_in_regions


def test_wide_register_cases_sweep_in_stretches_when_cut(solver):
    """cut_points = 1 on 2^23 positions gives hundreds of windows: the K = 1 forms above ran as stretches"""
    name = "wide keys, register form B=8"
    st, _, _ = solve_and_check(solver, name, 1, record=False)
    assert st.sweep_stretches > 64, st.as_dict()


# ------------------------------------------------------------------------------------------ 2. cap and counter edges
def test_largest_cap_beside_the_cut_bit(solver):
    """2^31 - 1 on regions and as default_cap: need[] holds min(cov, cap) below its cut bit 2^31, so the mask is the one
    with any cap above the coverage in its place, and positions under that cap are cut points (cov <= cap)"""
    rng = np.random.default_rng(81)
    L, n = 40_000, 3000
    span = rng.integers(50, 151, size=n)
    s = (rng.random(n) * (L - span + 1)).astype(np.int64)
    e, s = (s + span - 1).astype(np.uint32), s.astype(np.uint32)
    ids, lengths = np.zeros(n, np.uint32), np.array([L], np.uint32)
    edges = np.arange(0, L, 500)
    offs = np.array([0, edges.size], np.uint32)
    r0, r1 = edges.astype(np.uint32), (edges + 399).astype(np.uint32)            # the default shows between regions
    caps = rng.integers(1, 5, size=edges.size).astype(np.uint32)
    caps[::3] = CAP_MAX
    tame = np.where(caps == CAP_MAX, 100_000, caps).astype(np.uint32)
    want = pm.fast_expected_mask(s, e, ids, lengths, 100_000, offs, r0, r1, tame)
    counters = pm.demand_and_capped(s, e, ids, lengths, 100_000, offs, r0, r1, tame)
    assert 0 < pm.unpack(want, n).sum() < n
    for cut_points in (-1, 1):
        with solver.options(cut_points=cut_points):
            got = solver.solve_profile(s, e, ids, lengths, CAP_MAX, offs, r0, r1, caps)
            st, ps = solver.last_stats, solver.last_profile_stats
            assert np.array_equal(got, want), cut_points
            assert (int(ps.demand), int(ps.capped_positions)) == counters
            assert (st.sweep_stretches > 1) == (cut_points == 1), st.as_dict()
            assert np.array_equal(solver.solve_profile(s, e, ids, lengths, 100_000, offs, r0, r1, tame), want)


def test_demand_past_32_bits(solver):
    """11 M reads of 400 bases on 8 contigs of 2^19 positions (depth about 1 050), default_cap 2^20 above every
    coverage, one cap-0 region: the sum of need is 4.4e9 > 2^32 and must come back exact (profile_model.demand_and_capped,
    plain numpy).  The mask is NOT compared with the model bit for bit (the model would take minutes at this size): it
    is checked for validity and kept count through depth_report -- outside the cap-0 region need(p) = cov(p), so no
    position there may be short and every read that reaches out of the region is kept, and the rule never takes a read
    that lies wholly in cap-0 positions -- which here fixes the kept set, so the mask is compared with that set too.
    (Short reads and a deep pile on purpose: 300 000 reads of 16 000 bases reach the same sum on the plain walk, whose
    selection events each scan the last max_span buckets from memory; only the sum matters here.)"""
    rng = np.random.default_rng(82)
    n_contigs, L, span, n = 8, 1 << 19, 400, 11_000_000
    ids = rng.integers(0, n_contigs, size=n).astype(np.uint32)
    s = rng.integers(0, L - span + 1, size=n).astype(np.uint32)
    e = s + np.uint32(span - 1)
    lengths = np.full(n_contigs, L, np.uint32)
    zc, za, zb = 3, 100_000, 100_999
    offs = np.array([0] * (zc + 1) + [1] * (n_contigs - zc), np.uint32)
    r0, r1, caps = np.array([za], np.uint32), np.array([zb], np.uint32), np.array([0], np.uint32)
    default = 1 << 20
    demand, capped = pm.demand_and_capped(s, e, ids, lengths, default, offs, r0, r1, caps)
    assert demand > 1 << 32 and capped == zb - za + 1
    got = solver.solve_profile(s, e, ids, lengths, default, offs, r0, r1, caps)
    ps = solver.last_profile_stats
    assert (int(ps.demand), int(ps.capped_positions)) == (demand, capped)
    inside = (ids == zc) & (s >= za) & (e <= zb)
    assert 0 < inside.sum() < n and solver.last_stats.n_kept == n - int(inside.sum())
    # scope: everything but the cap-0 region
    t_offs = np.array([0] + [c + 1 + (c >= zc) for c in range(n_contigs)], np.uint32)
    t0 = np.array([0] * (zc + 1) + [zb + 1] + [0] * (n_contigs - zc - 1), np.uint32)
    t1 = np.array([L - 1] * zc + [za - 1] + [L - 1] * (n_contigs - zc), np.uint32)
    report = solver.depth_report(s, e, ids, lengths, default, keep_mask=got, target_offsets=t_offs, target_starts=t0,
                                 target_ends=t1)
    assert report.valid and int(report.stats.scope_positions) == n_contigs * L - (zb - za + 1)
    assert int(report.stats.reads_kept) == n - int(inside.sum())
    assert np.array_equal(got, pm.pack(~inside))


# ------------------------------------------------------------------------------------------ 3. two position batches
TWO_BATCH_LENGTHS = [1_200_000_000, 1_150_000_123, 5_000]


@functools.lru_cache(maxsize=None)
def two_batch_instance():
    """a few hundred reads of spans 1..300 in islands at both ends of two long contigs and on a short third, which shares
    the second batch; every contig with a table of its own, the long ones with a region on their first and one on their
    last position"""
    rng = np.random.default_rng(83)
    ss, ee, ii = [], [], []
    offs, r0, r1, caps = [0], [], [], []
    for c, L in enumerate(TWO_BATCH_LENGTHS):
        for a in (0, 4096, L - 1 - 4096, L - 1):
            span = rng.integers(1, 301, size=40)
            span[0], span[1] = 300, 1
            s = np.clip(a - rng.integers(0, span) + rng.integers(-2, 3, size=40), 0, L - span)
            ss.append(s); ee.append(s + span - 1); ii.append(np.full(40, c))
        edges = sorted({0, 1, L - 1, L} | {int(x) for a in (0, 4096, L - 1 - 4096, L) for x in
                                           np.clip(a + rng.integers(-300, 301, size=3 + c), 1, L - 1)})
        edges = edges[:-2] + edges[-1:] if len(edges) % 2 else edges              # [0, 0] ... [.., L - 2] | [L - 1, L - 1]
        rows = [(a, b - 1, int(rng.integers(0, 6))) for a, b in zip(edges[0::2], edges[1::2])]
        rows[0], rows[-1] = (0, 0, 1 + c), (rows[-1][0], L - 1, 2 + c)
        for k in rng.permutation(len(rows)).tolist():
            r0.append(rows[k][0]); r1.append(rows[k][1]); caps.append(rows[k][2])
        offs.append(len(r0))
    s, e, ids = (np.concatenate(x) for x in (ss, ee, ii))
    perm = rng.permutation(s.size)
    u = lambda x: np.asarray(x, np.uint32)
    inst = (u(s[perm]), u(e[perm]), u(ids[perm]), u(TWO_BATCH_LENGTHS), 3, u(offs), u(r0), u(r1), u(caps))
    c = pm.compact(*inst[:4], *inst[5:])
    model = c[:4] + (3,) + c[4:]
    return inst, pm.fast_expected_mask(*model), pm.demand_and_capped(*model)


@pytest.mark.parametrize("cut_points", [1, 0])
def test_second_position_batch_has_regions_of_its_own(solver, cut_points):
    """two contigs of about 1.2e9 positions (one call takes 2^31 - 2) and a short third: the second and third are a
    batch of their own, whose regions batch_cap_table places with first_contig = 1; the model through
    profile_model.compact.  Under stretches (forced, and as the library chooses on such shallow data) only: as one
    chain per contig the two walks over 1.2e9 positions take 13 s on an MI355X, against 0.05 s in stretches and
    0.25 s for test_gpu_by_contig.test_a_genome_past_one_calls_position_limit, the other test of two batches"""
    inst, want, counters = two_batch_instance()
    lengths = inst[3].astype(np.int64)
    assert int(lengths[:2].sum()) > (1 << 31) - 2 >= int(lengths[1:].sum())
    with solver.options(cut_points=cut_points):
        got = solver.solve_profile(*inst)
    st, ps = solver.last_stats, solver.last_profile_stats
    assert np.array_equal(got, want)
    assert (int(ps.demand), int(ps.capped_positions)) == counters
    # two batches: more positions than one takes, every contig counted, and more stretches than one batch's windows
    assert st.total_length == int(lengths.sum()) and st.n_contigs == 3
    assert st.n_reads == inst[0].size and st.n_kept == int(pm.unpack(want, inst[0].size).sum())
    assert st.sweep_stretches > 3840 + 3 and st.max_span == 300 and st.min_span == 1


# ------------------------------------------------------------------------------------------ 4. the device entry
@pytest.mark.parametrize("name", ["wide keys, register form B=6", "10 000 short regions"])
def test_device_entry_aligned_and_one_element_off(pkg, solver, name):
    (s, e, ids, lengths, default, offs, r0, r1, caps), want, counters = instance(name)
    n = s.size
    for shift in (0, 1):
        cols = [_dev(x, shift) for x in (s, e, ids)]
        d_mask = torch.full((pkg.mask_words(n) + 1,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        ptr = [t.data_ptr() + 4 * shift for t in cols]
        assert all(p % 16 == 4 * shift for p in ptr)
        ps = solver.solve_profile_device(ptr[0], ptr[1], ptr[2], n, lengths, default, d_mask.data_ptr(), offs, r0, r1, caps,
                                         stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = d_mask.cpu().numpy().view(np.uint64)
        assert np.array_equal(out[:pkg.mask_words(n)], want) and out[pkg.mask_words(n)] == np.uint64(0xFFFFFFFFFFFFFFFF), shift
        assert (int(ps.demand), int(ps.capped_positions)) == counters, shift


# ------------------------------------------------------------------------------------------ 5. the census
def test_census_every_form_was_taken():
    """every capped instantiation was launched by a case above that passed: five register forms x {K = 1, K = 4} and
    the plain walk x {rings in LDS, in global memory}, each on 32-bit records and on 64-bit keys; both k_profile_need
    forms; 5- and 6-pass sorts"""
    wanted = [(keys, "reg", b, k) for keys in ("rec", "k64") for b in (2, 3, 4, 6, 8) for k in (1, 4)]
    wanted += [(keys, "plain", rings) for keys in ("rec", "k64") for rings in ("lds", "global")]
    missing = [f for f in wanted if f not in FORMS]
    assert not missing, (missing, sorted(FORMS))
    assert set(FORMS) == set(wanted), sorted(FORMS)
    assert {"need_lds", "need_global"} <= set(NEED_FORMS), sorted(NEED_FORMS)
    assert {5, 6} <= set(PASSES), sorted(PASSES)
    print("profile_forms " + "; ".join(f"{f}: {len(c)}" for f, c in sorted(FORMS.items(), key=str)))
