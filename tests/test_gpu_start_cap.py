"""qmcp_hip_solve_start_cap_*: every (contig, start, group) cell reduced to its best K reads before the by-contig solve.
Keep mask, capped mask, statistics (the shortfall included) and cell-size histogram are compared bit for bit with the
literal model on the oracle (tests/start_cap_model.py), through the host entry and through the device entry."""
import ctypes as C

import numpy as np
import pytest

import multi_reference as mr
import start_cap_model as sm

pytestmark = pytest.mark.gpu

BINS = 8


def check(solver, oracle, s, e, ids, lengths, M, K, groups=None, prio=None, shortfall=True, bins=BINS, by_contig=None,
          what=""):
    """the host entry against the model; -> (keep bits, capped bits, stats dict of the entry)"""
    mask, capped, st, hist = solver.solve_start_cap(s, e, ids, lengths, M, K, groups=groups, priorities=prio,
                                                    shortfall=shortfall, hist_bins=bins)
    keep_w, cap_w, st_w, hist_w = sm.start_cap(oracle, s, e, ids, lengths, M, K, groups=groups, priorities=prio,
                                               shortfall=shortfall, hist_bins=bins, by_contig=by_contig)
    n = len(s)
    assert mask.size == capped.size == (n + 63) // 64
    assert np.array_equal(capped, sm.pack(cap_w)), f"{what}: capped mask"
    assert {k: st[k] for k in sm.STAT_KEYS} == st_w, f"{what}: stats"
    assert np.array_equal(hist, hist_w), f"{what}: histogram {hist} != {hist_w}"
    assert np.array_equal(mask, sm.pack(keep_w)), f"{what}: keep mask"
    assert not (mask & capped).any()
    assert st["cap"] == min(K, 0xFFFFFFFF) and st["largest_kept_cell"] <= K
    assert solver.last_stats.n_kept == keep_w.sum()
    return keep_w, cap_w, st


def piled_reads(rng, n, lengths, n_sites=40, unplaced=0.05, max_span=40):
    """n reads that start on at most n_sites sites over the contigs, every read with a span of its own, a few unplaced"""
    lengths = np.asarray(lengths, np.uint32)
    site_ids = rng.integers(0, lengths.size, size=n_sites)
    site_s = (rng.random(n_sites) * (lengths[site_ids] - max_span)).astype(np.int64)
    pick = rng.integers(0, n_sites, size=n)
    span = rng.integers(1, max_span + 1, size=n)
    ids = np.where(rng.random(n) < unplaced, mr.NO_CONTIG, site_ids[pick])
    return site_s[pick].astype(np.uint32), (site_s[pick] + span - 1).astype(np.uint32), ids.astype(np.uint32)


def kept_per_cell(keep, s, ids, groups=None):
    g = np.zeros(len(s), np.int64) if groups is None else np.asarray(groups, np.int64)
    on = np.flatnonzero(keep)
    if on.size == 0:
        return np.zeros(0, np.int64)
    rows = np.stack([np.asarray(ids, np.int64)[on], np.asarray(s, np.int64)[on], g[on]], axis=1)
    return np.unique(rows, axis=0, return_counts=True)[1]


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4095, 4097, 8191, 8193])
def test_sizes_across_word_wave_and_tile_edges(solver, oracle, n, K):
    rng = np.random.default_rng(100 + n)
    lengths = [700, 400]
    s, e, ids = piled_reads(rng, n, lengths)
    groups = rng.integers(0, 2, size=n).astype(np.uint32)
    prio = rng.integers(0, 4, size=n).astype(np.uint32)        # (ties in priority inside every cell)
    keep, _, st = check(solver, oracle, s, e, ids, lengths, 3, K, groups=groups, prio=prio, what=f"n={n} K={K}")
    counts = kept_per_cell(keep, s, ids, groups)
    assert counts.size == st["cells_kept"] and (counts <= K).all()          # promise (1), from the mask alone
    if n > 200:
        assert st["reads_capped"] > n // 2 and st["key_bits"] <= 32 and st["sort_passes"] == (st["key_bits"] + 7) // 8
        assert st["key_bits"] == sm.key_bits(s, e, ids, lengths, groups, prio)


@pytest.mark.parametrize("K", [1, 5, 20_000, 1 << 31])
def test_one_cell_holds_every_read(solver, oracle, K):
    n = 20_000
    rng = np.random.default_rng(3)
    s, ids = np.full(n, 17, np.uint32), np.zeros(n, np.uint32)
    e = (s + rng.integers(10, 60, size=n)).astype(np.uint32)
    prio = rng.integers(0, 3, size=n).astype(np.uint32)
    _, capped, st = check(solver, oracle, s, e, ids, [100], 5, K, prio=prio)
    assert st["cells"] == 1 and st["largest_cell"] == n and st["reads_survived"] == min(K, n)
    best = np.lexsort((np.arange(n), -(e.astype(np.int64) - s), -prio.astype(np.int64)))[:min(K, n)]
    assert np.array_equal(np.flatnonzero(~capped), np.sort(best))
    # no priorities: the K longest, then the lowest indices
    _, capped, st = check(solver, oracle, s, e, ids, [100], 5, K)
    longest = np.lexsort((np.arange(n), -(e.astype(np.int64) - s)))[:min(K, n)]
    assert np.array_equal(np.flatnonzero(~capped), np.sort(longest))
    assert st["key_bits"] == 6 + 7 and st["sort_passes"] == 2


def test_cells_straddle_the_sort_tile_edges(solver, oracle):
    """one read per start, except that the cells at sorted positions 4 093 and 8 189 hold six reads each: both cells lie
    across a sort tile's (4 096) and a scan tile's edge"""
    rng = np.random.default_rng(9)
    sizes = np.ones(9000, dtype=np.int64)
    sizes[4093] = 6
    sizes[8189 - 5] = 6                                       # (sorted position = reads of the cells before it)
    starts = np.repeat(np.arange(sizes.size), sizes)
    assert starts[4093] == starts[4098] == 4093 and starts[8189] == starts[8194] != starts[8188] and starts[8195] != starts[8194]
    perm = rng.permutation(starts.size)
    s = starts[perm].astype(np.uint32)
    e = (s + rng.integers(20, 40, size=s.size)).astype(np.uint32)
    prio = rng.integers(0, 3, size=s.size).astype(np.uint32)
    _, capped, st = check(solver, oracle, s, e, np.zeros(s.size, np.uint32), [9100], 4, 2, prio=prio)
    assert st["cells"] == 9000 and st["largest_cell"] == 6 and st["reads_capped"] == 8 and st["cells_over_cap"] == 2
    assert sorted(s[capped].tolist()) == [4093] * 4 + [8184] * 4


def test_one_cell_spans_two_whole_tiles(solver, oracle):
    rng = np.random.default_rng(10)
    starts = np.concatenate([np.arange(3000), np.full(10_000, 3000), np.arange(3001, 4000)])
    perm = rng.permutation(starts.size)
    s = starts[perm].astype(np.uint32)
    e = (s + rng.integers(20, 40, size=s.size)).astype(np.uint32)
    _, _, st = check(solver, oracle, s, e, np.zeros(s.size, np.uint32), [4100], 6, 4097)
    assert st["largest_cell"] == 10_000 and st["reads_capped"] == 10_000 - 4097 and st["cells_over_cap"] == 1


def test_groups(solver, oracle):
    rng = np.random.default_rng(11)
    lengths = [600, 300]
    s, e, ids = piled_reads(rng, 3000, lengths, n_sites=30)
    prio = rng.integers(0, 61, size=s.size).astype(np.uint32)
    groups = rng.integers(0, 2, size=s.size).astype(np.uint32)
    # two groups on the same starts each keep their own K: the survivors are those of the two groups taken alone
    _, capped, st = check(solver, oracle, s, e, ids, lengths, 4, 2, groups=groups, prio=prio)
    placed = ids != mr.NO_CONTIG
    for g in (0, 1):
        on = np.flatnonzero(groups == g)
        alone = solver.solve_start_cap(s[on], e[on], ids[on], lengths, 4, 2, priorities=prio[on])[1]
        assert np.array_equal(sm.unpack(alone, on.size), capped[on])
    assert (np.unique(np.stack([ids, s, groups], 1)[placed & ~capped], axis=0, return_counts=True)[1] <= 2).all()
    # groups=None equals one constant group, whatever its value
    a = solver.solve_start_cap(s, e, ids, lengths, 4, 2, priorities=prio, shortfall=True, hist_bins=BINS)
    b = solver.solve_start_cap(s, e, ids, lengths, 4, 2, groups=np.full(s.size, 0xDEADBEEF, np.uint32), priorities=prio,
                               shortfall=True, hist_bins=BINS)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert {k: a[2][k] for k in sm.STAT_KEYS + ("key_bits",)} == {k: b[2][k] for k in sm.STAT_KEYS + ("key_bits",)}
    # a large offset costs nothing: group - group_min
    far = (groups + np.uint32(0xFFFFFFF0)).astype(np.uint32)
    c = solver.solve_start_cap(s, e, ids, lengths, 4, 2, groups=far, priorities=prio)
    d = solver.solve_start_cap(s, e, ids, lengths, 4, 2, groups=groups, priorities=prio)
    assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1]) and c[2]["key_bits"] == d[2]["key_bits"]
    check(solver, oracle, s, e, ids, lengths, 4, 2, groups=far, prio=prio)


def test_order_priority_beats_span_beats_index(solver, oracle):
    # one cell of six reads: (priority, span) = (1, 9), (2, 3), (2, 5), (2, 5), (0, 30), (1, 9)
    s = np.full(6, 10, np.uint32)
    prio = np.array([1, 2, 2, 2, 0, 1], np.uint32)
    e = (s + np.array([9, 3, 5, 5, 30, 9])).astype(np.uint32)
    ids = np.zeros(6, np.uint32)
    for K, want in ((1, [2]), (2, [2, 3]), (3, [1, 2, 3]), (4, [0, 1, 2, 3]), (5, [0, 1, 2, 3, 5]), (6, list(range(6)))):
        _, capped, _ = check(solver, oracle, s, e, ids, [100], 6, K, prio=prio)
        assert np.flatnonzero(~capped).tolist() == want
    # a permuted input has the same survivors as a multiset of (start, end, group, priority)
    rng = np.random.default_rng(12)
    lengths = [500, 300]
    s, e, ids = piled_reads(rng, 4000, lengths, n_sites=25, max_span=12)
    groups = rng.integers(0, 3, size=s.size).astype(np.uint32)
    prio = rng.integers(0, 4, size=s.size).astype(np.uint32)
    rows = np.stack([ids, s, e, groups, prio], axis=1).astype(np.int64)
    _, capped, _ = check(solver, oracle, s, e, ids, lengths, 5, 3, groups=groups, prio=prio)
    perm = rng.permutation(s.size)
    _, capped2, _ = check(solver, oracle, s[perm], e[perm], ids[perm], lengths, 5, 3, groups=groups[perm], prio=prio[perm])
    placed = ids != mr.NO_CONTIG
    canon = lambda r: r[np.lexsort(r.T[::-1])]
    assert np.array_equal(canon(rows[placed & ~capped]), canon(rows[perm][placed[perm] & ~capped2]))


def test_two_contigs_with_equal_starts_are_different_cells(solver, oracle):
    rng = np.random.default_rng(13)
    n = 600
    s = rng.integers(0, 10, size=n).astype(np.uint32)
    e = (s + rng.integers(5, 30, size=n)).astype(np.uint32)
    ids = rng.integers(0, 2, size=n).astype(np.uint32)
    _, capped, st = check(solver, oracle, s, e, ids, [50, 50], 4, 2)
    assert st["cells"] == 20 and st["reads_survived"] == 40 and st["reads_capped"] == n - 40


def test_no_cell_over_the_cap_is_solve_by_contig_bit_for_bit(solver, oracle):
    rng = np.random.default_rng(14)
    s, e, ids, lengths = mr.random_by_contig(rng, 3, max_reads_per_contig=2000)
    K = int(sm.cells_and_ranks(s, e, ids)[3].max())
    for M in (1, 7, 40):
        plain = solver.solve_by_contig(s, e, ids, lengths, M)
        mask, capped, st, _ = solver.solve_start_cap(s, e, ids, lengths, M, K, shortfall=True)
        assert np.array_equal(mask, plain) and not capped.any()
        assert st["cells_over_cap"] == st["reads_capped"] == st["short_positions"] == st["short_bases"] == 0
    check(solver, oracle, s, e, ids, lengths, 7, K)
    # with groups that make every read's cell its own, K = 1 caps nothing either
    own = rng.permutation(s.size).astype(np.uint32)
    mask, capped, st, _ = solver.solve_start_cap(s, e, ids, lengths, 7, 1, groups=own, shortfall=True)
    assert np.array_equal(mask, solver.solve_by_contig(s, e, ids, lengths, 7)) and not capped.any()
    assert st["short_positions"] == 0 and st["cells"] == st["reads_placed"]


def test_one_span_and_a_cap_of_one_is_dedup_read_mode(solver, oracle):
    rng = np.random.default_rng(15)
    lengths = [900, 500]
    s, _, ids = piled_reads(rng, 5000, lengths, n_sites=300, max_span=50)
    e = (s + 49).astype(np.uint32)
    prio = rng.integers(0, 5, size=s.size).astype(np.uint32)
    for q in (prio, None):
        want = solver.solve_dedup(s, e, ids, lengths, 3, qualities=q)
        got = solver.solve_start_cap(s, e, ids, lengths, 3, 1, priorities=q)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert got[2]["cells"] == want[2]["families"] and got[2]["reads_capped"] == want[2]["duplicate_units"]
    check(solver, oracle, s, e, ids, lengths, 3, 1, prio=prio)


def test_two_runs_give_equal_masks(solver, oracle):
    rng = np.random.default_rng(16)
    lengths = [700, 400]
    s, e, ids = piled_reads(rng, 9000, lengths)
    prio = rng.integers(0, 2, size=s.size).astype(np.uint32)
    a = solver.solve_start_cap(s, e, ids, lengths, 5, 3, priorities=prio, shortfall=True, hist_bins=BINS)
    b = solver.solve_start_cap(s, e, ids, lengths, 5, 3, priorities=prio, shortfall=True, hist_bins=BINS)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert {k: a[2][k] for k in sm.STAT_KEYS} == {k: b[2][k] for k in sm.STAT_KEYS}


def deep_reads(rng, L, length, per_start, shorten=0.0):
    """per_start reads (on average) on every start of [0, L - length], `shorten` of them cut to a third .. all of it"""
    n = int((L - length + 1) * per_start)
    s = rng.integers(0, L - length + 1, size=n)
    span = np.where(rng.random(n) < shorten, rng.integers(length // 3, length, size=n), length)
    return s.astype(np.uint32), (s + span - 1).astype(np.uint32)


@pytest.mark.parametrize("K", [1, 2, 4])
def test_mixed_lengths_deep_and_shallow(solver, oracle, K):
    rng = np.random.default_rng(17)
    # 30 % shorter reads at 5 x M on two contigs: the inner solve takes a mixed-span route
    M = 20
    s0, e0 = deep_reads(rng, 4000, 100, 1.0, shorten=0.3)
    s1, e1 = deep_reads(rng, 2500, 100, 1.0, shorten=0.3)
    s, e = np.concatenate([s0, s1]), np.concatenate([e0, e1])
    ids = np.concatenate([np.zeros(s0.size, np.uint32), np.ones(s1.size, np.uint32)])
    perm = rng.permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    _, _, st = check(solver, oracle, s, e, ids, [4000, 2500], M, K, what="deep")
    assert st["cells_over_cap"] > 0
    # a shallow input with cut points (stretches no read covers)
    s, e = deep_reads(rng, 6000, 60, 0.2, shorten=0.3)
    hole = (s > 2000) & (s < 2100) | (s > 4000) & (s < 4200)
    s, e = s[~hole], e[~hole]
    check(solver, oracle, s, e, np.zeros(s.size, np.uint32), [6000], 8, K, what="shallow")


def raw_host(pkg, solver, s, e, ids, groups, prio, lengths, M, K, flags, mask, capped, hist, bins):
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    p64 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint64))
    return pkg._hip.qmcp_hip_solve_start_cap_host(solver._ctx, p(s), p(e), p(ids), p(groups), p(prio), s.size, p(lengths),
                                                  lengths.size, M, K, flags, p64(mask), p64(capped), p64(hist), bins,
                                                  None, None)


def test_priority_range_and_errors_leave_the_outputs_untouched(pkg, solver, oracle):
    rng = np.random.default_rng(18)
    lengths = [500, 300]
    s, e, ids = piled_reads(rng, 1000, lengths, n_sites=30)
    placed = np.flatnonzero(ids != mr.NO_CONTIG)
    prio = rng.integers(100, 2000, size=s.size).astype(np.uint32)
    prio[placed[3]], prio[placed[7]] = 100, 100 + 65535
    prio[ids == mr.NO_CONTIG] = 0xFFFFFFF0                      # (unplaced reads do not count towards the range)
    check(solver, oracle, s, e, ids, lengths, 3, 2, prio=prio, what="range 65535")
    guard = np.uint64(0xA5A5A5A5A5A5A5A5)
    words = (s.size + 63) // 64

    def refused(code, word, s=s, e=e, ids=ids, prio=prio, K=2, flags=0, lengths=lengths, bins=BINS, no_hist=False):
        mask, capped, hist = (np.full(words + 2, guard, np.uint64) for _ in range(3))
        rc = raw_host(pkg, solver, s, e, ids, None, prio, lengths, 3, K, flags, mask, capped, None if no_hist else hist,
                      bins)
        assert rc == code, (rc, pkg._hip.qmcp_hip_last_error())
        assert word in pkg._hip.qmcp_hip_last_error().decode(), pkg._hip.qmcp_hip_last_error()
        assert (mask == guard).all() and (capped == guard).all() and (hist == guard).all()

    p2 = prio.copy()
    p2[placed[7]] += 1
    refused(pkg.QMCP_ERANGE, "65535", prio=p2)
    refused(pkg.QMCP_EINVAL, "cap", K=0)
    refused(pkg.QMCP_EINVAL, "flag", flags=2)
    refused(pkg.QMCP_EINVAL, "hist_out", no_hist=True)          # bins without a histogram buffer
    refused(pkg.QMCP_ERANGE, "hist_bins", bins=4097)            # (refused before a bin is written)
    # a bad read inside a capped read: the worst of a cell ends past its contig
    order, cell, rank, sizes = sm.cells_and_ranks(s, e, ids, None, prio)
    i = int(order[np.flatnonzero(rank >= 2)[0]])
    e2 = e.copy()
    e2[i] = lengths[int(ids[i])]
    refused(pkg.QMCP_EREAD, "read", e=e2)
    s2 = s.copy()
    s2[i] = e[i] + 1
    refused(pkg.QMCP_EREAD, "start > end", s=s2)
    ids2 = ids.copy()
    ids2[i] = 2
    refused(pkg.QMCP_EINVAL, "contig id", ids=ids2)
    with pytest.raises(pkg.QmcpError, match="null buffer"):
        pkg._check(pkg._hip.qmcp_hip_solve_start_cap_host(solver._ctx, None, None, None, None, None, 5, None, 1, 3, 2, 0,
                                                          None, None, None, 0, None, None))
    check(solver, oracle, s, e, ids, lengths, 3, 2, prio=prio, what="after the refusals")


def test_wide_keys_and_the_sort_field_by_field(solver, oracle):
    """two contigs of 2^27 positions: gstart takes 29 bits.  Groups over 20 bits force the split 64-bit key; groups over
    the full uint32 range with 6 bits of priority and 4 of span go beyond 64 bits: one sort per field, and the cells are
    found on the columns.  The oracle does not take 2^28 positions, so the model's inner solve is the by-contig entry."""
    inner = solver.solve_by_contig
    for g_hi, bits, passes in (((1 << 20) - 1, 29 + 20 + 6 + 4, 8), ((1 << 32) - 1, 29 + 32 + 6 + 4, 4 + 4 + 1 + 1)):
        rng = np.random.default_rng(19)
        lengths = [1 << 27, 1 << 27]
        n, n_sites = 4096, 300
        site_ids = rng.integers(0, 2, size=n_sites)
        site_s = rng.integers(0, (1 << 27) - 100, size=n_sites)
        site_s[:4] = (1 << 27) - 40                             # gstart's top bits in use on both contigs
        pick = rng.integers(0, n_sites, size=n)
        s = site_s[pick].astype(np.uint32)
        span = rng.integers(20, 36, size=n)
        span[:2] = [20, 35]
        e = (s + span - 1).astype(np.uint32)
        groups = rng.choice(np.array([0, 1, g_hi // 3, g_hi], dtype=np.uint64), size=n).astype(np.uint32)
        groups[:2] = [0, g_hi]
        ids = site_ids[pick].astype(np.uint32)
        ids[2:] = np.where(rng.random(n - 2) < 0.03, mr.NO_CONTIG, ids[2:])
        prio = rng.integers(0, 61, size=n).astype(np.uint32)
        prio[:2] = [0, 60]
        _, _, st = check(solver, oracle, s, e, ids, lengths, 2, 2, groups=groups, prio=prio, shortfall=False,
                         by_contig=inner, what=f"{bits} bits")
        assert st["key_bits"] == bits and st["sort_passes"] == passes and st["cells_over_cap"] > 0
        # the ends are no part of a cell: with every group 0 the cells are the sites
        _, _, st = check(solver, oracle, s, e, ids, lengths, 2, 2, prio=prio, shortfall=False, by_contig=inner)
        assert st["cells"] <= n_sites


def test_device_entry_equals_the_host_entry_at_any_alignment(pkg, solver, oracle):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(20)
    lengths = [700, 400]
    n = 5000
    s, e, ids = piled_reads(rng, n, lengths)
    groups = rng.integers(0, 3, size=n).astype(np.uint32)
    prio = rng.integers(0, 61, size=n).astype(np.uint32)
    words = pkg.mask_words(n)
    guard = -0x0123456789ABCDEF
    keep_w, cap_w, st_w, hist_w = sm.start_cap(oracle, s, e, ids, lengths, 3, 2, groups=groups, priorities=prio,
                                               shortfall=True, hist_bins=BINS)
    for shift in (0, 1):
        cols = []
        for x in (s, e, ids, groups, prio):
            t = torch.zeros(n + shift + 4, dtype=torch.int32, device=dev)   # (a base allocation is 256-byte aligned)
            t[shift:shift + n] = torch.from_numpy(x.view(np.int32)).to(dev)
            cols.append(t)
        d_mask = torch.full((words + 3,), guard, dtype=torch.int64, device=dev)
        d_cap = torch.full((words + 3,), guard, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ptr = [t.data_ptr() + 4 * shift for t in cols]
        assert all(p % 16 == 4 * shift for p in ptr)
        st, hist = solver.solve_start_cap_device(ptr[0], ptr[1], ptr[2], n, lengths, 3, 2, d_mask.data_ptr(),
                                                 d_groups=ptr[3], d_priorities=ptr[4], shortfall=True,
                                                 d_capped_mask=d_cap.data_ptr(), hist_bins=BINS,
                                                 stream=torch.cuda.current_stream().cuda_stream)
        got, got_cap = d_mask.cpu().numpy(), d_cap.cpu().numpy()
        assert np.array_equal(got[:words].view(np.uint64), sm.pack(keep_w)), shift
        assert np.array_equal(got_cap[:words].view(np.uint64), sm.pack(cap_w)), shift
        assert (got[words:] == guard).all() and (got_cap[words:] == guard).all()
        assert {k: st[k] for k in sm.STAT_KEYS} == st_w and np.array_equal(hist, hist_w)
    # no groups, no priorities, no capped mask
    d_mask = torch.full((words + 3,), guard, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    st, _ = solver.solve_start_cap_device(ptr[0], ptr[1], ptr[2], n, lengths, 3, 2, d_mask.data_ptr())
    want = sm.start_cap(oracle, s, e, ids, lengths, 3, 2)
    assert np.array_equal(d_mask.cpu().numpy()[:words].view(np.uint64), sm.pack(want[0]))
    assert st["short_positions"] == 0 and st["reads_capped"] == want[2]["reads_capped"]


def test_random_stress(solver, oracle):
    for seed in range(120):
        rng = np.random.default_rng(7000 + seed)
        n_contigs = int(rng.integers(1, 4))
        lengths = rng.integers(60, 3000, size=n_contigs).astype(np.uint32)
        n = int(rng.integers(0, 3001))
        s, e, ids = piled_reads(rng, n, lengths, n_sites=int(rng.integers(1, 400)), unplaced=float(rng.random() * 0.2))
        groups = None if rng.random() < 0.3 else rng.integers(0, int(rng.choice([2, 5, 1 << 20])), size=n).astype(np.uint32)
        prio = None if rng.random() < 0.3 else rng.integers(0, int(rng.choice([2, 61, 60000])), size=n).astype(np.uint32)
        check(solver, oracle, s, e, ids, lengths, int(rng.choice([1, 2, 5, 30])), int(rng.choice([1, 2, 3, 8, 1000])),
              groups=groups, prio=prio, shortfall=bool(seed % 2), bins=int(rng.choice([0, 1, 4, 64])), what=f"seed {seed}")
