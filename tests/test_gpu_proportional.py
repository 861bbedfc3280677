"""qmcp_hip_solve_proportional_*: keep a fraction of the depth everywhere.  Every mask bit for bit against
tests/proportional_model.py (the canonical rule under need(p) = min(cov(p), M, max(ceil(cov(p) * num / den), floor)))
and every counter of the stats against it: random instances under both cut-point settings, axis tails, the exact
quotient on a staircase of depths, the same need through the profile entry's region table, the plain route at both ends
of the fraction's range, two position batches, argument errors, the device entry, and the cost against the profile call
with the equivalent table."""
import ctypes as C
import functools
import itertools
import json
import os
import statistics
import time

import numpy as np
import pytest
import torch

import profile_model as pm
import proportional_model as qm

pytestmark = pytest.mark.gpu

NO_CONTIG = 0xFFFFFFFF
NO_LIMIT = (1 << 31) - 1
FRACTIONS = [(1, 7), (1, 4), (1, 3), (1, 2), (2, 3), (9, 10), (1048575, 1048576)]
FLOORS = [0, 1, 3]
LIMITS = [1, 5, NO_LIMIT]
COUNTERS = ["reads_placed", "bases_in", "bases_kept", "demand", "whole_positions", "floor_positions", "capped_positions",
            "max_depth", "max_need", "num", "den", "floor", "plain_route"]
# The proportional call's time over the profile call's under the region table that spells the same need out: both are
# the capped route as one chain per contig, and the proportional call builds need[] without a table.  The five per cent
# are the margin DESIGN.md section 4.12 derives for two calls timed in one process (run-to-run spread on both sides of
# the ratio plus the walk-to-pass balance between boxes).
COST_MARGIN = 1.05


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")


def is_plain(num, den, floor, M):
    return num == den or floor >= M or num == 0


def expected_stats(s, e, ids, lengths, num, den, floor, M, mask):
    st = qm.stats(s, e, ids, lengths, num, den, floor, M, mask)
    if is_plain(num, den, floor, M):
        for k in ("demand", "whole_positions", "floor_positions", "capped_positions", "max_depth", "max_need"):
            st[k] = 0
        st["plain_route"] = 1
    return st


def counters_of(ps):
    d = ps.as_dict()
    return {k: int(d[k]) for k in COUNTERS}


def check(solver, s, e, ids, lengths, num, den, floor, M, fast=True, want=None):
    if want is None:
        want = qm.expected_mask(s, e, ids, lengths, num, den, floor, M, fast=fast)
    got = solver.solve_proportional(s, e, ids, lengths, (num, den), floor, M)
    assert np.array_equal(got, want), (num, den, floor, M)
    assert counters_of(solver.last_proportional_stats) == expected_stats(s, e, ids, lengths, num, den, floor, M, want)
    return want


def reads_on(rng, lengths, n, max_span, empty=None, unplaced=0.05):
    """n reads of spans 1..max_span on the contigs (never on `empty`), a few of them unplaced, in random order"""
    lengths = np.asarray(lengths, np.int64)
    live = [c for c in range(lengths.size) if c != empty and lengths[c] > 0]
    ids = rng.choice(live, size=n).astype(np.int64) if live else np.zeros(0, np.int64)
    Ls = lengths[ids]
    span = np.minimum(rng.integers(1, max_span + 1, size=ids.size), Ls)
    s = (rng.random(ids.size) * (Ls - span + 1)).astype(np.int64)
    e = s + span - 1
    ids = ids.astype(np.uint32)
    ids[rng.random(ids.size) < unplaced] = NO_CONTIG
    return s.astype(np.uint32), e.astype(np.uint32), ids


# ------------------------------------------------------------------------------------------ 1. random instances
def test_random_instances_under_both_cut_point_settings(solver):
    """189 instances (every fraction x floor x limit three times): at most 300 reads of spans 1..40 on 1..3 contigs of
    at most 400 positions, one of them without reads, a few reads unplaced; each under cut_points = -1 and 1.  Every
    tenth instance goes through profile_model.select, the others through fast_select (the CPU tests hold the two
    together)"""
    rng = np.random.default_rng(2101)
    combos = list(itertools.product(FRACTIONS, FLOORS, LIMITS)) * 3
    for k, ((num, den), floor, M) in enumerate(combos):
        n_contigs = int(rng.integers(1, 4))
        lengths = rng.integers(1, 401, size=n_contigs).astype(np.uint32)
        empty = int(rng.integers(0, n_contigs)) if n_contigs > 1 else None
        s, e, ids = reads_on(rng, lengths, int(rng.integers(1, 301)), 40, empty)
        want = None
        for cut_points in (-1, 1):
            with solver.options(cut_points=cut_points):
                want = check(solver, s, e, ids, lengths, num, den, floor, M, fast=k % 10 != 0, want=want)
        kept = pm.unpack(want, s.size)
        assert not kept[ids == NO_CONTIG].any()


# ------------------------------------------------------------------------------------------ 2. axis tails
@pytest.mark.parametrize("lengths", [[1], [2], [3], [4], [5], [7], [8], [9], [5, 2, 5], [6, 3, 4], [7, 7, 4], [9, 1, 5]])
def test_axis_tails(solver, lengths):
    """the last positions of the axis go one by one: every length around a group of four, and three contigs whose
    total is 0 .. 3 modulo 4"""
    rng = np.random.default_rng(2102 + sum(lengths) * 7 + len(lengths))
    assert len(lengths) == 1 or sum(lengths) % 4 == [[5, 2, 5], [6, 3, 4], [7, 7, 4], [9, 1, 5]].index(lengths)
    s, e, ids = reads_on(rng, lengths, 40, 6, unplaced=0.0)
    for (num, den), floor, M in (((1, 2), 0, NO_LIMIT), ((1, 3), 1, 5)):
        check(solver, s, e, ids, np.asarray(lengths, np.uint32), num, den, floor, M, fast=False)


# ------------------------------------------------------------------------------------------ 3. arithmetic
@pytest.mark.parametrize("num,den", [(1, 3), (1, 7), (1048575, 1048576), (999983, 1048576)])
def test_quotient_is_exact_on_a_staircase_of_depths(solver, num, den):
    """4 200 reads [0, i] on 4 200 positions: every depth 1 .. 4 200 once, multiples of den next to their successors;
    with 1048575 / 1048576 the product cov * num passes 2^32 (4.40e9), with 999983 / 1048576 -- a prime numerator -- it
    passes 2^31 and ends just below 2^32 (4.20e9): neither fits a signed 32-bit product"""
    L = 4200
    s, e = np.zeros(L, np.uint32), np.arange(L, dtype=np.uint32)
    ids, lengths = np.zeros(L, np.uint32), np.array([L], np.uint32)
    cov, need = qm.need_array(s, e, L, num, den, 0, NO_LIMIT)
    assert sorted(cov.tolist()) == list(range(1, L + 1))
    assert den <= 7 or L * num > 1 << 31
    assert num != 1048575 or L * num > 1 << 32
    want = qm.expected_mask(s, e, ids, lengths, num, den, fast=True)
    got = solver.solve_proportional(s, e, ids, lengths, (num, den))
    ps = solver.last_proportional_stats
    assert int(ps.demand) == int(need.sum()) and int(ps.max_need) == int(need.max()) and int(ps.max_depth) == L
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------ 4. two builders, one need
def test_same_need_through_the_profile_entry(solver):
    rng = np.random.default_rng(2104)
    lengths = np.array([300, 1, 257, 64], np.uint32)
    s, e, ids = reads_on(rng, lengths, 700, 40, empty=1)
    for (num, den), floor, M in (((1, 3), 0, NO_LIMIT), ((2, 3), 3, 5), ((1048575, 1048576), 1, NO_LIMIT)):
        got = solver.solve_proportional(s, e, ids, lengths, (num, den), floor, M)
        demand = int(solver.last_proportional_stats.demand)
        offs, r0, r1, caps = qm.region_table(s, e, ids, lengths, num, den, floor, M)
        same = solver.solve_profile(s, e, ids, lengths, 0, offs, r0, r1, caps)
        assert np.array_equal(got, same)
        assert demand == int(solver.last_profile_stats.demand) > 0


# ------------------------------------------------------------------------------------------ 5. fast ends
def test_both_ends_of_the_range_are_the_plain_call(solver):
    rng = np.random.default_rng(2105)
    lengths = np.array([3000, 500], np.uint32)
    n = 6000
    ids = (rng.random(n) < 0.2).astype(np.uint32)
    s = (rng.random(n) * (lengths[ids].astype(np.int64) - 99)).astype(np.uint32)
    e = s + 99                                                                    # one length: the plain call's fast routes
    ids[::97] = NO_CONTIG
    placed = ids != NO_CONTIG
    for (num, den), floor, M, at in (((5, 5), 0, 7, 7), ((1, 1), 2, 7, 7), ((1, 3), 9, 7, 7), ((1, 3), 7, 7, 7),
                                     ((0, 4), 3, 7, 3), ((0, 1), 9, 7, 7)):
        plain = solver.solve_by_contig(s, e, ids, lengths, at)
        path, kept = solver.last_stats.path, int(solver.last_stats.n_kept)
        got = solver.solve_proportional(s, e, ids, lengths, (num, den), floor, M)
        ps = solver.last_proportional_stats
        assert np.array_equal(got, plain), (num, den, floor, M)
        assert ps.plain_route == 1 and solver.last_stats.path == path and int(solver.last_stats.n_kept) == kept
        assert counters_of(ps) == expected_stats(s, e, ids, lengths, num, den, floor, M, plain)
        assert int(ps.reads_placed) == int(placed.sum()) and int(ps.bases_in) == 100 * int(placed.sum())
        assert int(ps.bases_kept) == 100 * kept
    nothing = solver.solve_proportional(s, e, ids, lengths, (0, 3), 0, 7)
    ps = solver.last_proportional_stats
    assert not nothing.any() and ps.plain_route == 1 and int(ps.bases_kept) == 0
    assert int(ps.reads_placed) == int(placed.sum()) and int(solver.last_stats.n_kept) == 0
    everything = solver.solve_proportional(s, e, ids, lengths, (3, 3))
    assert np.array_equal(pm.unpack(everything, n), placed) and solver.last_proportional_stats.plain_route == 1
    assert int(solver.last_proportional_stats.bases_kept) == 100 * int(placed.sum())


# ------------------------------------------------------------------------------------------ 6. two position batches
TWO_BATCH_LENGTHS = [1_200_000_000, 1_150_000_123, 5_000]


@functools.lru_cache(maxsize=None)
def two_batch_instance():
    """the island shape of test_gpu_profile_forms.two_batch_instance without its tables: 40 reads of spans 1..300 at
    both ends of two long contigs and on a short third, which shares the second batch; the model through
    profile_model.compact"""
    rng = np.random.default_rng(2106)
    ss, ee, ii = [], [], []
    for c, L in enumerate(TWO_BATCH_LENGTHS):
        for a in (0, 4096, L - 1 - 4096, L - 1):
            span = rng.integers(1, 301, size=40)
            span[0], span[1] = 300, 1
            s = np.clip(a - rng.integers(0, span) + rng.integers(-2, 3, size=40), 0, L - span)
            ss.append(s); ee.append(s + span - 1); ii.append(np.full(40, c))
    s, e, ids = (np.concatenate(x) for x in (ss, ee, ii))
    perm = rng.permutation(s.size)
    u = lambda x: np.asarray(x, np.uint32)
    inst = (u(s[perm]), u(e[perm]), u(ids[perm]), u(TWO_BATCH_LENGTHS))
    return inst, pm.compact(*inst)[:4]


@pytest.mark.parametrize("num,den,floor,M", [(1, 3, 1, NO_LIMIT), (2, 3, 0, 5)])
def test_two_position_batches_sum_their_counters(solver, num, den, floor, M):
    """two contigs of about 1.2e9 positions (one call takes 2^31 - 2) and a short third: two batches, whose counters
    add up and whose maxima are taken over both.  Under stretches only (as one chain per contig the walks over 1.2e9
    positions take seconds)"""
    inst, small = two_batch_instance()
    lengths = inst[3].astype(np.int64)
    assert int(lengths[:2].sum()) > (1 << 31) - 2 >= int(lengths[1:].sum())
    want = qm.expected_mask(*small, num, den, floor, M, fast=True)
    with solver.options(cut_points=1):
        got = solver.solve_proportional(*inst, (num, den), floor, M)
    st, ps = solver.last_stats, solver.last_proportional_stats
    assert np.array_equal(got, want)
    assert counters_of(ps) == expected_stats(*small, num, den, floor, M, want)
    assert int(ps.max_depth) == max(int(c.max()) for c, _ in qm.need_arrays(*small, num, den, floor, M))
    assert st.total_length == int(lengths.sum()) and st.n_contigs == 3
    assert st.n_reads == inst[0].size and st.n_kept == int(pm.unpack(want, inst[0].size).sum())


# ------------------------------------------------------------------------------------------ 7. argument errors
def test_errors_are_refused_on_the_host_and_leave_the_mask_alone(pkg, solver):
    s, e = np.array([0, 5], np.uint32), np.array([9, 20], np.uint32)
    ids, lengths = np.zeros(2, np.uint32), np.array([100], np.uint32)
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    cases = [(1, 0, 0, 5, 0, pkg.QMCP_EINVAL),                                    # den == 0
             (3, 2, 0, 5, 0, pkg.QMCP_EINVAL),                                    # num > den
             (1, 2, 0, 5, 1, pkg.QMCP_EINVAL), (1, 2, 0, 5, 1 << 31, pkg.QMCP_EINVAL),   # unknown flag bits
             (1, (1 << 20) + 1, 0, 5, 0, pkg.QMCP_ERANGE),                        # den > 2^20
             (1, 2, 0, 1 << 31, 0, pkg.QMCP_ERANGE), (2, 2, 0, 0xFFFFFFFF, 0, pkg.QMCP_ERANGE)]  # max_coverage >= 2^31
    for num, den, floor, M, flags, code in cases:
        mask = np.full(1, 0xDEADBEEF, np.uint64)
        rc = pkg._hip.qmcp_hip_solve_proportional_host(solver._ctx, p32(s), p32(e), p32(ids), 2, p32(lengths), 1, num, den,
                                                       floor, M, flags, mask.ctypes.data_as(C.POINTER(C.c_uint64)), None,
                                                       None)
        assert rc == code and mask[0] == 0xDEADBEEF, (num, den, M, flags, rc)
    assert pkg._hip.qmcp_hip_solve_proportional_host(solver._ctx, p32(s), p32(e), p32(ids), 2, p32(lengths), 1, 1 << 20,
                                                     1 << 20, 0, NO_LIMIT, 0, mask.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                     None, None) == pkg.QMCP_OK    # the limits themselves are fine
    d_mask = torch.full((1,), 0x5EED, dtype=torch.int64, device="cuda:0")
    ds, de, di = _dev(s), _dev(e), _dev(ids)
    torch.cuda.synchronize()
    for proportion, M, code in (((1, (1 << 20) + 1), 5, pkg.QMCP_ERANGE), ((1, 2), 1 << 31, pkg.QMCP_ERANGE)):
        with pytest.raises(pkg.QmcpError) as ex:
            solver.solve_proportional_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), 2, lengths, proportion,
                                             d_mask.data_ptr(), 0, M)
        torch.cuda.synchronize()
        assert ex.value.code == code and int(d_mask.cpu()[0]) == 0x5EED
    with pytest.raises(pkg.QmcpError) as ex:                                      # found on the device, mask cleared
        solver.solve_proportional(np.array([5], np.uint32), np.array([100], np.uint32), np.zeros(1, np.uint32), lengths, 0.5)
    assert ex.value.code == pkg.QMCP_EREAD


# ------------------------------------------------------------------------------------------ 8. the device entry
def test_device_entry_equals_host_entry(pkg, solver):
    rng = np.random.default_rng(2108)
    lengths = np.array([500, 333], np.uint32)
    s, e, ids = reads_on(rng, lengths, 999, 60)
    want = solver.solve_proportional(s, e, ids, lengths, 0.25, 1, 9)
    host = counters_of(solver.last_proportional_stats)
    assert (host["num"], host["den"]) == (1, 4) and host["plain_route"] == 0
    n = s.size
    ds, de, di = _dev(s), _dev(e), _dev(ids)
    d_mask = torch.full((max(pkg.mask_words(n), 1),), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ps = solver.solve_proportional_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, 0.25, d_mask.data_ptr(),
                                          1, 9)
    torch.cuda.synchronize()
    assert np.array_equal(d_mask.cpu().numpy().view(np.uint64)[:pkg.mask_words(n)], want)
    assert counters_of(ps) == host
    assert np.array_equal(want, qm.expected_mask(s, e, ids, lengths, 1, 4, 1, 9, fast=True))


# ------------------------------------------------------------------------------------------ 9. cost
def test_costs_no_more_than_the_profile_call_with_the_equivalent_table(pkg, solver):
    """the generator of test_gpu_profile's cost test at 2^21 reads: two spans (100 and 150) on 8 contigs, shuffled, under
    near_uniform = -1, speculation = -1 and cut_points = -1; f = 1/2, no floor, no limit, against solve_profile_device
    under the region table that spells the same need out (default cap 0).  Wall time of the whole device call, medians
    of 5 after a warm-up; the reads are halved while one call takes more than about a second.
    QMCP_PROPORTIONAL_TIME_OUT=<file> keeps the figures."""
    n_contigs, L = 8, 500_000
    num, den = 1, 2
    lengths = np.full(n_contigs, L, np.uint32)
    n = 1 << 21

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    with solver.options(near_uniform=-1, speculation=-1, cut_points=-1):
        while True:
            rng = np.random.default_rng(79)
            ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), n // n_contigs)
            span = np.where(rng.random(n) < 0.5, 100, 150).astype(np.int64)
            s = (rng.random(n) * (L - span + 1)).astype(np.int64)
            e = s + span - 1
            perm = rng.permutation(n)
            s, e, ids = s[perm], e[perm], ids[perm]
            offs, r0, r1, caps = [0], [], [], []
            for c in range(n_contigs):                                           # the need in exact 64-bit integers
                cov = pm.coverage(s[ids == c], e[ids == c], L)
                _, a, b, cap = pm.regions_of((cov * num + den - 1) // den)
                r0.append(a); r1.append(b); caps.append(cap); offs.append(offs[-1] + a.size)
            offs, r0, r1, caps = np.asarray(offs, np.uint32), np.concatenate(r0), np.concatenate(r1), np.concatenate(caps)
            ds, de, di = _dev(s), _dev(e), _dev(ids)
            d_prop = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device="cuda:0")
            d_prof = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device="cuda:0")
            prop = lambda: solver.solve_proportional_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths,
                                                            (num, den), d_prop.data_ptr())
            prof = lambda: solver.solve_profile_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, 0,
                                                       d_prof.data_ptr(), offs, r0, r1, caps)
            prof(); prop()                                                       # warm-up: arena growth
            if max(timed(prof), timed(prop)) <= 1000.0 or n <= 1 << 16:
                break
            n //= 2
        assert solver.last_stats.path == 2 and solver.last_proportional_stats.plain_route == 0
        t_prof, t_prop, ms_need, ms_tally = [], [], [], []
        for _ in range(5):
            t_prof.append(timed(prof))
            demand = int(solver.last_profile_stats.demand)
            t_prop.append(timed(prop))
            ps = solver.last_proportional_stats
            ms_need.append(float(ps.ms_need)); ms_tally.append(float(ps.ms_tally))
    assert torch.equal(d_prop, d_prof) and int(ps.demand) == demand > 0
    a, b = statistics.median(t_prof), statistics.median(t_prop)
    figures = {"reads": n, "contigs": n_contigs, "positions": int(n_contigs * L), "fraction": [num, den], "floor": 0,
               "max_coverage": NO_LIMIT, "regions": int(r0.size), "max_depth": int(ps.max_depth),
               "profile_ms_median": round(a, 3), "profile_ms_runs": [round(x, 3) for x in t_prof],
               "proportional_ms_median": round(b, 3), "proportional_ms_runs": [round(x, 3) for x in t_prop],
               "ms_need_median": round(statistics.median(ms_need), 4),
               "ms_tally_median": round(statistics.median(ms_tally), 4), "ratio": round(b / a, 4), "margin": COST_MARGIN}
    print("proportional_time " + json.dumps(figures))
    out = os.environ.get("QMCP_PROPORTIONAL_TIME_OUT")
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(figures, indent=1) + "\n")
    assert b <= COST_MARGIN * a, figures
