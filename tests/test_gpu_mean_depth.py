"""qmcp_hip_solve_mean_depth_*: the deepest coverage whose by-contig solve keeps at most a number of bases inside a region
set.  Every expected value comes from the CPU oracle and numpy (tests/mean_depth_model.py): bases(M) from the oracle's
mask and a membership array painted from the raw regions, M* from brute force over every coverage (or the model's
bisection where 0 .. top is long), the curve from the definition."""
import os

import numpy as np
import pytest

import bam_py
import budget_model as bm
import mean_depth_model as mm
import multi_reference as mr
from forcing import forced

pytestmark = pytest.mark.gpu

NO_CONTIG = mr.NO_CONTIG
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("budget", "positions", "reads_placed", "n_kept", "kept_bases", "bases_above", "bound_above", "total_bases",
          "coverage", "max_depth", "top", "probes", "curve_entries", "saturated", "regions_in", "regions_used")


def popcount(mask):
    return int(np.unpackbits(np.ascontiguousarray(mask).view(np.uint8)).sum())


def launches(solver, name):
    return solver.kernel_times().get(name, (0, 0.0))[0]


def merged_regions(model):
    """the maximal runs of region positions, contig by contig (regions that touch or overlap are one)"""
    runs, at = 0, 0
    for length in model.lengths.astype(np.int64).tolist():
        m = model.inside[at:at + length].astype(np.int8)
        runs += int(np.count_nonzero(np.diff(np.concatenate([[0], m])) == 1))
        at += length
    return runs


def table_args(regions):
    return {} if regions is None else dict(region_offsets=regions[0], region_starts=regions[1], region_ends=regions[2])


def check_answer(model, budget, got, M, ms, curve=None, regions=None):
    """one call's mask, coverage and statistics against the model"""
    where = (budget, M, ms.as_dict())
    assert M == ms.coverage and ms.budget == budget and ms.top == model.top, where
    assert ms.reads_placed == model.placed and ms.max_depth == model.max_depth, where
    assert ms.total_bases == model.total_bases and ms.positions == model.positions, where
    assert np.array_equal(got, model.mask(M)), where                              # bit for bit the solve at M*
    assert ms.n_kept == popcount(got) == model.count(M), where
    assert ms.kept_bases == model.bases(M) <= budget, where                       # (1)
    if M < model.top:
        above = model.bases(M + 1)
        bound = int(np.minimum(model.cov[model.inside], min(M + 1, mm.CURVE_MAX)).sum())
        assert above > budget, where                                              # (2)
        assert (ms.bases_above, ms.bound_above) in ((above, 0), (0, bound)), (where, above, bound)
        assert ms.bases_above > budget or ms.bound_above > budget, where          # one of the two ruled M* + 1 out
    else:
        assert ms.bases_above == 0 and ms.bound_above == 0, where
    assert ms.probes <= bm.probe_limit(model.top), where
    assert ms.saturated == (1 if ms.n_kept == model.placed else 0), where
    if regions is None:
        assert ms.regions_in == 0 and ms.regions_used == 0, where
    else:
        assert ms.regions_in == int(regions[0][-1]) and ms.regions_used == merged_regions(model), where
    if curve is not None:
        assert ms.curve_entries == curve.size and np.array_equal(curve, model.curve_R()), where


def report_sum(solver, s, e, ids, lengths, mask, regions):
    """the independent device check: the kept depth inside the regions as the depth report sums it"""
    if regions is None:
        return int(solver.depth_report(s, e, ids, lengths, 1, keep_mask=mask).contig_rows["sum_kept"].sum())
    rep = solver.depth_report(s, e, ids, lengths, 1, keep_mask=mask, target_offsets=regions[0], target_starts=regions[1],
                              target_ends=regions[2])
    return int(rep.region_rows["sum_kept"].sum())


# ------------------------------------------------------------------------------------------ 1: mixed spans
@pytest.fixture(scope="module")
def mixed(oracle):
    """random_by_contig(rng, 4, 2500), seeds 0 .. 5, the regions of test_mean_depth_cpu.py; the models are made on demand
    and kept (the oracle's masks are cached in them)"""
    data, models = [], {}
    for seed in range(6):
        s, e, ids, lengths = mr.random_by_contig(np.random.default_rng(seed), 4, 2500)
        data.append((s, e, ids, lengths, mm.random_regions(np.random.default_rng(1000 + seed), lengths)))

    def get(seed, with_regions, pairs=False):
        s, e, ids, lengths, regions = data[seed]
        n = s.size & ~1 if pairs else s.size
        regions = regions if with_regions else None
        key = (seed, with_regions, pairs)
        if key not in models:
            models[key] = mm.Model(oracle, s[:n], e[:n], ids[:n], lengths, 64, regions=regions, whole_pairs=pairs)
        return s[:n], e[:n], ids[:n], lengths, regions, models[key]
    return get


@pytest.mark.parametrize("with_regions", [False, True], ids=["everywhere", "regions"])
@pytest.mark.parametrize("seed", range(6))
def test_mixed_spans_end_on_the_models_coverage_with_the_oracles_mask(solver, mixed, seed, with_regions):
    s, e, ids, lengths, regions, model = mixed(seed, with_regions)
    total = model.total_bases
    budgets = [0, 1] + [int(total * f) for f in (0.1, 0.37, 0.5, 0.9)] + [total - 1, total, 1 << 63]
    for budget in budgets:
        if budget < 0:
            continue                                                              # (no base inside the regions)
        got, M, ms, curve = solver.solve_mean_depth(s, e, ids, lengths, 64, budget_bases=budget, curve=True,
                                                    **table_args(regions))
        assert model.answers(budget) == [M], (budget, M)                          # monotone here (test_mean_depth_cpu.py)
        check_answer(model, budget, got, M, ms, curve, regions)
        if budget == 0 and model.curve_R()[min(1, model.top)] > 0:
            assert ms.probes == 0 and M == 0 and not got.any()                    # the bound alone: S_R(1) > 0
        if budget >= total:
            assert M == model.top
        assert solver.last_stats.n_kept == (model.count(M) if M else 0)
        assert report_sum(solver, s, e, ids, lengths, got, regions) == ms.kept_bases
    # a mean depth is floor(mean * positions), and the package's positions are the library's
    got, M, ms = solver.solve_mean_depth(s, e, ids, lengths, 64, mean_depth=2.5, **table_args(regions))
    assert ms.budget == int(np.floor(2.5 * model.positions)) and ms.positions == model.positions
    check_answer(model, int(ms.budget), got, M, ms, None, regions)
    # a short curve buffer takes what fits
    _, _, _, short = solver.solve_mean_depth(s, e, ids, lengths, 3, budget_bases=total, curve=True, **table_args(regions))
    assert np.array_equal(short, model.curve_R()[:short.size]) and short.size == min(3, model.max_depth) + 1


# ------------------------------------------------------------------------------------------ 2: one span, deep
@pytest.fixture(scope="module")
def deep(oracle):
    rng = np.random.default_rng(202)
    L, n, span = 20_000, 40_000, 150
    s = rng.integers(0, L - span + 1, n).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    ids = np.zeros(n, np.uint32)
    model = mm.Model(oracle, s, e, ids, [L], 200)
    assert model.max_depth > 200 and model.top == 200
    return s, e, ids, [L], model


ROUTES = [{}, {"QMCP_HIP_SWEEP": "fast"}, {"QMCP_HIP_SWEEP": "gen"}, {"QMCP_HIP_SWEEP": "ev"}, {"QMCP_HIP_CUTS": "1"},
          {"QMCP_HIP_CUTS": "0"}, {"QMCP_HIP_NO_RANK": "1"}, {"QMCP_HIP_NEAR": "0"}]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "-".join(f"{k[9:]}={v}" for k, v in r.items()) or "auto")
def test_one_span_deep_under_every_forced_route(solver, deep, route):
    s, e, ids, lengths, model = deep
    total = model.total_bases
    for budget in ((total // 10, total // 2, 9 * total // 10) if not route else (total // 2,)):
        with forced(solver, **route):
            got, M, ms, curve = solver.solve_mean_depth(s, e, ids, lengths, 200, budget_bases=budget, curve=True)
        assert M == model.largest(budget), (budget, M)
        check_answer(model, budget, got, M, ms, curve)
        print(f"route {route or 'auto'}, budget {budget}: M* = {M}, {ms.probes} probes, kept_bases {ms.kept_bases}")


# ------------------------------------------------------------------------------------------ 3: sums beyond 32 bits
@pytest.mark.parametrize("L,n,want,with_regions", [((1 << 24) - 1, 300, 280, False), ((1 << 20) - 1, 6000, 5000, True)],
                         ids=["everywhere", "regions"])
def test_sums_beyond_32_bits(solver, L, n, want, with_regions):
    """n identical reads covering all of one contig: a cover of min(cov, M) = M is any M reads, so bases(M) = M |R| and
    M* = floor(budget / |R|); kept and total bases exceed 2^32.  With the regions -- everything but position 0, on a
    shorter contig under more reads -- the sums are the region tally's and the weighted count's.  (The solve itself takes
    seconds on a contig this long: one serial sweep over its positions; the call runs one or two of them.)"""
    s, e, ids = np.zeros(n, np.uint32), np.full(n, L - 1, np.uint32), np.zeros(n, np.uint32)
    regions = (np.array([0, 2], np.uint32), np.array([1, 70_000], np.uint32), np.array([70_000, L + 5], np.uint32))
    P = L - 1 if with_regions else L
    budget = want * P + 12_345
    got, M, ms, curve = solver.solve_mean_depth(s, e, ids, [L], 10_000, budget_bases=budget, curve=True,
                                                **(table_args(regions) if with_regions else {}))
    assert M == want == ms.coverage == ms.n_kept == popcount(got) and ms.positions == P
    assert ms.kept_bases == want * P > 1 << 32 and ms.total_bases == n * P > 1 << 32
    assert (ms.max_depth, ms.top, ms.reads_placed, ms.saturated) == (n, n, n, 0)
    assert (ms.bases_above, ms.bound_above) in (((want + 1) * P, 0), (0, (want + 1) * P))
    assert np.array_equal(curve, P * np.arange(n + 1, dtype=np.uint64)) and ms.probes <= bm.probe_limit(n)
    assert (ms.regions_in, ms.regions_used) == ((2, 1) if with_regions else (0, 0))
    assert np.array_equal(got, solver.solve_by_contig(s, e, ids, [L], M))         # (the oracle's rule: checked in case 1)
    print(f"L {L}, {n} reads: M* = {M}, {ms.probes} probes, ms_solves {ms.ms_solves:.0f}")


# ------------------------------------------------------------------------------------------ 4: the clamped last bin
def test_the_clamped_last_bin_with_regions(solver):
    L, n, want = 64, 12_000, 9_000
    s, e, ids = np.zeros(n, np.uint32), np.full(n, L - 1, np.uint32), np.zeros(n, np.uint32)
    regions = (np.array([0, 2], np.uint32), np.array([40, 10], np.uint32), np.array([63, 19], np.uint32))
    budget = 34 * want + 7
    got, M, ms, curve = solver.solve_mean_depth(s, e, ids, [L], 20_000, budget_bases=budget, curve=True, **table_args(regions))
    assert M == want == ms.n_kept == popcount(got) and ms.kept_bases == 34 * want and ms.positions == 34
    assert ms.max_depth == n and ms.top == n and ms.total_bases == 34 * n and ms.reads_placed == n
    assert ms.curve_entries == 8192 == curve.size
    assert np.array_equal(curve, 34 * np.arange(8192, dtype=np.uint64))
    # beyond the curve the bound is the curve's last entry: it rules nothing out there, a probe does
    assert ms.bases_above == 34 * (want + 1) and ms.bound_above == 0
    assert ms.probes <= bm.probe_limit(n) and ms.saturated == 0 and (ms.regions_in, ms.regions_used) == (2, 2)
    assert np.array_equal(got, solver.solve_by_contig(s, e, ids, [L], M))


# ------------------------------------------------------------------------------------------ 5: whole pairs
@pytest.mark.parametrize("with_regions", [False, True], ids=["everywhere", "regions"])
@pytest.mark.parametrize("seed", range(6))
def test_whole_pairs_keep_properties_one_and_two(pkg, solver, mixed, seed, with_regions):
    s, e, ids, lengths, regions, model = mixed(seed, with_regions, pairs=True)
    n = s.size
    placed = ids != NO_CONTIG
    assert n == 0 or (placed[0::2] != placed[1::2]).any()                         # unplaced mates among them
    total = model.total_bases
    for budget in [0, 1, 2] + [int(total * f) for f in (0.1, 0.37, 0.5, 0.9)] + [total, model.bases(model.top)]:
        got, M, ms, curve = solver.solve_mean_depth(s, e, ids, lengths, 64, budget_bases=budget,
                                                    flags=pkg.MEAN_DEPTH_WHOLE_PAIRS, curve=True, **table_args(regions))
        assert M in model.answers(budget), (budget, M, model.answers(budget))     # (1) and (2); not claimed unique
        check_answer(model, budget, got, M, ms, curve, regions)                   # kept_bases: on the completed mask
        kept = bm.unpack(got, n)
        both = placed[0::2] & placed[1::2]
        assert np.array_equal(kept[0::2][both], kept[1::2][both]) and not kept[~placed].any()
        assert report_sum(solver, s, e, ids, lengths, got, regions) == ms.kept_bases
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_mean_depth(s[:n - 1], e[:n - 1], ids[:n - 1], lengths, 64, budget_bases=5,
                                flags=pkg.MEAN_DEPTH_WHOLE_PAIRS)
    assert ex.value.code == pkg.QMCP_EINVAL and "odd" in str(ex.value)


# ------------------------------------------------------------------------------------------ 6: several batches
def test_several_batches(pkg, oracle, solver, mixed):
    """two empty contigs as long as one solver call allows between case 1's contigs cut the call into several batches,
    three of them with reads, and the regions lie on contigs of different batches: the region histogram adds up across
    them.  Contig 2 has a region that ends on its last position and contig 3, in the same batch, one that starts at 0:
    two regions on the batch's axis.  The model sees the two long contigs at length 1: a contig without reads decides
    nothing, and their one region is position 0.  Then one such contig, with that region, in front of the only contig
    with reads: two batches, the second the one with reads -- its regions start behind the first's in the table, and its
    columns are gathered once, for the depth, and reused by every probe; with several batches with reads (two of seed
    3's, three of seed 4's) the depth and every probe gather each of them"""
    huge = (1 << 31) - 3
    cases = []
    for seed, flags in ((3, 0), (4, pkg.MEAN_DEPTH_WHOLE_PAIRS)):
        s, e, ids, lengths, _, _ = mixed(seed, False, pairs=True)
        ids = ids.copy()
        on = ids != NO_CONTIG
        assert len(set(ids[on].tolist())) >= 3                                    # reads on either side of both
        ids[on] = np.array([0, 2, 3, 5], np.uint32)[ids[on]]
        wide = np.array([lengths[0], huge, lengths[1], lengths[2], huge, lengths[3]], np.uint32)
        w = wide.astype(np.int64)
        regions = (np.array([0, 2, 3, 5, 6, 7, 9], np.uint32),
                   np.array([w[0] - 60, 5, 0, w[2] - 100, 20, 0, 0, 3, w[5] // 2], np.uint32),
                   np.array([w[0] - 1, 40, 0, w[2] - 1, 30, w[3] // 2, 0, 9, w[5] + 7], np.uint32))
        live = sum(bool(np.isin(ids, group).any()) for group in ([0], [2, 3], [5]))   # seed 3: two, seed 4: three
        assert live == (3 if seed == 4 else 2)
        cases.append((s, e, ids, wide, [1, 4], regions, live, flags))
    rng = np.random.default_rng(91)
    L, n = 3000, 400
    span = rng.integers(1, 120, n)
    s = (rng.random(n) * (L - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    ids = np.where(rng.random(n) < 0.04, NO_CONTIG, 1).astype(np.uint32)
    assert 0 < np.count_nonzero(ids == NO_CONTIG) < n // 4
    regions = (np.array([0, 1, 4], np.uint32), np.array([0, 700, 40, L - 90], np.uint32),
               np.array([0, 1500, 300, L + 7], np.uint32))
    for flags in (0, pkg.MEAN_DEPTH_WHOLE_PAIRS):
        cases.append((s, e, ids, np.array([huge, L], np.uint32), [0], regions, 1, flags))

    def profiled(reads, live, **kw):
        solver.set_profiling(True)
        try:
            out = solver.solve_mean_depth(*reads, 64, **kw)
            gathers, scatters = launches(solver, "k_bc_gather"), launches(solver, "k_bc_scatter_mask")
        finally:
            solver.set_profiling(False)
        probes = out[2].probes
        assert gathers == (1 if live == 1 else live * (1 + probes)), (live, probes, gathers)
        assert scatters == live * probes, (live, probes, scatters)
        return out

    for s, e, ids, wide, long_ones, regions, live, flags in cases:
        small = wide.copy()
        small[long_ones] = 1
        w = wide.astype(np.int64)
        model = mm.Model(oracle, s, e, ids, small, 64, regions=regions, whole_pairs=bool(flags))
        if wide.size == 6:
            assert model.inside[small[:3].sum() - 1] and model.inside[small[:3].sum()]  # adjacent on the axis, two contigs
        total = model.total_bases
        for budget in (total // 5, total // 2, total):
            got, M, ms, curve = profiled((s, e, ids, wide), live, budget_bases=budget, flags=flags, curve=True,
                                         **table_args(regions))
            assert M in model.answers(budget) and (flags or model.answers(budget) == [M])
            check_answer(model, budget, got, M, ms, curve, regions)
            st = solver.last_stats                                                # the probe's at M*: zeros for M* == 0
            assert (st.n_contigs, st.total_length) == ((wide.size, int(w.sum())) if M else (0, 0)) and st.n_kept <= ms.n_kept
        # without a table every position counts: the long contigs' too
        got, M, ms = profiled((s, e, ids, wide), live, mean_depth=1e-6, flags=flags)
        assert ms.positions == int(w.sum()) and ms.budget == int(np.floor(1e-6 * int(w.sum())))
        assert M in mm.Model(oracle, s, e, ids, small, 64, whole_pairs=bool(flags)).answers(int(ms.budget))


# ------------------------------------------------------------------------------------------ 7: edges
def test_edges(pkg, oracle, solver):
    none = np.zeros(0, np.uint32)
    # no reads, with and without a table
    got, M, ms, curve = solver.solve_mean_depth(none, none, none, [100, 50], 10, budget_bases=7, curve=True)
    assert (got.size, M, ms.probes, ms.n_kept, ms.top, ms.saturated, ms.positions) == (0, 0, 0, 0, 0, 1, 150)
    assert curve.tolist() == [0]
    got, M, ms = solver.solve_mean_depth(none, none, none, [100, 50], 10, mean_depth=3.0, region_offsets=[0, 1, 2],
                                         region_starts=[90, 0], region_ends=[120, 4])
    assert (M, ms.probes, ms.positions, ms.budget, ms.regions_in, ms.regions_used) == (0, 0, 15, 45, 2, 2)
    # every read unplaced
    s, e = np.array([3, 4, 5, 6], np.uint32), np.array([9, 9, 9, 9], np.uint32)
    for flags in (0, pkg.MEAN_DEPTH_WHOLE_PAIRS):
        got, M, ms = solver.solve_mean_depth(s, e, np.full(4, NO_CONTIG, np.uint32), [100], 10, budget_bases=3, flags=flags)
        assert (M, ms.probes, ms.reads_placed, ms.max_depth, ms.kept_bases) == (0, 0, 0, 0, 0) and not got.any()
    # contigs of length 0 (one with a region on it: dropped) and contigs without reads between others
    rng = np.random.default_rng(55)
    lengths = np.array([0, 900, 0, 400, 700, 0, 1200, 0], np.uint32)
    ids = rng.choice([1, 4, 6], 3000).astype(np.uint32)
    span = rng.integers(1, 120, 3000)
    s = (rng.random(3000) * (lengths[ids] - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    ids[rng.random(3000) < 0.05] = NO_CONTIG
    tables = {
        "none": None,
        "some": (np.array([0, 1, 3, 3, 4, 4, 5, 7, 7], np.uint32), np.array([0, 100, 850, 0, 2, 0, 600], np.uint32),
                 np.array([5, 300, 950, 399, 9, 0, 1199], np.uint32)),
        "empty": (np.zeros(9, np.uint32), none, none),
        "off the reads": (np.array([0, 0, 0, 0, 1, 1, 1, 1, 1], np.uint32), np.array([10], np.uint32),
                          np.array([300], np.uint32)),                            # contig 3 has no read
    }
    for name, regions in tables.items():
        for max_coverage in (1, 25, 10_000):
            model = mm.Model(oracle, s, e, ids, lengths, max_coverage, regions=regions)
            total = model.total_bases
            for budget in (0, 1, total // 4, total // 2, total, 1 << 40):
                got, M, ms, curve = solver.solve_mean_depth(s, e, ids, lengths, max_coverage, budget_bases=budget,
                                                            curve=True, **table_args(regions))
                assert M in model.answers(budget), (name, max_coverage, budget, M)    # (1) and (2)
                check_answer(model, budget, got, M, ms, curve, regions)
                if max_coverage == 1:
                    assert M == (1 if model.bases(1) <= budget else 0) and ms.probes <= 1
                if name in ("empty", "off the reads"):
                    # no base inside the regions: every coverage fits every budget, the answer is the deepest
                    assert ms.kept_bases == 0 == ms.total_bases and M == model.top and ms.probes == 1
                    assert ms.positions == (0 if name == "empty" else 291)
                assert report_sum(solver, s, e, ids, lengths, got, regions) == ms.kept_bases
    # more merged regions than the weights' kernel stages in LDS, each shorter than a wave: the table is read from memory
    L = 60_000
    r0 = np.arange(0, L, 10, dtype=np.uint32)[::-1].copy()
    regions = (np.array([0, r0.size], np.uint32), r0, r0 + 2)
    span = rng.integers(1, 200, 4000)
    s = (rng.random(4000) * (L - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    ids = np.zeros(4000, np.uint32)
    model = mm.Model(oracle, s, e, ids, [L], 40, regions=regions)
    assert model.positions == 3 * 6000 and merged_regions(model) == 6000 > 4096
    for budget in (model.total_bases // 3, model.total_bases):
        got, M, ms, curve = solver.solve_mean_depth(s, e, ids, [L], 40, budget_bases=budget, curve=True, **table_args(regions))
        assert M in model.answers(budget)
        check_answer(model, budget, got, M, ms, curve, regions)
        assert report_sum(solver, s, e, ids, [L], got, regions) == ms.kept_bases


# ------------------------------------------------------------------------------------------ 8: the device entry
def test_device_entry_equals_the_host_entry_and_waits_for_the_callers_stream(pkg, solver, mixed):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    for seed, flags, with_regions, shift in ((1, 0, True, 0), (2, pkg.MEAN_DEPTH_WHOLE_PAIRS, True, 1),
                                             (5, pkg.MEAN_DEPTH_WHOLE_PAIRS, False, 1), (0, 0, False, 0)):
        s, e, ids, lengths, regions, model = mixed(seed, with_regions, pairs=bool(flags))
        n = s.size & ~1
        s, e, ids = s[:n], e[:n], ids[:n]
        if not flags:                              # (the same reads as under the flag: an even count)
            model = mm.Model(model.oracle, s, e, ids, lengths, 64, regions=regions)
        budget = model.total_bases // 3
        want, want_M, want_ms, want_curve = solver.solve_mean_depth(s, e, ids, lengths, 64, budget_bases=budget, flags=flags,
                                                                    curve=True, **table_args(regions))
        side = torch.cuda.Stream(device=dev)
        # shift 1: the columns begin one element into their buffers -- 4-byte aligned only, the 32-bit forms run
        d_s, d_e, d_ids = (torch.zeros(n + shift, dtype=torch.int32, device=dev)[shift:] for _ in range(3))
        src = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids)]
        d_mask = torch.full((pkg.mask_words(n),), -1, dtype=torch.int64, device=dev)
        assert all(t.data_ptr() % 16 == 4 * shift for t in (d_s, d_e, d_ids))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(4):                     # (the columns are still being written when the call is made)
                d_s.copy_(src[2]); d_e.copy_(src[0]); d_ids.copy_(src[1])
            d_s.copy_(src[0]); d_e.copy_(src[1]); d_ids.copy_(src[2])
            M, ms, curve = solver.solve_mean_depth_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, 64,
                                                          d_mask.data_ptr(), budget_bases=budget, flags=flags, curve=True,
                                                          stream=side.cuda_stream, **table_args(regions))
        got = d_mask.cpu().numpy().view(np.uint64)
        assert M == want_M and np.array_equal(got, want) and np.array_equal(curve, want_curve)
        for f in FIELDS:
            assert getattr(ms, f) == getattr(want_ms, f), f
        check_answer(model, budget, got, M, ms, curve, regions)
        # a mean depth on the device entry
        M2, ms2 = solver.solve_mean_depth_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, 64,
                                                 d_mask.data_ptr(), mean_depth=1.25, flags=flags, **table_args(regions))
        assert ms2.budget == int(np.floor(1.25 * model.positions)) and M2 in model.answers(int(ms2.budget))


# ------------------------------------------------------------------------------------------ 9: bad input
def test_a_bad_read_or_contig_id_has_the_by_contig_code_and_leaves_the_mask_alone(pkg, solver):
    torch = pytest.importorskip("torch")
    s = np.array([0, 5, 9, 1], np.uint32)
    e = np.array([3, 8, 9, 2], np.uint32)
    cases = [(np.array([0, 2, 0, 0], np.uint32), [10, 10], pkg.QMCP_EINVAL),     # id 2 of 2 contigs
             (np.array([0, 1, 1, 0], np.uint32), [10, 9], pkg.QMCP_EREAD),       # end 9 on a 9-position contig
             (np.array([0, 0, 0, 0], np.uint32), [10, 1 << 31], pkg.QMCP_ERANGE)]
    dev = torch.device("cuda", 0)
    offs, r0, r1 = (np.array(v, np.uint32) for v in ([0, 1, 2], [2, 0], [6, 3]))
    for ids, lengths, code in cases:
        with pytest.raises(pkg.QmcpError) as by_contig:
            solver.solve_by_contig(s, e, ids, lengths, 2)
        assert by_contig.value.code == code
        mask = np.full(1, 0xABCDEF, np.uint64)
        st, ms = pkg.Stats(), pkg.MeanDepthStats()
        lens = np.asarray(lengths, np.uint32)
        rc = pkg._hip.qmcp_hip_solve_mean_depth_host(solver._ctx, pkg._p32(s), pkg._p32(e), pkg._p32(ids), 4, pkg._p32(lens),
                                                     lens.size, 5, 20, pkg._p32(offs), pkg._p32(r0), pkg._p32(r1), 0, None, 0,
                                                     pkg._p64(mask), st, ms)
        assert rc == code and mask[0] == 0xABCDEF
        d = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids)]
        d_mask = torch.full((1,), 0x1234, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        with pytest.raises(pkg.QmcpError) as ex:
            solver.solve_mean_depth_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 4, lengths, 5,
                                           d_mask.data_ptr(), budget_bases=20)
        assert ex.value.code == code and int(d_mask.cpu()[0]) == 0x1234
    # the context is whole afterwards
    got, M, ms = solver.solve_mean_depth(s, e, np.zeros(4, np.uint32), [10], 5, budget_bases=11)
    assert M == ms.top and popcount(got) == 4 and ms.saturated == 1 and ms.kept_bases == 11


# ------------------------------------------------------------------------------------------ 10: the file flow
def test_downsample_bam_mean_depth_writes_whole_pairs_within_the_base_budget(pkg, oracle, solver, tmp_path):
    path = os.path.join(GOLDEN, "tiny_other_writer.bam")
    bed = tmp_path / "regions.bed"
    bed.write_text("chrT\t100\t600\nchrT\t500\t1000\nchrT\t2550\t9000\nchrU\t0\t60\n")   # overlapping; clipped
    header, parsed, _ = bam_py.parse(path)
    # (min_mapq 15 drops the file's three-record template, whose record would otherwise be kept through two reads)
    cols = pkg.read_bam(path, per_reference=True, min_mapq=15)
    s, e, ids, lengths = cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"]
    n = s.size
    assert n % 2 == 0 and n >= 8 and np.unique(cols["bam_ids"]).size == n
    placed = ids != NO_CONTIG
    regions = pkg.targets_from_bed(bed, pkg.reference_names(path))
    model = mm.Model(oracle, s, e, ids, lengths, 200, regions=regions, whole_pairs=True)
    assert model.positions == 900 + 2450 + 60 == pkg.region_positions(lengths, *regions) and model.top >= 2
    budget = model.bases(model.top) - 1                                           # the budget bites
    out, report = tmp_path / "out.bam", tmp_path / "mean_depth.tsv"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, 200, per_reference=True, min_mapq=15,
                                 budget_bases=budget, mean_depth_targets=bed, mean_depth_report=report)
    lines = report.read_text().splitlines()
    split = lines.index("#M\tbases")
    rows = dict(line.split("\t") for line in lines[:split] if not line.startswith("#"))
    M = int(rows["coverage"])
    assert M in model.answers(budget) and 0 < M < model.top
    kept = model.bits(M)
    kept_ids = np.sort(np.asarray(cols["bam_ids"], np.int64)[np.flatnonzero(kept)])
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == len(orecs) == kept_ids.size
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]   # the mask's reads and no others
    assert model.bases(M) <= budget                                               # their bases inside the BED's regions
    both = placed[0::2] & placed[1::2]
    assert np.array_equal(kept[0::2][both], kept[1::2][both])                     # whole pairs: no find_pairs followed
    # the report's numbers are the stats of the same call made here
    got, M2, ms, curve = solver.solve_mean_depth(s, e, ids, lengths, 200, budget_bases=budget, flags=pkg.MEAN_DEPTH_WHOLE_PAIRS,
                                                 curve=True, **table_args(regions))
    check_answer(model, budget, got, M2, ms, curve, regions)
    assert M2 == M and set(rows) == {name for name, _ in pkg.MeanDepthStats._fields_} | {"records_written", "mean_depth_in",
                                                                                       "mean_depth_kept"}
    for f in FIELDS:
        assert int(rows[f]) == getattr(ms, f), f
    assert int(rows["records_written"]) == written and float(rows["ms_solves"]) >= 0
    assert float(rows["mean_depth_in"]) == pytest.approx(model.total_bases / model.positions, abs=1e-6)
    assert float(rows["mean_depth_kept"]) == pytest.approx(model.bases(M) / model.positions, abs=1e-6)
    table = np.array([line.split("\t") for line in lines[split + 1:]], dtype=np.uint64)
    assert np.array_equal(table[:, 0], np.arange(curve.size)) and np.array_equal(table[:, 1], curve)
    # a mean depth is floor(mean * the regions' positions); without a BED every position of every reference counts
    report2 = tmp_path / "mean2.tsv"
    written2 = pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "out2.bam", 200, per_reference=True, min_mapq=15,
                                  mean_depth=0.2, mean_depth_report=report2)
    rows2 = dict(line.split("\t") for line in report2.read_text().splitlines() if not line.startswith("#") and
                 not line[0].isdigit())
    everywhere = mm.Model(oracle, s, e, ids, lengths, 200, whole_pairs=True)
    total = int(np.asarray(lengths, np.int64).sum())
    assert int(rows2["positions"]) == total and int(rows2["budget"]) == int(np.floor(0.2 * total))
    assert int(rows2["coverage"]) in everywhere.answers(int(rows2["budget"]))
    assert written2 == int(rows2["n_kept"]) == everywhere.count(int(rows2["coverage"]))
    assert int(rows2["kept_bases"]) == everywhere.bases(int(rows2["coverage"])) <= int(rows2["budget"])
