"""qmcp_hip_solve_budget_*: the deepest coverage whose by-contig solve fits a read budget.  Every expected value comes
from the CPU oracle and numpy (tests/budget_model.py): M* from brute force over every coverage (or the model's own
bisection where 0 .. top is long), the mask from the oracle at M*, the curve from the definition."""
import time

import numpy as np
import pytest

import bam_py
import budget_model as bm
import multi_reference as mr
from forcing import forced

pytestmark = pytest.mark.gpu

NO_CONTIG = mr.NO_CONTIG


def popcount(mask):
    return int(np.unpackbits(np.ascontiguousarray(mask).view(np.uint8)).sum())


def check_answer(model, budget, got, M, bs, curve=None):
    """one call's mask, coverage and statistics against the model"""
    where = (budget, M, bs.as_dict())
    assert M == bs.coverage and bs.budget == budget and bs.top == model.top, where
    assert bs.reads_placed == model.placed and bs.max_depth == model.max_depth, where
    assert bs.total_bases == model.total_bases, where
    assert np.array_equal(got, model.mask(M)), where                              # bit for bit the solve at M*
    assert bs.n_kept == popcount(got) == model.count(M) <= budget, where          # (1)
    if M < model.top:
        above = model.count(M + 1)
        assert above > budget, where                                              # (2)
        assert bs.kept_above in (0, above) and bs.bound_above <= above, where
        assert bs.kept_above > budget or bs.bound_above > budget, where           # one of the two ruled M* + 1 out
    else:
        assert bs.kept_above == 0 and bs.bound_above == 0, where
    assert bs.probes <= bm.probe_limit(model.top), where
    assert bs.saturated == (1 if bs.n_kept == model.placed else 0), where
    if curve is not None:
        assert bs.curve_entries == curve.size and np.array_equal(curve, model.curve()), where


# ------------------------------------------------------------------------------------------ 1: mixed spans
@pytest.fixture(scope="module")
def mixed(oracle):
    """random_by_contig(rng, 4, 2500), seeds 0 .. 5, each with its model (the oracle's masks are cached in it)"""
    out = []
    for seed in range(6):
        s, e, ids, lengths = mr.random_by_contig(np.random.default_rng(seed), 4, 2500)
        out.append((s, e, ids, lengths, bm.Model(oracle, s, e, ids, lengths, 64)))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_mixed_spans_end_on_the_models_coverage_with_the_oracles_mask(solver, mixed, seed):
    s, e, ids, lengths, model = mixed[seed]
    placed = model.placed
    budgets = [0, 1] + [int(placed * f) for f in (0.1, 0.37, 0.5, 0.9)] + [placed - 1, placed, 1 << 63]
    for budget in budgets:
        if budget < 0:
            continue                                                              # (a seed without a placed read)
        got, M, bs, curve = solver.solve_budget(s, e, ids, lengths, 64, budget_reads=budget, curve=True)
        assert model.answers(budget) == [M], (budget, M)                          # the one largest feasible coverage
        check_answer(model, budget, got, M, bs, curve)
        if budget == 0:
            assert bs.probes == 0 and M == 0 and not got.any()
        if budget >= placed:
            assert M == model.top
        assert solver.last_stats.n_kept == (model.count(M) if M else 0)
    # a fraction is floor(f * placed reads)
    got, M, bs = solver.solve_budget(s, e, ids, lengths, 64, fraction=0.37)
    assert bs.budget == int(np.floor(0.37 * placed))
    check_answer(model, bs.budget, got, M, bs)
    # a short curve buffer takes what fits
    _, _, bs2, short = solver.solve_budget(s, e, ids, lengths, 3, budget_reads=placed, curve=True)
    assert np.array_equal(short, bm.Model(model.oracle, s, e, ids, lengths, 3).curve()) and short.size == min(3, model.max_depth) + 1


# ------------------------------------------------------------------------------------------ 2: one span, deep
@pytest.fixture(scope="module")
def deep(oracle):
    rng = np.random.default_rng(202)
    L, n, span = 20_000, 40_000, 150
    s = rng.integers(0, L - span + 1, n).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    ids = np.zeros(n, np.uint32)
    model = bm.Model(oracle, s, e, ids, [L], 200)
    assert model.max_depth > 200 and model.top == 200
    return s, e, ids, [L], model


ROUTES = [{}, {"QMCP_HIP_SWEEP": "fast"}, {"QMCP_HIP_SWEEP": "gen"}, {"QMCP_HIP_SWEEP": "ev"}, {"QMCP_HIP_CUTS": "1"},
          {"QMCP_HIP_CUTS": "0"}, {"QMCP_HIP_NO_RANK": "1"}, {"QMCP_HIP_NEAR": "0"}]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "-".join(f"{k[9:]}={v}" for k, v in r.items()) or "auto")
def test_one_span_deep_under_every_forced_route(solver, deep, route):
    s, e, ids, lengths, model = deep
    n = s.size
    for budget in ((n // 10, n // 2, 9 * n // 10) if not route else (n // 2,)):
        with forced(solver, **route):
            got, M, bs, curve = solver.solve_budget(s, e, ids, lengths, 200, budget_reads=budget, curve=True)
        assert M == model.largest(budget), (budget, M)
        check_answer(model, budget, got, M, bs, curve)
        print(f"route {route or 'auto'}, budget {budget}: M* = {M}, {bs.probes} probes, n_kept {bs.n_kept}")


# ------------------------------------------------------------------------------------------ 3: the curve's clamp
def test_a_coverage_beyond_the_curve_and_the_clamped_last_bin(solver):
    L, n, budget = 64, 12_000, 9_000
    s, e, ids = np.zeros(n, np.uint32), np.full(n, L - 1, np.uint32), np.zeros(n, np.uint32)
    got, M, bs, curve = solver.solve_budget(s, e, ids, [L], 20_000, budget_reads=budget, curve=True)
    # every read covers everything: a cover of min(cov, M) = M is any M reads, so count(M) = M, and M* is the budget
    assert M == budget == bs.n_kept == popcount(got) and bs.coverage == M
    assert bs.max_depth == n and bs.top == n and bs.total_bases == L * n and bs.reads_placed == n
    assert bs.curve_entries == 8192 == curve.size
    assert np.array_equal(curve, L * np.arange(8192, dtype=np.uint64)) and curve[-1] == 64 * 8191
    assert bs.kept_above in (0, budget + 1) and bs.bound_above <= budget + 1
    assert bs.probes <= bm.probe_limit(n) and bs.saturated == 0
    assert np.array_equal(got, solver.solve_by_contig(s, e, ids, [L], M))         # (the oracle's rule: checked in case 1)


# ------------------------------------------------------------------------------------------ 4: whole pairs
@pytest.mark.parametrize("seed", range(6))
def test_whole_pairs_keep_properties_one_and_two(pkg, oracle, solver, mixed, seed):
    s, e, ids, lengths, _ = mixed[seed]
    n = s.size & ~1
    s, e, ids = s[:n], e[:n], ids[:n]
    model = bm.Model(oracle, s, e, ids, lengths, 64, whole_pairs=True)
    placed = ids != NO_CONTIG
    assert n == 0 or (placed[0::2] != placed[1::2]).any()                         # unplaced mates among them
    for budget in [0, 1, 2] + [int(model.placed * f) for f in (0.1, 0.37, 0.5, 0.9)] + [model.placed]:
        got, M, bs, curve = solver.solve_budget(s, e, ids, lengths, 64, budget_reads=budget,
                                                flags=pkg.BUDGET_WHOLE_PAIRS, curve=True)
        assert M in model.answers(budget), (budget, M, model.answers(budget))     # (1) and (2); not claimed unique
        check_answer(model, budget, got, M, bs, curve)
        kept = bm.unpack(got, n)
        both = placed[0::2] & placed[1::2]
        assert np.array_equal(kept[0::2][both], kept[1::2][both]) and not kept[~placed].any()
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_budget(s[:n - 1], e[:n - 1], ids[:n - 1], lengths, 64, budget_reads=5, flags=pkg.BUDGET_WHOLE_PAIRS)
    assert ex.value.code == pkg.QMCP_EINVAL and "odd" in str(ex.value)


# ------------------------------------------------------------------------------------------ 5: edges
def test_edges(pkg, oracle, solver):
    none = np.zeros(0, np.uint32)
    got, M, bs, curve = solver.solve_budget(none, none, none, [100, 50], 10, budget_reads=7, curve=True)
    assert (got.size, M, bs.probes, bs.n_kept, bs.top, bs.saturated) == (0, 0, 0, 0, 0, 1) and curve.tolist() == [0]
    # every read unplaced
    s, e = np.array([3, 4, 5, 6], np.uint32), np.array([9, 9, 9, 9], np.uint32)
    for flags in (0, pkg.BUDGET_WHOLE_PAIRS):
        got, M, bs = solver.solve_budget(s, e, np.full(4, NO_CONTIG, np.uint32), [100], 10, budget_reads=3, flags=flags)
        assert (M, bs.probes, bs.reads_placed, bs.max_depth) == (0, 0, 0, 0) and not got.any()
    # contigs of length 0 and contigs without reads between others
    rng = np.random.default_rng(55)
    lengths = np.array([0, 900, 0, 400, 700, 0, 1200, 0], np.uint32)
    ids = rng.choice([1, 4, 6], 3000).astype(np.uint32)
    span = rng.integers(1, 120, 3000)
    s = (rng.random(3000) * (lengths[ids] - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    ids[rng.random(3000) < 0.05] = NO_CONTIG
    for max_coverage in (1, 25, 10_000):
        model = bm.Model(oracle, s, e, ids, lengths, max_coverage)
        for budget in (0, 1, model.placed // 4, model.placed // 2, model.placed, 1 << 40):
            got, M, bs, curve = solver.solve_budget(s, e, ids, lengths, max_coverage, budget_reads=budget, curve=True)
            assert model.answers(budget) == [M]
            check_answer(model, budget, got, M, bs, curve)
            if max_coverage == 1:
                assert M == (1 if model.count(1) <= budget else 0) and bs.probes <= 1
            if budget >= model.placed:
                # the budget covers every placed read, but a search that ends below the largest depth keeps fewer
                assert M == model.top and bs.saturated == (1 if model.count(M) == model.placed else 0)
    assert bm.Model(oracle, s, e, ids, lengths, 25).count(25) < model.placed      # (so saturated == 0 was exercised)


def launches(solver, name):
    return solver.kernel_times().get(name, (0, 0.0))[0]


def test_several_batches(pkg, oracle, solver, mixed):
    """two empty contigs as long as one solver call allows between case 1's contigs cut the call into several batches,
    three of them with reads: every probe then runs over all of them, and the depth histogram adds up across them.  The
    model sees the two at length 1: a contig without reads decides nothing.  Then one such contig in front of the only
    contig with reads: two batches, the second the one with reads -- its columns are gathered once, for the depth, and
    every probe reuses them; with several batches with reads (two of seed 3's, three of seed 4's) the depth and every probe
    gather each of them"""
    huge = (1 << 31) - 3
    cases = []
    for seed, flags in ((3, 0), (4, pkg.BUDGET_WHOLE_PAIRS)):
        s, e, ids, lengths, _ = mixed[seed]
        n = s.size & ~1
        s, e, ids = s[:n], e[:n], ids[:n].copy()
        on = ids != NO_CONTIG
        assert len(set(ids[on].tolist())) >= 3                                    # reads on either side of both
        ids[on] = np.array([0, 2, 3, 5], np.uint32)[ids[on]]
        wide = np.array([lengths[0], huge, lengths[1], lengths[2], huge, lengths[3]], np.uint32)
        live = sum(bool(np.isin(ids, group).any()) for group in ([0], [2, 3], [5]))   # seed 3: two, seed 4: three
        assert live == (3 if seed == 4 else 2)
        cases.append((s, e, ids, wide, [1, 4], live, flags))
    rng = np.random.default_rng(91)
    L, n = 3000, 400
    span = rng.integers(1, 120, n)
    s = (rng.random(n) * (L - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    ids = np.where(rng.random(n) < 0.04, NO_CONTIG, 1).astype(np.uint32)
    assert 0 < np.count_nonzero(ids == NO_CONTIG) < n // 4
    for flags in (0, pkg.BUDGET_WHOLE_PAIRS):
        cases.append((s, e, ids, np.array([huge, L], np.uint32), [0], 1, flags))
    for s, e, ids, wide, long_ones, live, flags in cases:
        small = wide.copy()
        small[long_ones] = 1
        model = bm.Model(oracle, s, e, ids, small, 64, whole_pairs=bool(flags))
        for budget in (model.placed // 5, model.placed // 2, model.placed):
            solver.set_profiling(True)
            try:
                got, M, bs, curve = solver.solve_budget(s, e, ids, wide, 64, budget_reads=budget, flags=flags, curve=True)
                gathers, scatters = launches(solver, "k_bc_gather"), launches(solver, "k_bc_scatter_mask")
            finally:
                solver.set_profiling(False)
            assert M in model.answers(budget) and (flags or model.answers(budget) == [M])
            check_answer(model, budget, got, M, bs, curve)
            st = solver.last_stats                                                # the probe's at M*: zeros for M* == 0
            assert (st.n_contigs, st.total_length) == ((wide.size, int(wide.astype(np.int64).sum())) if M else (0, 0))
            assert st.n_kept <= bs.n_kept
            assert gathers == (1 if live == 1 else live * (1 + bs.probes)), (live, bs.probes, gathers)
            assert scatters == live * bs.probes, (live, bs.probes, scatters)


# ------------------------------------------------------------------------------------------ 6: the device entry
def test_device_entry_equals_the_host_entry_and_waits_for_the_callers_stream(pkg, solver, mixed):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    for seed, flags in ((1, 0), (2, pkg.BUDGET_WHOLE_PAIRS)):
        s, e, ids, lengths, model = mixed[seed]
        n = s.size & ~1
        s, e, ids = s[:n], e[:n], ids[:n]
        placed = int((ids != NO_CONTIG).sum())
        budget = placed // 3
        want, want_M, want_bs, want_curve = solver.solve_budget(s, e, ids, lengths, 64, budget_reads=budget, flags=flags,
                                                                curve=True)
        side = torch.cuda.Stream(device=dev)
        d_s, d_e, d_ids = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
        src = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids)]
        d_mask = torch.full((pkg.mask_words(n),), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(4):                     # (the columns are still being written when the call is made)
                d_s.copy_(src[2]); d_e.copy_(src[0]); d_ids.copy_(src[1])
            d_s.copy_(src[0]); d_e.copy_(src[1]); d_ids.copy_(src[2])
            M, bs, curve = solver.solve_budget_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, 64,
                                                      d_mask.data_ptr(), budget_reads=budget, flags=flags, curve=True,
                                                      stream=side.cuda_stream)
        got = d_mask.cpu().numpy().view(np.uint64)
        assert M == want_M and np.array_equal(got, want) and np.array_equal(curve, want_curve)
        for f in ("budget", "reads_placed", "n_kept", "kept_above", "bound_above", "total_bases", "coverage", "max_depth",
                  "top", "probes", "curve_entries", "saturated"):
            assert getattr(bs, f) == getattr(want_bs, f), f
        # fraction on the device entry: the caller counts the placed reads
        M2, bs2 = solver.solve_budget_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, 64,
                                             d_mask.data_ptr(), fraction=1 / 3, placed_reads=placed, flags=flags)
        assert bs2.budget == int(np.floor((1 / 3) * placed)) and M2 == solver.solve_budget(
            s, e, ids, lengths, 64, budget_reads=int(bs2.budget), flags=flags)[1]


# ------------------------------------------------------------------------------------------ 7: bad input
def test_a_bad_read_or_contig_id_has_the_by_contig_code_and_leaves_the_mask_alone(pkg, solver):
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
        mask = np.full(1, 0xABCDEF, np.uint64)
        st, bs = pkg.Stats(), pkg.BudgetStats()
        lens = np.asarray(lengths, np.uint32)
        rc = pkg._hip.qmcp_hip_solve_budget_host(solver._ctx, pkg._p32(s), pkg._p32(e), pkg._p32(ids), 4, pkg._p32(lens),
                                                 lens.size, 5, 2, 0, None, 0, pkg._p64(mask), st, bs)
        assert rc == code and mask[0] == 0xABCDEF
        d = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids)]
        d_mask = torch.full((1,), 0x1234, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        with pytest.raises(pkg.QmcpError) as ex:
            solver.solve_budget_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 4, lengths, 5, d_mask.data_ptr(),
                                       budget_reads=2)
        assert ex.value.code == code and int(d_mask.cpu()[0]) == 0x1234
    # the context is whole afterwards
    got, M, bs = solver.solve_budget(s, e, np.zeros(4, np.uint32), [10], 5, budget_reads=4)
    assert M == bs.top and popcount(got) == 4 and bs.saturated == 1


# ------------------------------------------------------------------------------------------ 8: the file flow
def test_downsample_bam_budget_writes_whole_pairs_within_the_budget(pkg, oracle, solver, tmp_path):
    path = tmp_path / "in.bam"
    refs = [("chrA", 5000), ("chrB", 3000), ("chrC", 1200)]
    header, parsed, _ = mr.write_multi_reference_bam(path, np.random.default_rng(23), refs, 1500)
    cols = pkg.read_bam(path, per_reference=True)
    s, e, ids, lengths = cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"]
    n = s.size
    assert n % 2 == 0 and n > 2000
    placed = ids != NO_CONTIG
    model = bm.Model(oracle, s, e, ids, lengths, 200, whole_pairs=True)
    budget = len(parsed) // 3
    out, report = tmp_path / "out.bam", tmp_path / "budget.tsv"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, 200, per_reference=True, budget_reads=budget, budget_report=report)
    lines = report.read_text().splitlines()
    split = lines.index("#M\tbases")
    rows = dict(line.split("\t") for line in lines[:split] if not line.startswith("#"))
    M = int(rows["coverage"])
    assert M in model.answers(budget) and 0 < M < model.top                       # the budget bites
    kept = model.bits(M)
    kept_ids = np.sort(np.asarray(cols["bam_ids"], np.int64)[np.flatnonzero(kept)])
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == len(orecs) == kept_ids.size <= budget      # within the budget: no find_pairs
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]   # the mask's reads and no others
    both = placed[0::2] & placed[1::2]
    assert np.array_equal(kept[0::2][both], kept[1::2][both]) and kept[0::2][both].any()  # whole pairs
    # the report parses back to the stats and the curve
    above = model.count(M + 1)
    assert int(rows["budget"]) == budget and int(rows["reads_placed"]) == model.placed and int(rows["n_kept"]) == written
    assert int(rows["records_written"]) == written and int(rows["max_depth"]) == model.max_depth
    assert int(rows["top"]) == model.top and int(rows["total_bases"]) == model.total_bases and int(rows["saturated"]) == 0
    assert int(rows["kept_above"]) in (0, above) and int(rows["bound_above"]) <= above
    assert int(rows["probes"]) <= bm.probe_limit(model.top) and float(rows["ms_solves"]) > 0
    assert set(rows) == {name for name, _ in pkg.BudgetStats._fields_} | {"records_written"}
    curve = np.array([line.split("\t") for line in lines[split + 1:]], dtype=np.uint64)
    assert int(rows["curve_entries"]) == curve.shape[0] and np.array_equal(curve[:, 0], np.arange(curve.shape[0]))
    assert np.array_equal(curve[:, 1], model.curve())
    # the whole file's placed, filtered reads
    out2 = tmp_path / "all.bam"
    written2 = pkg.downsample_bam("quasi-mcp-hip", path, out2, 200, per_reference=True, budget_fraction=1.0)
    all_ids = np.sort(np.asarray(cols["bam_ids"], np.int64)[np.flatnonzero(placed)])
    _, orecs2, _ = bam_py.parse(out2)
    assert model.max_depth <= 200 and written2 == all_ids.size == len(orecs2)
    assert [r["raw"] for r in orecs2] == [parsed[i]["raw"] for i in all_ids.tolist()]
    # a fraction counts the placed reads
    written3 = pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "half.bam", 200, per_reference=True, budget_fraction=0.5)
    want3 = model.answers(model.placed // 2)
    assert written3 <= model.placed // 2 and written3 in [model.count(m) for m in want3]


# ------------------------------------------------------------------------------------------ 9: the cost
def test_the_budget_call_takes_no_longer_than_the_callers_bisection(pkg, solver):
    """2 M reads on 8 contigs (the ladder test's shape), max_coverage 1 000, a budget of half the reads; median of 5 runs
    after a warm-up, the two alternating in this process, timed by the wall clock around blocking calls.  The bisection is
    the only route without the entry: solve_by_contig_device per trial over 1 .. top -- it regroups the reads every
    time -- and the count by torch; the largest depth, which it needs for top, is handed to it for nothing."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    n_contigs, pairs, L, max_coverage = 8, 125_000, 20_000, 1000
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, seed=500 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
    perm = np.random.default_rng(8).permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    n = s.size
    budget = n // 2
    lengths = np.full(n_contigs, L, np.uint32)
    d_s, d_e, d_ids = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids))
    masks = [torch.zeros(pkg.mask_words(n), dtype=torch.int64, device=dev) for _ in range(3)]
    shifts = torch.arange(64, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    top = min(max_coverage, bm.depth(s, e, ids, lengths).max())
    found = {}

    def budget_call():
        M, bs = solver.solve_budget_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, max_coverage,
                                           masks[0].data_ptr(), budget_reads=budget, stream=stream)
        torch.cuda.synchronize()
        found["budget"] = (M, bs)

    def bisection():
        lo, hi, best, trial = 0, int(top) + 1, 1, 2
        masks[best].zero_()
        trials = 0
        while hi - lo > 1:
            mid = (lo + hi) // 2
            torch.cuda.synchronize()
            solver.solve_by_contig_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, mid,
                                          masks[trial].data_ptr(), stream=stream)
            count = int(((masks[trial].unsqueeze(1) >> shifts) & 1).sum())
            trials += 1
            if count <= budget:
                lo, best, trial = mid, trial, best
            else:
                hi = mid
        torch.cuda.synchronize()
        found["bisection"] = (lo, masks[best], trials)

    budget_call()
    bisection()
    (M, bs), (M_b, mask_b, trials) = found["budget"], found["bisection"]
    assert M == M_b and 0 < M < top and torch.equal(masks[0], mask_b)             # the same coverage and mask either way
    assert bs.n_kept <= budget and bs.n_kept == int(((masks[0].unsqueeze(1) >> shifts) & 1).sum())
    t_budget, t_bisect = [], []
    for _ in range(5):
        for f, times in ((budget_call, t_budget), (bisection, t_bisect)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times.append((time.perf_counter() - t0) * 1e3)
    t_budget, t_bisect = sorted(t_budget)[2], sorted(t_bisect)[2]
    print(f"budget call {t_budget:.3f} ms ({bs.probes} probes), bisection {t_bisect:.3f} ms ({trials} trials); "
          f"{bs.as_dict()}")
    assert t_budget <= t_bisect, (t_budget, t_bisect, bs.as_dict())
