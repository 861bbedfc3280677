"""The stable LSD radix sort behind every sorting entry (csrc/api/radix_passes.inc.hip) and the grouping step of the
by-contig family (group_reads): every pass count whose result lands in another buffer, the masks bit for bit against the
oracle, and the timing spans' names and launch counts.

The wide (u64 key) form of the other entries is run with at least five passes by
  test_gpu_profile_forms.py::test_case_equals_the_model["wide keys, ..."]      the capped route, 5 and 6 passes
  test_gpu_quality.py::test_keys_wider_than_32_bits_and_errors                 the quality pass
  test_gpu_dedup.py::test_wide_keys_and_the_sort_field_by_field                dedup: split u64 keys, and one sort per
                                                                               field (four rounds, the values carried over)
the plain solve's wide form is pinned here (test_plain_solve_with_64_bit_keys)."""
import numpy as np
import pytest

import multi_reference as mr
import profile_model as pm
import stratified_model as sm

pytestmark = pytest.mark.gpu

GROUPING = ("k_bc_keys", "k_radix_hist_rec(by contig)", "scan_radix_hist(by contig, 3 kernels)",
            "k_radix_scatter_rec(by contig)", "k_bc_bounds", "k_bc_gather")
BY_CONTIG_RADIX = GROUPING[1:4]
STRATIFIED_RADIX = ("k_radix_hist_rec(stratified)", "scan_radix_hist(stratified, 3 kernels)",
                    "k_radix_scatter_rec(stratified)")
STRATIFIED = ("k_st_keys",) + STRATIFIED_RADIX + ("k_bc_bounds(stratified)", "k_bc_gather", "k_bc_scatter_mask",
                                                   "k_st_tally")


def reads_on_a_few_contigs(seed, n_contigs, n=2500, unplaced=0.02):
    """n shuffled reads of mixed spans on at most six of n_contigs contigs -- the first, the last, and ids that differ
    from another one's in the second or the third key byte only (3, 259, 65 539) --, a few of them unplaced; the contigs
    that hold reads are 600 positions long, the others 40"""
    rng = np.random.default_rng(seed)
    live = np.unique([c for c in (0, 3, 259, 65_539, n_contigs // 2, n_contigs - 1) if c < n_contigs])
    lengths = np.full(n_contigs, 40, np.uint32)
    lengths[live] = 600
    ids = live[rng.integers(0, live.size, size=n)].astype(np.uint32)
    span = rng.integers(1, 120, size=n)
    s = (rng.random(n) * (600 - span + 1)).astype(np.int64)
    e = s + span - 1
    ids[rng.random(n) < unplaced] = mr.NO_CONTIG
    return s.astype(np.uint32), e.astype(np.uint32), ids, lengths      # (drawn in random order: nothing is grouped)


def grouping_spans(times):
    """the spans of the grouping, gather and scatter-back among a call's kernel times -> {name: launches}"""
    return {k: v[0] for k, v in times.items()
            if "by contig" in k or "stratified" in k or k.startswith(("k_bc_", "k_st_"))}


def profiled_twice(solver, call):
    """the call twice (the second one finds every buffer sized), the second with the per-kernel events on"""
    call()
    solver.set_profiling(True)
    try:
        got = call()
        return got, solver.kernel_times(), solver.last_stats
    finally:
        solver.set_profiling(False)


@pytest.mark.parametrize("n_contigs, passes", [(1, 1), (300, 2), (70_000, 3)])
def test_by_contig_grouping_at_every_pass_parity(solver, oracle, n_contigs, passes):
    """1, 2 and 3 passes: the grouped records end in record buffer 0, 1 and 0"""
    s, e, ids, lengths = reads_on_a_few_contigs(n_contigs, n_contigs)
    want = mr.oracle_by_contig(oracle, s, e, ids, lengths, 7)
    got, times, st = profiled_twice(solver, lambda: solver.solve_by_contig(s, e, ids, lengths, 7))
    assert np.array_equal(got, want)
    assert st.n_reads == int(np.count_nonzero(ids != mr.NO_CONTIG)) and st.n_contigs == n_contigs
    assert st.arena_grown_mid_solve == 0
    spans = grouping_spans(times)
    assert set(spans) == set(GROUPING) | {"k_bc_scatter_mask"}, sorted(spans)
    assert all(spans[k] == passes for k in BY_CONTIG_RADIX), spans
    assert spans["k_bc_keys"] == spans["k_bc_bounds"] == 1 and spans["k_bc_gather"] == spans["k_bc_scatter_mask"] >= 1


@pytest.mark.parametrize("n_strata, n_contigs, passes", [(1, 1, 1), (3, 100, 2), (3, 30_000, 3)])
def test_stratified_grouping_at_every_pass_parity(solver, oracle, n_strata, n_contigs, passes):
    s, e, ids, lengths = reads_on_a_few_contigs(100 + n_contigs, n_contigs)
    rng = np.random.default_rng(n_contigs)
    strata = sm.random_strata(rng, s.size, n_strata)
    caps = np.array([6, 2, 11][:n_strata], np.uint32)
    want = sm.stratified_bits(oracle, s, e, ids, strata, lengths, caps)
    got, times, st = profiled_twice(solver, lambda: solver.solve_stratified(s, e, ids, strata, lengths, caps))
    assert np.array_equal(got, sm.pack(want))
    rows = sm.rows(s, e, ids, strata, n_strata, want)
    assert np.array_equal(sm.rows_of(solver.last_stratum_rows), rows)
    assert st.n_kept == int(want.sum()) and st.arena_grown_mid_solve == 0
    spans = grouping_spans(times)
    assert set(spans) == set(STRATIFIED), sorted(spans)
    assert all(spans[k] == passes for k in STRATIFIED_RADIX), spans
    assert spans["k_st_keys"] == spans["k_bc_bounds(stratified)"] == spans["k_st_tally"] == 1
    assert spans["k_bc_gather"] == spans["k_bc_scatter_mask"] >= 1


def island_reads(seed, lengths, max_span, live, per_island=30):
    """reads of spans 1..max_span (both present) in islands at both ends of every contig in `live` and around a multiple
    of 64 inside it, shuffled, 3 % unplaced"""
    rng = np.random.default_rng(seed)
    ss, ee, ii = [], [], []
    for c in live:
        L = int(lengths[c])
        for a in (0, 64 * int(rng.integers(L // 256, L // 128)), L - 1):
            span = np.minimum(rng.integers(1, max_span + 1, size=per_island), L)
            span[0], span[1] = min(max_span, L), 1
            s = np.clip(a - rng.integers(0, span) + rng.integers(-2, 3, size=per_island), 0, L - span)
            ss.append(s); ee.append(s + span - 1); ii.append(np.full(per_island, c))
    s, e, ids = (np.concatenate(x) for x in (ss, ee, ii))
    perm = rng.permutation(s.size)
    s, e, ids = s[perm].astype(np.uint32), e[perm].astype(np.uint32), ids[perm].astype(np.uint32)
    ids[(rng.random(ids.size) < 0.03) & (perm > 1)] = mr.NO_CONTIG        # (the two pinned spans stay placed)
    return s, e, ids, np.asarray(lengths, np.uint32)


# 2^18 + 5 positions (19 bits) with spans 1..20 000 (15 bits): 34 key bits, five passes -- the keys end in buffer 1, the
# read indices in value buffer 0; 2^25 + 168 positions (26 bits): 41 bits, six passes -- buffer 0 and value buffer 1
WIDE = {5: ([100_000, 100_000, (1 << 18) + 5 - 200_000], (0, 1, 2)),
        6: ([167_773] * 200, (0, 1, 77, 130, 198, 199))}


@pytest.mark.parametrize("passes", sorted(WIDE))
def test_plain_solve_with_64_bit_keys(pkg, solver, oracle, passes):
    """the plain solve's sort-based route on u64 keys and a split value column, through the by-contig entry (one batch);
    the oracle runs on profile_model.compact's copy of the instance (the islands moved together)"""
    lengths, live = WIDE[passes]
    s, e, ids, lengths = island_reads(900 + passes, lengths, 20_000, live)
    want = mr.oracle_by_contig(oracle, *pm.compact(s, e, ids, lengths)[:4], 4)
    for cut_points in (-1, 1):
        with solver.options(cut_points=cut_points):
            got, times, st = profiled_twice(solver, lambda: solver.solve_by_contig(s, e, ids, lengths, 4))
        assert np.array_equal(got, want), cut_points
        assert st.path == pkg.PATH_GENERAL and st.sort_passes == passes and (st.min_span, st.max_span) == (1, 20_000)
        assert st.arena_grown_mid_solve == 0
        assert times["k_radix_hist"][0] == times["scan_radix_hist(3 kernels)"][0] == times["k_radix_scatter"][0] == passes
        assert "k_radix_hist_rec" not in times
