"""The pass-major route's narrow stages after they were folded together (csrc/kernels/pass_major.inc.hip): the table
stage in two launches (k_pm_row_sums, k_pm_tables) instead of a three-launch scan, k_pm_descr and k_pm_range_table; the
settling of the quota-crossing groups in k_pm_walk's own tail instead of k_pm_settle.  Every case compares the keep mask
of the pass-major form with the range-major form's (options(pass_major=-1)) and the oracle's, on the smallest inputs the
route takes (the ranked route starts at 128 Ki reads).  The partition's arithmetic has a host model of its own:
tests/test_pm_tables_model.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _reads(rng, lengths, counts, span):
    ss, ee = [], []
    for L, k in zip(lengths, counts):
        sp = min(span, int(L))
        a = rng.integers(0, int(L) - sp + 1, size=int(k), dtype=np.uint32)
        ss.append(a); ee.append((a + np.uint32(sp - 1)).astype(np.uint32))
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return np.concatenate(ss), np.concatenate(ee), np.array(lengths, np.uint32), offs


def _three_way(pkg, oracle, lengths, counts, span, M, seed, **opts):
    """-> (kernel_times of the pass-major solve, its stats); asserts pass-major == range-major == oracle"""
    s, e, lengths, offs = _reads(np.random.default_rng(seed), lengths, counts, span)
    with pkg.Solver(0) as sv:
        sv.set_profiling(True)
        with sv.options(pass_major=1, **opts):
            pm = sv.solve(s, e, lengths, M, contig_read_offsets=offs)
        times, st = sv.kernel_times(), sv.last_stats
        with sv.options(pass_major=-1, **opts):
            rm = sv.solve(s, e, lengths, M, contig_read_offsets=offs)
    assert np.array_equal(pm, rm)
    assert np.array_equal(pm, oracle.solve(s, e, lengths, M, contig_read_offsets=offs))
    return times, st


def _assert_folded(times, solves=1):
    assert "k_pm_walk" in times
    assert "k_pm_settle" not in times and "scan_radix_hist(3 kernels)" not in times
    assert times["k_pm_row_sums"][0] == solves and times["k_pm_tables"][0] == solves


TABLE_EDGES = [
    # lengths, read counts, span, M
    ([100_000], [131_072], 150, 40),                      # sixteen full passes: pitch 16, the last pass full
    ([100_000], [131_073], 150, 40),                      # one read into the next pass; three padded passes of zeros
    ([100_000], [8192 * 19 + 5], 150, 40),                # pitch 20: row parts of 3, 3, ..., 2, 0 entries
    ([5_000, 50_000, 5_000], [0, 200_001, 0], 100, 25),   # reads only in the middle contig: ranges without a record
    ([(1 << 21) - 5], [600_000], 150, 3),                 # 256 ranges, most slices empty, ranges with no listed group
]


@pytest.mark.parametrize("lengths,counts,span,M", TABLE_EDGES)
def test_table_edges(pkg, oracle, lengths, counts, span, M):
    times, _ = _three_way(pkg, oracle, lengths, counts, span, M, seed=sum(counts) % 9973)
    _assert_folded(times)


@pytest.mark.parametrize("M", [1, 50])
@pytest.mark.parametrize("L,n", [(3_300, 200_037), (40_000, 400_013)])
def test_settling_in_the_walks_tail(pkg, oracle, L, n, M):
    """genomes small enough that every chunk of 1 024 records holds colliding positions, so quotas run out inside chunks:
    3 300 positions (207 ranges of 16, sixty reads a position, a chunk or two per range) and 40 000 positions (157
    ranges of 256, a wave-slot per pass and range: four chunks, the last one partial -- wave-slots % 16 != 0).  No range
    holds more than 1 / 24 of the reads, so the ranked route is kept"""
    times, st = _three_way(pkg, oracle, [L], [n], 30, M, seed=M + L)
    assert st.sort_passes == 1
    _assert_folded(times)


def test_near_uniform_route_ranks_through_the_same_walk(pkg, oracle):
    """1 % of the reads clipped, deep enough for path 3: its head runs again with a filter (the same two table kernels)
    and its ranking is the same walk"""
    rng = np.random.default_rng(3)
    s, e = pkg.reads_gen(pkg.KIND_UNIFORM, 125_000, 30_000, seed=11)
    s = s.astype(np.int64); e = e.astype(np.int64)
    pick = rng.random(s.size) < 0.01
    clip = rng.integers(1, 40, size=s.size)
    front = rng.random(s.size) < 0.5
    s = np.where(pick & front, s + clip, s).astype(np.uint32)
    e = np.where(pick & ~front, e - clip, e).astype(np.uint32)
    with pkg.Solver(0) as sv:
        sv.set_profiling(True)
        with sv.options(pass_major=1):
            pm = sv.solve(s, e, 30_000, 100)
        times, st = sv.kernel_times(), sv.last_stats
        with sv.options(pass_major=-1):
            rm = sv.solve(s, e, 30_000, 100)
    assert st.path == pkg.PATH_NEAR_UNIFORM
    assert np.array_equal(pm, rm) and np.array_equal(pm, oracle.solve(s, e, 30_000, 100))
    assert "k_pm_walk" in times and "k_pm_settle" not in times and "scan_radix_hist(3 kernels)" not in times
    assert times["k_pm_row_sums"][0] == times["k_pm_tables"][0] >= 1


@pytest.mark.parametrize("span", [31, 32, 120, 150])
def test_quotas_from_the_event_sweep(pkg, oracle, span):
    """five contigs of ragged lengths, ranges that straddle their borders; 354 434 positions with six reads starting at
    each on average (fewer than ln 2 / span of the start positions hold no read, or the host takes the block-scan
    pipeline): mean depth 6 x span >= 186, M = 3 keeps it >= 11 x M, so the event-driven sweep runs and the walk takes
    its quotas from the sweep's own output -- against the same call through k_sweep_expand.  (Span 31 is below the
    event-driven form's shortest span, 32: there the block-scan pipeline runs and the walk reads selend[] - boff[]; the
    three-way comparison holds all the same.)"""
    lengths = [70_001, 33_333, 250_000, 1_000, 100]
    counts = [420_000, 200_000, 1_500_000, 6_000, 600 if span <= 100 else 0]   # (one span: no reads on a contig shorter than it)
    assert sum(counts) * span >= 11 * 3 * sum(lengths)
    times, _ = _three_way(pkg, oracle, lengths, counts, span, 3, seed=span)
    _assert_folded(times)
    times2, _ = _three_way(pkg, oracle, lengths, counts, span, 3, seed=span, keep_expand=1)
    if span >= 32:
        assert "k_sweep_uniform_ev" in times and "k_sweep_expand" not in times
        assert "k_sweep_uniform_ev" in times2 and "k_sweep_expand" in times2
    else:
        assert "k_sweep_uniform_ev" not in times
