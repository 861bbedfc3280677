"""The pass-major form's two range grids (csrc/pm_grid_plan.h; options(pm_grid=-1 / +1)): ranges cut on the genome's
global axis, where they straddle contig borders, or at the contigs' starts.  The keep mask must be bit-equal between the
grids, equal to the range-major form's (options(pass_major=-1)) and to the oracle's, and n_kept must match; stats.pm_grid
says which grid a call took.  Shapes: ragged contigs with one shorter than a range (shift 11, 176 aligned ranges);
contigs that are whole numbers of ranges (shift 6: the grand total boff[ltot] is then no range's position); reads on the
middle contig only; 60 short contigs, whose 300 aligned ranges do not fit one partition level -- the call falls back to
the global grid; the event-driven sweep, whose output the walk reads through the range's contig; a start beyond its
contig.  The grids' arithmetic has a host model: tests/test_pm_grid_model.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _reads(seed, lengths, counts, span):
    rng = np.random.default_rng(seed)
    ss, ee = [], []
    for L, k in zip(lengths, counts):
        sp = min(span, int(L))
        a = rng.integers(0, int(L) - sp + 1, size=int(k), dtype=np.uint32)
        ss.append(a); ee.append((a + np.uint32(sp - 1)).astype(np.uint32))
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return np.concatenate(ss), np.concatenate(ee), np.array(lengths, np.uint32), offs


def _four_way(pkg, oracle, lengths, counts, span, M, seed, **opts):
    """-> {grid option: (stats, kernel times)}; asserts global == aligned == range-major == oracle"""
    s, e, lengths, offs = _reads(seed, lengths, counts, span)
    want = oracle.solve(s, e, lengths, M, contig_read_offsets=offs)      # (packed: a bit per read)
    n_kept = int(np.unpackbits(want.view(np.uint8)).sum())
    out = {}
    with pkg.Solver(0) as sv:
        for grid in (-1, 1):
            sv.set_profiling(True)
            with sv.options(pass_major=1, pm_grid=grid, **opts):
                got = sv.solve(s, e, lengths, M, contig_read_offsets=offs)
            out[grid] = (sv.last_stats, sv.kernel_times())
            assert "k_pm_walk" in out[grid][1]
            assert np.array_equal(got, want), grid
            assert out[grid][0].n_kept == n_kept and out[grid][0].pm_heaviest_wave_slots > 0
        with sv.options(pass_major=-1, **opts):
            rm = sv.solve(s, e, lengths, M, contig_read_offsets=offs)
        assert sv.last_stats.pm_grid == 0 and sv.last_stats.n_kept == out[1][0].n_kept
    assert np.array_equal(rm, want)
    return out


def test_ragged_contigs_one_shorter_than_a_range(pkg, oracle):
    out = _four_way(pkg, oracle, [70_001, 33_333, 250_000, 1_000], [300_000, 200_011, 500_000, 40_005], 120, 60, seed=1)
    assert out[-1][0].pm_grid == -1 and out[1][0].pm_grid == 1


def test_contigs_of_whole_ranges_the_grand_total(pkg, oracle):
    out = _four_way(pkg, oracle, [4096, 8192, 2048], [85_000, 172_000, 43_000], 30, 50, seed=2)
    assert out[-1][0].pm_grid == -1 and out[1][0].pm_grid == 1


def test_reads_on_the_middle_contig_only(pkg, oracle):
    out = _four_way(pkg, oracle, [5_000, 50_000, 5_000], [0, 200_001, 0], 100, 25, seed=3)
    assert out[-1][0].pm_grid == -1 and out[1][0].pm_grid == 1


def test_too_many_aligned_ranges_fall_back_to_the_global_grid(pkg, oracle):
    """60 contigs of 1 090 positions, ranges of 256: five ranges a contig, 300 in all"""
    counts = [6_667] * 40 + [6_666] * 20
    assert sum(counts) == 400_000
    out = _four_way(pkg, oracle, [1_090] * 60, counts, 30, 50, seed=4)
    assert out[-1][0].pm_grid == -1 and out[1][0].pm_grid == -1


def test_quotas_from_the_event_sweep_through_the_ranges_contig(pkg, oracle):
    """six reads a position on average, span 120, M = 3: deep enough for the event-driven sweep, and the walk takes its
    quotas from the sweep's own output (no k_sweep_expand) -- per range through one contig on the aligned grid, through
    a search per position where a range of the global grid straddles a border"""
    out = _four_way(pkg, oracle, [70_001, 33_333, 250_000, 1_000], [420_000, 200_000, 1_500_000, 6_000], 120, 3, seed=5)
    for grid in (-1, 1):
        st, times = out[grid]
        assert st.path == 1 and st.pm_grid == grid
        assert "k_sweep_uniform_ev" in times and "k_sweep_expand" not in times


def test_a_start_beyond_its_contig_fails_the_call(pkg, oracle, solver):
    s, e, lengths, offs = _reads(6, [70_001, 33_333, 250_000, 1_000], [100_000, 60_000, 140_000, 2_000], 120)
    bad_s, bad_e = s.copy(), e.copy()
    bad_s[123_456] = 4_000_000_000      # (on the second contig)
    bad_e[123_456] = 4_000_000_100
    with solver.options(pass_major=1, pm_grid=1):
        with pytest.raises(pkg.QmcpError):
            solver.solve(bad_s, bad_e, lengths, 20, contig_read_offsets=offs)
        got = solver.solve(s, e, lengths, 20, contig_read_offsets=offs)
        assert solver.last_stats.pm_grid == 1
    assert np.array_equal(got, oracle.solve(s, e, lengths, 20, contig_read_offsets=offs))
