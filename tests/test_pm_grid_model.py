"""The pass-major form's contig-aligned range grid on the CPU: the host's plan (csrc/pm_grid_plan.h, compiled with g++
alone) feeds tests/pass_major_model.py -- untouched -- the reads' starts on the grid's axis, and the model's own asserts
keep every index in bounds.  Mapped back through the per-range tables (pos0, live) the bucket counts must be the
genome's and the keep mask of walk + settle "the S(p) lowest read indices of every start position p" for random quotas,
under both grids; the grids' balance at cfg4's shape is what the issue measured (heaviest range over the median: 1.013
aligned, 1.154 global), and the chooser takes the aligned grid there."""
import numpy as np
import pytest

import pass_major_model as pm
import pm_grid_model as gm


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return gm.build_driver(tmp_path_factory.mktemp("pm_grid_plan"))


_expected_mask = pm.expected_mask


CASES = [
    # lengths, reads, shift
    ([4096, 8192, 2048], [9_000, 20_011, 5_000], 6),                          # every contig a whole number of ranges
    ([70_001, 33_333, 250_000, 1_000], [9_000, 20_011, 30_000, 5], 11),       # a contig shorter than one range
    ([5_000, 0, 50_000, 5_000, 0], [0, 0, 25_000, 3_000, 0], 8),              # contigs of zero length and of zero reads
    ([100_000, 30_000], [2 * 8192 + 77, 8192 + 5], 9),                        # passes straddle the border, the last is partial
]


@pytest.mark.parametrize("want", [-1, 1])
@pytest.mark.parametrize("lengths,reads,shift", CASES)
def test_round_trip_through_the_grid_tables(driver, lengths, reads, shift, want):
    rng = np.random.default_rng(len(lengths) * 100 + shift)
    g = gm.plan(driver, lengths, reads, shift, want)
    assert g["aligned"] == (1 if want > 0 else 0)
    lengths = np.asarray(lengths, np.int64)
    poff = np.concatenate([[0], np.cumsum(lengths)])
    ltot, width, n_ranges = int(poff[-1]), 1 << shift, g["n_ranges"]
    contig = np.repeat(np.arange(len(lengths)), reads)
    local = np.concatenate([rng.integers(0, max(int(L), 1), size=int(k)) for L, k in zip(lengths, reads)])
    gs = (poff[contig] + local).astype(np.int64)                   # the genome's positions
    vs = gm.virtual_starts(local, contig, lengths, g["vbase"])     # the grid's axis
    n = vs.size
    pos0, live = g["pos0"], g["live"]
    # the ranges tile the genome: every position in exactly one range, the last range ends where the genome does
    covered = np.zeros(ltot, np.int64)
    for d in range(n_ranges):
        assert 0 <= live[d] <= width and pos0[d] + live[d] <= ltot
        covered[pos0[d]:pos0[d] + live[d]] += 1
        if live[d] and g["contig"][d] != gm.NO_CONTIG:
            c = g["contig"][d]
            assert poff[c] <= pos0[d] and pos0[d] + live[d] <= poff[c + 1]
    assert np.all(covered == 1)
    if want > 0:
        assert n_ranges == int(sum((L + width - 1) // width for L in lengths)) and np.all(g["contig"][live > 0] != gm.NO_CONTIG)
        assert pos0[n_ranges - 1] + live[n_ranges - 1] == ltot     # (boff[ltot] is nobody's position: written apart)
    keys16, idx16, cntp, lstw = pm.producer(vs, shift, n_ranges)
    pitch, stride = pm.pitch_for(n), pm.stride_for(n_ranges)
    Tp = pm.scan_table(cntp)
    desc, range_start = pm.descriptors(Tp, lstw, n, n_ranges)
    assert int(range_start[-1]) == n
    quota = rng.choice([0, 0, 1, 1, 2, 5, 1 << 20], size=ltot)
    counts = np.zeros(ltot, np.int64)
    mask = np.zeros(n, bool)
    kept_total, ambs = 0, {}
    for d in range(n_ranges):
        g0, n_ws = pm.range_wave_slots(Tp, pitch, d)
        if n_ws == 0:
            assert range_start[d + 1] == range_start[d]
            continue
        hist = pm.offsets(keys16, desc, Tp, pitch, d, shift, stride)
        assert hist[live[d]:].sum() == 0                            # no key beyond the range's live positions
        counts[pos0[d]:pos0[d] + live[d]] += hist[:live[d]]
        q = np.zeros(width, np.int64)
        q[:live[d]] = quota[pos0[d]:pos0[d] + live[d]]              # the walk's prologue: quotas for i < live only
        ambs[d], kept = pm.walk(keys16, idx16, desc, Tp, pitch, d, q, stride, n, mask, rng)
        kept_total += kept
    assert np.array_equal(counts, np.bincount(gs, minlength=ltot))
    for d, amb in ambs.items():
        kept_total += pm.settle(amb, keys16, idx16, desc, Tp, pitch, d, n, stride, mask)
    want_mask = _expected_mask(gs, quota)
    assert np.array_equal(mask, want_mask) and kept_total == int(want_mask.sum())


def test_a_start_beyond_its_contig_keeps_its_digit_inside_the_grid(driver):
    """invalid starts (the call fails) are clamped into their contig; a read given for a contig without positions lands
    on a key of the grid all the same"""
    lengths, reads, shift = [1000, 0, 3000, 0], [10, 3, 10, 2], 7
    for want in (-1, 1):
        g = gm.plan(driver, lengths, reads, shift, want)
        contig = np.repeat(np.arange(4), reads)
        vs = gm.virtual_starts(np.full(contig.size, 1 << 20), contig, lengths, g["vbase"])
        assert (vs >> shift).max() < g["n_ranges"]
        assert np.all(np.diff(g["vbase"]) >= 0)


def test_balance_at_the_benchmark_shape_and_the_chooser(driver):
    """cfg4's shape -- 8 contigs of 10^6 positions, ranges of 2^15 -- at 120 passes per contig, uniform starts"""
    rng = np.random.default_rng(4)
    lengths, shift = [1_000_000] * 8, 15
    reads = [120 * gm.PASS + 1234] * 8
    contig = np.repeat(np.arange(8), reads)
    local = rng.integers(0, 1_000_000, size=contig.size)
    ratio = {}
    for want in (-1, 1):
        g = gm.plan(driver, lengths, reads, shift, want)
        slots = gm.wave_slots_per_range(gm.virtual_starts(local, contig, lengths, g["vbase"]), shift, g["n_ranges"])
        ratio[want] = slots.max() / np.median(slots[slots > 0])
        assert g["n_ranges"] == (248 if want > 0 else 245)
    print("heaviest range over the median: aligned %.4f global %.4f" % (ratio[1], ratio[-1]))
    assert ratio[1] <= 1.03 and ratio[-1] >= 1.10
    auto = gm.plan(driver, lengths, [12_500_000] * 8, shift, 0)      # cfg4 itself
    assert auto["aligned"] == 1 and auto["n_ranges"] == 248 and auto["heaviest_aligned"] < auto["heaviest_global"]


def test_the_chooser_keeps_the_global_grid_where_aligned_does_not_pay(driver):
    # 60 contigs of 1 090 positions at shift 8: 300 aligned ranges -- more than one partition level holds
    g = gm.plan(driver, [1090] * 60, [6_667] * 60, 8, 1)
    assert g["aligned"] == 0 and g["aligned_ranges"] == 300 and g["n_ranges"] == (60 * 1090 >> 8) + 1
    # one contig: the grids are the same grid, nothing is strictly lighter
    g = gm.plan(driver, [1_000_000], [2_000_000], 12, 0)
    assert g["aligned"] == 0 and g["heaviest_aligned"] == g["heaviest_global"]
    # ... and switched off
    assert gm.plan(driver, [1_000_000] * 8, [12_500_000] * 8, 15, -1)["aligned"] == 0
