"""The two per-range kernels of the pass-major form around their loops (csrc/kernels/pass_major.inc.hip): k_pm_offsets
with its first requests ahead of the clear and 16-byte position loads, eight wave-slots a request; k_pm_walk's quota
prologue on the event-driven sweep's output (a range's positions in one round, the block by multiply and shift --
csrc/pm_div.h) and its settling tail (list entries up front, the next groups' requests on their way while a group is
walked, a group's records marked one group later).

Offsets and tail: tests/cpp/pm_stage_driver against the host model, as tests/test_gpu_pm_stages.py does, on cases built
for the edges of those loops; each case states what it must contain and the test checks that on the model before the
device is asked.  The walk's prologue takes its quotas from the event-driven sweep only inside a solve, so those cases
solve end to end -- pass-major form, event-driven sweep forced -- against the range-major form and the oracle.  (The
event-driven sweep's shortest span is 32: for spans 1, 2 and 3 the host takes the block-scan pipeline whatever is forced
and the walk reads selend[] - boff[]; the three-way comparison holds all the same, and the division itself is gone
through for those divisors in tests/test_pm_div.py.)"""
import numpy as np
import pytest

import pass_major_model as pm
import pm_grid_model as gm
import pm_stage_compare as sc
from pm_stage_cases import _spans
from test_gpu_pm_stages import run_case, stage_driver  # noqa: F401  (the driver's fixture and its one-process runner)

pytestmark = pytest.mark.gpu
K_U = 4            # position requests of one round of k_pm_offsets (QMCP_PM_OFFSETS_U) ...
REC = 8            # ... of REC wave-slots each (QMCP_PM_OFFSETS_REC: a lane loads REC records)
WAVES = 16         # waves of a per-range workgroup


@pytest.fixture(scope="module")
def grid_driver(tmp_path_factory):
    return gm.build_driver(tmp_path_factory.mktemp("pm_grid_plan_trips"))


# --------------------------------------------------------------------------------------------- cases through the driver
def _ranged_case(name, length, per_range, stop_after, seed, pairs=False):
    """one contig; per_range: {range: reads} -- the reads of a range follow each other in read order, ranges ascending,
    at random positions of the range (pairs: read 2 i and 2 i + 1 of a range on position i of it: consecutive indices
    on one position)"""
    shift = pm.range_shift_for(length)
    width = 1 << shift
    rng = np.random.default_rng(seed)
    starts = []
    for r in sorted(per_range):
        k = int(per_range[r])
        live = min(width, length - r * width)
        assert live >= 1
        if pairs:
            assert k % 2 == 0 and k // 2 <= live
            s = r * width + np.repeat(np.arange(k // 2), 2)
        else:
            s = r * width + rng.integers(0, live, size=k)
        starts.append(s)
    starts = np.concatenate(starts)
    contig = np.zeros(starts.size, np.int64)
    return sc.make_case(name, [length], [starts.size], starts, _spans(starts, [length], contig, 30), stop_after=stop_after,
                        seed=seed)


def _wave_slots(case):
    """-> per range of the grid: (wave-slots, records in the last one)"""
    m = sc.model_of(case)
    out = []
    for d in range(m["n_ranges"]):
        g0, n_ws = pm.range_wave_slots(m["Tp"], m["pitch"], d)
        last = pm.unpack(m["desc"][g0 + n_ws - 1], m["stride"])[1] if n_ws else 0
        out.append((n_ws, int(last)))
    return out


def test_offsets_round_edges(stage_driver, grid_driver, tmp_path):
    """2 045 positions: 256 ranges of 8, the last with 5 live positions (live < 1 024; the range that writes boff[ltot]).
    Ranges with 0, 1, 3, 4 and 5 wave-slots; ranges whose every wave has 1, kU - 1, kU, kU + 1, 2 kU and 2 kU + 1
    requests of eight wave-slots (128 x wave-slots: x requests a wave) -- either side of one round and of two -- beside
    waves with none (the ranges of a few wave-slots); a last wave-slot of 1 record and one of 64"""
    per = {1: 64, 2: 192, 3: 256, 4: 320}
    for i, x in enumerate((1, K_U - 1, K_U, K_U + 1, 2 * K_U, 2 * K_U + 1)):
        per[10 + i] = WAVES * REC * x * 64         # 128 x wave-slots = 16 x requests
    per[200] = 65                                  # behind them: its second wave-slot holds one record
    per[255] = 3
    case = sc.plan_case(_ranged_case("offsets_round_edges", 2045, per, "C", 11), grid_driver)
    assert case["shift"] == 3 and int(case["grid"]["n_ranges"]) == 256 and int(case["grid"]["live"][255]) == 5
    ws = _wave_slots(case)
    have = {n for n, _ in ws}
    assert {0, 1, 3, 4, 5} <= have
    assert {WAVES * REC * x for x in (1, K_U - 1, K_U, K_U + 1, 2 * K_U, 2 * K_U + 1)} <= have
    assert any(n >= 2 and last == 1 for n, last in ws) and any(n >= 1 and last == 64 for n, last in ws)
    requests_per_wave = {((n + REC - 1) // REC + WAVES - 1 - w) // WAVES for n, _ in ws for w in range(WAVES)}
    assert {0, 1, K_U - 1, K_U, K_U + 1, 2 * K_U, 2 * K_U + 1} <= requests_per_wave
    dump = run_case(stage_driver, case, tmp_path)
    sc.compare_stage_dump(case, dump)
    assert dump["returncode"] == 0


def test_offsets_live_not_a_multiple_of_1024(stage_driver, grid_driver, tmp_path):
    """1 046 000 positions: 256 ranges of 4 096, the last with 1 520 live positions (not a multiple of the workgroup's
    1 024 threads); 20 000 reads anywhere, so most ranges hold a wave-slot or two and some none"""
    rng = np.random.default_rng(12)
    L, n = 1_046_000, 20_000
    starts = rng.integers(0, L, size=n)
    case = sc.make_case("offsets_live_1520", [L], [n], starts, _spans(starts, [L], np.zeros(n, np.int64), 30), stop_after="C",
                        seed=12)
    case = sc.plan_case(case, grid_driver)
    assert case["shift"] == 12 and int(case["grid"]["live"][255]) == 1520
    dump = run_case(stage_driver, case, tmp_path)
    sc.compare_stage_dump(case, dump)
    assert dump["returncode"] == 0


def _listed_groups(case, quota):
    """-> per range: the (chunk, position, skip) groups the walk lists under this quota vector (the model's walk)"""
    m = sc.model_of(case)
    shift, width = case["shift"], 1 << case["shift"]
    out = []
    for d in range(m["n_ranges"]):
        q = np.zeros(width, np.int64)
        pos0, live = int(case["grid"]["pos0"][d]), int(case["grid"]["live"][d])
        q[:live] = quota[pos0:pos0 + live]
        amb, _ = pm.walk(m["keys16"], m["idx16"], m["desc"], m["Tp"], m["pitch"], d, q, m["stride"], m["n"],
                         np.zeros(m["n"], bool), np.random.default_rng(d))
        out.append(amb)
    return out


def test_tail_group_counts(stage_driver, grid_driver, tmp_path):
    """300 000 positions, ranges of 2 048; quota 1 everywhere.  Pairs of reads with consecutive indices on one position:
    a pair is a listed group with one record to pass over.  Ranges with 0 listed groups (single reads), 1, 31, 32, 33
    (a wave's two-at-a-time rounds of old: 16 x 2 - 1, 16 x 2, 16 x 2 + 1), 300, and 1 023, 1 024, 1 025 (a wave's 64
    list entries of one load: 16 x 64); the 1 025 pairs fill 33 wave-slots: the last groups lie in the third, partial
    chunk.  One position with 64 reads: 63 to pass over"""
    per = {0: 0, 1: 2, 2: 62, 3: 64, 4: 66, 5: 600, 6: 2046, 7: 2048, 8: 2050}
    base = _ranged_case("tail_pairs", 300_000, {r: k for r, k in per.items() if k}, "D", 13, pairs=True)
    width = 1 << pm.range_shift_for(300_000)
    assert width == 2048
    rng = np.random.default_rng(14)
    singles = 20 * width + rng.permutation(width)[:500]                 # range 20: 500 reads, no two on a position
    heap = np.full(64, 30 * width + 77)                                  # range 30: 64 reads on one position
    starts = np.concatenate([base["starts"].astype(np.int64), singles, heap])
    case = sc.make_case("tail_group_counts", [300_000], [starts.size], starts,
                        _spans(starts, [300_000], np.zeros(starts.size, np.int64), 30), seed=13)
    case = sc.plan_case(case, grid_driver)
    ones = np.ones(case["ltot"], np.uint32)
    case["quotas"] = [ones, case["quotas"][4]]                           # ... and "one short of enough": a skip of 1 everywhere
    groups = _listed_groups(case, ones)
    counts = [len(g) for g in groups]
    assert [counts[r] for r in (20, 1, 2, 3, 4, 5, 6, 7, 8, 30)] == [0, 1, 31, 32, 33, 300, 1023, 1024, 1025, 1]
    assert {skip for g in groups for _, _, skip in g} == {1, 63}
    n_ws8 = _wave_slots(case)[8][0]
    assert n_ws8 == 33 and max(c for c, _, _ in groups[8]) == 2          # a group in the last chunk, of one wave-slot
    dump = run_case(stage_driver, case, tmp_path)
    sc.compare_stage_dump(case, dump)
    assert dump["returncode"] == 0


# ----------------------------------------------------------------------- the walk's prologue on the event sweep's output
SWEEP_EVENTS = 3   # QMCP_SWEEP_EVENTS
RAGGED = [70_001, 33_335, 250_001, 1_001]   # multiples of none of 2, 3, 150, 255, 256
RAGGED_READS = [40_000, 20_000, 140_000, 1_000]


def _reads(rng, lengths, counts, span):
    ss, ee = [], []
    for L, k in zip(lengths, counts):
        a = rng.integers(0, int(L) - span + 1, size=int(k), dtype=np.uint32)
        ss.append(a); ee.append((a + np.uint32(span - 1)).astype(np.uint32))
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return np.concatenate(ss), np.concatenate(ee), np.array(lengths, np.uint32), offs


def _event_three_way(pkg, oracle, lengths, counts, span, M, seed, pm_grid=0):
    """pass-major form (event-driven sweep forced, whole contigs: no cut points, so nothing expands the sweep's output)
    == range-major form == oracle; -> kernel times and statistics of the pass-major solve"""
    s, e, lengths, offs = _reads(np.random.default_rng(seed), lengths, counts, span)
    with pkg.Solver(0) as sv:
        sv.set_profiling(True)
        with sv.options(pass_major=1, sweep=SWEEP_EVENTS, cut_points=-1, pm_grid=pm_grid):
            got = sv.solve(s, e, lengths, M, contig_read_offsets=offs)
        times, st = sv.kernel_times(), sv.last_stats
        with sv.options(pass_major=-1, sweep=SWEEP_EVENTS, cut_points=-1):
            rm = sv.solve(s, e, lengths, M, contig_read_offsets=offs)
    assert np.array_equal(got, rm)
    assert np.array_equal(got, oracle.solve(s, e, lengths, M, contig_read_offsets=offs))
    assert "k_pm_walk" in times
    if span >= 32:   # the walk took its quotas from the sweep's own output
        assert "k_sweep_uniform_ev" in times and "k_sweep_expand" not in times
    return times, st


@pytest.mark.parametrize("pm_grid", [1, -1], ids=["aligned", "global"])
@pytest.mark.parametrize("ell", [1, 2, 3, 150, 255, 256])
def test_event_quotas_by_span(pkg, oracle, ell, pm_grid):
    """four contigs whose lengths are multiples of none of the spans; on the global grid (pm_grid = -1) ranges straddle
    the contigs' borders and look every position's contig up"""
    assert ell == 1 or all(L % ell for L in RAGGED)
    _, st = _event_three_way(pkg, oracle, RAGGED, RAGGED_READS, ell, 3, seed=ell, pm_grid=pm_grid)
    assert st.pm_grid == pm_grid


def test_event_quotas_near_the_position_limit(pkg, oracle):
    """8 388 001 positions, 607 short of the form's 2^23: p - base runs up to 5 000 000 in the first contig, and the
    second one's base / (4 ell) is 8 333"""
    lengths = [5_000_001, 3_388_000]
    assert sum(lengths) < (1 << 23) and all(L % 150 for L in lengths)
    _event_three_way(pkg, oracle, lengths, [120_000, 80_000], 150, 3, seed=5)


@pytest.mark.parametrize("live", [1, 15, 16, 17, 16 * 1024 - 1, 16 * 1024 + 1])
def test_event_quotas_by_live(pkg, oracle, live):
    """one contig on the global grid, its last range with `live` positions: below, at and above the sixteen positions a
    thread has in flight, and either side of a whole round of the workgroup (16 x 1 024)"""
    width = 32 if live < 32 else 32768
    L = (200 if live < 32 else 128) * width + live
    assert pm.range_shift_for(L) == (5 if live < 32 else 15)
    span = 40 if live < 32 else 150
    _, st = _event_three_way(pkg, oracle, [L], [200_000], span, 3, seed=live, pm_grid=-1)
    assert st.pm_grid == -1
