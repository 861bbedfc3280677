"""k_pm_prepare_sort's ranking by per-lane counts (csrc/kernels/pm_lane_rank.inc.hip) against the host model, through
the stage driver (tests/cpp/pm_stage_driver.hip) and pm_stage_compare.compare_stage_dump -- every producer buffer, the
tables and the stages behind them.  The form serves the unfiltered producer's passes whose digits span at most 32
ranges; the cases of tests/pm_stage_cases.py lie on one long contig (128 .. 255 ranges a pass) and take the ballot form.
Here a pass spans at most 32 ranges: a genome of 32 positions (shift 0: a position is a range), or several contigs of 32
ranges each with every pass inside one contig.  The model knows nothing of lanes: whichever form ranks a pass, the
buffers are the model's.  The cases sit at the edges of a lane's sixteen reads, a wave's 1 024 and a pass's 8 192."""
import zlib

import numpy as np
import pytest

import pass_major_model as pm
import pm_stage_compare as sc
from pm_stage_compare import make_case
from test_gpu_pm_stages import grid_driver, run_case, stage_driver  # noqa: F401  (fixtures; one trouble list for both files)

pytestmark = pytest.mark.gpu
PASS = pm.PASS
SPAN = 5


def _seed(name):
    return zlib.crc32(name.encode()) & 0xFFFF


def _ends(starts, lengths, contig, span=SPAN):
    last = np.maximum(np.asarray(lengths, np.int64) - 1, 0)
    return np.minimum(np.asarray(starts, np.int64) + span - 1, last[contig])


def _one_contig(name, length, n, pick, **kw):
    """pick(rng, i) -> the starts of the reads i = 0 .. n - 1 on one contig of `length` positions"""
    def build():
        rng = np.random.default_rng(_seed(name))
        starts = np.asarray(pick(rng, np.arange(n)), np.int64)
        return make_case(name, [length], [n], starts, _ends(starts, [length], np.zeros(n, np.int64)), seed=_seed(name), **kw)
    return build


def _random(length):
    return lambda rng, i: rng.integers(0, length, size=i.size)


def _contigs(name, lengths, counts, wish=-1, expect_aligned=None, stop_after="D"):
    def build():
        rng = np.random.default_rng(_seed(name))
        contig = np.repeat(np.arange(len(lengths)), counts)
        starts = np.concatenate([rng.integers(0, L, size=k) for L, k in zip(lengths, counts)])
        return make_case(name, lengths, counts, starts, _ends(starts, lengths, contig), wish=wish, expect_aligned=expect_aligned,
                         stop_after=stop_after, seed=_seed(name))
    return build


def _invalid(name):
    """one invalid read in the first lane's share of pass 0 (wave 0, lane 0) and one in the last lane's (wave 7, lane 63)"""
    def build():
        rng = np.random.default_rng(_seed(name))
        n = PASS + 100
        starts = rng.integers(0, 32, size=n)
        ends = _ends(starts, [32], np.zeros(n, np.int64))
        starts[3], ends[3] = 4_000_000_000, 4_000_000_004      # beyond the contig: taken as its last position
        starts[PASS - 2], ends[PASS - 2] = ends[PASS - 2] + 1, starts[PASS - 2]   # start after end
        return make_case(name, [32], [n], starts, ends, stop_after="C", expect_bad=1, seed=_seed(name))
    return build


def _filtered(name):
    """the filtered producer keeps the ballot form and its lists in read-index order: a few exceptions in several waves"""
    def build():
        rng = np.random.default_rng(_seed(name))
        n = 2 * PASS + 100
        starts = rng.integers(0, 32 - SPAN, size=n)
        ends = starts + SPAN - 1
        for i in (0, 15, 16, 1023, 1024, 5000, 5001, PASS - 1, PASS, 2 * PASS + 99):
            ends[i] -= 1 + (i % 3)
        return make_case(name, [32], [n], starts, ends, ell_reg=SPAN, seed=_seed(name))
    return build


def _cases():
    cases = {}
    for n in (1, 15, 16, 17, 1023, 1024, 1025, PASS - 1, PASS, PASS + 1, 3 * PASS + 5):
        cases["size_%d" % n] = _one_contig("lane_size_%d" % n, 32, n, _random(32))
    n = 2 * PASS + 40
    cases["one_digit"] = _one_contig("lane_one_digit", 32, n, lambda rng, i: np.full(i.size, 7))
    cases["one_digit_odd_field"] = _one_contig("lane_one_digit_odd", 32, n, lambda rng, i: np.full(i.size, 31))
    cases["alternating_per_read"] = _one_contig("lane_alt_read", 32, n, lambda rng, i: 4 + (i & 1))
    cases["alternating_two_words"] = _one_contig("lane_alt_words", 32, n, lambda rng, i: 31 * (i & 1))
    cases["alternating_per_sixteen"] = _one_contig("lane_alt_sixteen", 32, n, lambda rng, i: 9 + 20 * ((i >> 4) & 1))
    cases["ranges_32"] = _one_contig("lane_ranges_32", 32, n, _random(32))
    cases["ranges_33_ballot_form"] = _one_contig("lane_ranges_33", 33, n, _random(33))
    cases["ranges_3"] = _one_contig("lane_ranges_3", 3, n, _random(3))
    cases["sorted"] = _one_contig("lane_sorted", 32, n, lambda rng, i: np.sort(rng.integers(0, 32, size=i.size)))
    # every pass inside one contig of exactly 32 ranges of 128 positions, under either grid
    for wish, grid in ((-1, "global"), (1, "aligned")):
        cases["contigs_of_32_ranges_" + grid] = _contigs("lane_contigs_32_" + grid, [4096] * 5, [PASS, 2 * PASS, PASS, PASS, PASS - 300],
                                                        wish=wish, expect_aligned=1 if wish > 0 else 0)
    # passes that hold two or three contigs whose digits together span at most 32 ranges
    cases["two_contigs_a_pass"] = _contigs("lane_two_contigs", [16, 16], [5000, 6000])
    cases["three_contigs_ragged"] = _contigs("lane_three_contigs", [10, 12, 9], [3000, 9000, 7000])
    # ... and passes of both forms in one call: eight contigs of 20 ranges, 40 or more where a pass straddles contigs
    cases["both_forms_in_one_call"] = _contigs("lane_both_forms", [2560] * 8, [PASS + 500, PASS, PASS + 77, 100, 3000, PASS, 5, 2 * PASS],
                                               wish=1, expect_aligned=1)
    cases["invalid_first_and_last_lane"] = _invalid("lane_invalid")
    cases["filtered_keeps_the_ballot_form"] = _filtered("lane_filtered")
    return cases


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_lane_form_buffers_match_the_model(name, stage_driver, grid_driver, tmp_path):
    case = sc.plan_case(CASES[name](), grid_driver)
    # (the ranges a pass's digits span, as the kernel counts them: first position of its first contig to the last
    #  position of its last -- 32 is the lane form's limit, 33 takes the ballot form)
    if name == "ranges_32":
        assert case["shift"] == 0 and ((case["ltot"] - 1) >> case["shift"]) + 1 == 32
    if name == "ranges_33_ballot_form":
        assert case["shift"] == 0 and ((case["ltot"] - 1) >> case["shift"]) + 1 == 33
    if name.startswith("contigs_of_32_ranges"):
        assert case["shift"] == 7 and all(int(L) >> 7 == 32 for L in case["lengths"])
    dump = run_case(stage_driver, case, tmp_path)
    sc.compare_stage_dump(case, dump)
    assert dump["returncode"] == 0
