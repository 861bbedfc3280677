"""k_pm_prepare_sort's flat write-out (csrc/kernels/pass_major.inc.hip) against the host model, through the stage driver
(tests/cpp/pm_stage_driver.hip) and pm_stage_compare.compare_stage_dump -- every producer buffer, the tables and the
stages behind them, the canary outside the slices' padded groups included.  The unfiltered producer stages a pass whose
digits span at most 32 ranges in the padded layout it has in memory and copies the stage out as one run; every other
pass keeps the slice-by-slice write-out.  The cases sit where the padded pass is shortest and longest (8 192 and 10 176
slots of the stage's 10 240), at the edges of a group of 64 and of a pass, and on both sides of the choice of form.
Which form a pass takes is worked out here from the plan (the digit interval of the pass's contigs), not read from the
kernel; tests/pm_flat_writeout_model.py restates the mapping on the host."""
import zlib

import numpy as np
import pytest

import pass_major_model as pm
import pm_flat_writeout_model as fw
import pm_stage_compare as sc
from pm_stage_compare import make_case
from test_gpu_pm_stages import grid_driver, run_case, stage_driver  # noqa: F401  (fixtures; one trouble list for both files)

pytestmark = pytest.mark.gpu
PASS = pm.PASS
SPAN = 5
FLAT, SLICES, BOTH = {True}, {False}, {True, False}


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
        assert starts.size == n
        return make_case(name, [length], [n], starts, _ends(starts, [length], np.zeros(n, np.int64)), seed=_seed(name), **kw)
    return build


def _random(length):
    return lambda rng, i: rng.integers(0, length, size=i.size)


def _contigs(name, lengths, counts, wish=-1, expect_aligned=None):
    def build():
        rng = np.random.default_rng(_seed(name))
        contig = np.repeat(np.arange(len(lengths)), counts)
        starts = np.concatenate([rng.integers(0, L, size=k) for L, k in zip(lengths, counts)])
        return make_case(name, lengths, counts, starts, _ends(starts, lengths, contig), wish=wish, expect_aligned=expect_aligned,
                         seed=_seed(name))
    return build


def _most_padding(light_at):
    """one pass of 31 digits of 257 records and one of 225, in a random order of the reads: ptot = 10 176"""
    counts = [257] * 32
    if light_at is not None:
        counts[light_at] = 225
    else:
        counts[17] = 225
    return lambda rng, i: rng.permutation(np.repeat(np.arange(32), counts))


def _invalid(name):
    """one invalid read in the first pass and one in the last"""
    def build():
        rng = np.random.default_rng(_seed(name))
        n = 2 * PASS + 100
        starts = rng.integers(0, 32, size=n)
        ends = _ends(starts, [32], np.zeros(n, np.int64))
        starts[3], ends[3] = 4_000_000_000, 4_000_000_004      # beyond the contig: taken as its last position
        starts[n - 2], ends[n - 2] = ends[n - 2] + 1, starts[n - 2]   # start after end
        return make_case(name, [32], [n], starts, ends, stop_after="C", expect_bad=1, seed=_seed(name))
    return build


def _filtered(name):
    """the filtered producer keeps the unpadded stage (its exception corner lies behind it) and the slice write-out"""
    def build():
        rng = np.random.default_rng(_seed(name))
        n = 2 * PASS + 100
        starts = rng.integers(0, 32 - SPAN, size=n)
        ends = starts + SPAN - 1
        for i in (0, 63, 64, 1023, 1024, 5000, 5001, PASS - 1, PASS, 2 * PASS + 99):
            ends[i] -= 1 + (i % 3)
        return make_case(name, [32], [n], starts, ends, ell_reg=SPAN, seed=_seed(name))
    return build


def _cases():
    """name -> (case builder, the forms its passes take)"""
    cases = {}
    for n in (1, 63, 64, 65, PASS - 1, PASS, PASS + 1, 3 * PASS + 5):
        cases["size_%d" % n] = (_one_contig("flat_size_%d" % n, 32, n, _random(32)), FLAT)
    cases["no_padding"] = (_one_contig("flat_no_padding", 32, 2 * PASS, lambda rng, i: i % 32), FLAT)
    cases["one_digit_whole_pass"] = (_one_contig("flat_one_digit", 32, PASS, lambda rng, i: np.full(i.size, 7)), FLAT)
    cases["padding_of_1_and_63"] = (_one_contig("flat_pad_1_63", 32, PASS, lambda rng, i: np.where(i == 4321, 29, 6)), FLAT)
    cases["most_padding"] = (_one_contig("flat_most_padding", 32, PASS, _most_padding(None)), FLAT)
    cases["most_padding_light_digit_first"] = (_one_contig("flat_most_padding_first", 32, PASS, _most_padding(0)), FLAT)
    cases["most_padding_light_digit_last"] = (_one_contig("flat_most_padding_last", 32, PASS, _most_padding(31)), FLAT)
    cases["digits_0_and_31_only"] = (_one_contig("flat_ends_only", 32, PASS + 700, lambda rng, i: 31 * rng.integers(0, 2, size=i.size)), FLAT)
    cases["ranges_33_slice_form"] = (_one_contig("flat_ranges_33", 33, 2 * PASS + 40, _random(33)), SLICES)
    # contigs of 20 ranges of 128 positions: a pass inside one contig leaves flat, one that straddles two spans 40
    for wish, grid in ((-1, "global"), (1, "aligned")):
        cases["both_forms_in_one_call_" + grid] = (
            _contigs("flat_both_forms_" + grid, [2560] * 8, [PASS + 500, PASS, PASS + 77, 100, 3000, PASS, 5, 2 * PASS],
                     wish=wish, expect_aligned=1 if wish > 0 else 0), BOTH)
    cases["two_contigs_a_pass"] = (_contigs("flat_two_contigs", [16, 16], [5000, 6000]), FLAT)
    cases["three_contigs_ragged"] = (_contigs("flat_three_contigs", [10, 12, 9], [3000, 9000, 7000]), FLAT)
    cases["invalid_first_and_last_pass"] = (_invalid("flat_invalid"), FLAT)
    cases["filtered_keeps_the_slice_form"] = (_filtered("flat_filtered"), SLICES)
    return cases


CASES = _cases()


def pass_forms(case):
    """per pass: does it leave flat?  The producer's rule on the plan's grid: the unfiltered producer, and the ranges
    from the first position of the pass's first contig to the last position of its last are at most 32"""
    g, shift, roff = case["grid"], case["shift"], case["roff"]
    vbase, lengths = np.asarray(g["vbase"], np.int64), case["lengths"]
    contig = pm.contig_of_reads(roff)
    n = contig.size
    forms = []
    for base in range(0, n, PASS):
        c_first, c_last = int(contig[base]), int(contig[min(n, base + PASS) - 1])
        d_lo = int(vbase[c_first]) >> shift
        d_hi = (int(vbase[c_last]) + max(int(lengths[c_last]) - 1, 0)) >> shift
        forms.append(case["ell_reg"] == 0 and fw.takes_flat_form(d_lo, d_hi))
    return forms


@pytest.mark.parametrize("name", list(CASES))
def test_flat_writeout_buffers_match_the_model(name, stage_driver, grid_driver, tmp_path):
    build, want_forms = CASES[name]
    case = sc.plan_case(build(), grid_driver)
    forms = pass_forms(case)
    assert set(forms) == want_forms, "the case's passes take the forms %s" % forms
    m = sc.model_of(case)
    ptot = m["cntp"].sum(axis=0)[:len(forms)]
    assert all(int(p) <= fw.STAGE_WORDS for p, flat in zip(ptot, forms) if flat)
    if name == "one_digit_whole_pass":
        assert ptot.tolist() == [PASS]
    if name == "padding_of_1_and_63":
        assert ptot.tolist() == [PASS + 64] and sorted((m["lstw"][:, 0] >> 16)[[6, 29]].tolist()) == [1, PASS - 1]
    if name.startswith("most_padding"):
        assert ptot.tolist() == [10176]
    if name == "no_padding":
        assert ptot.tolist() == [PASS, PASS] and ((m["lstw"][:32, :2] >> 16) == 256).all()
    if name == "ranges_33_slice_form":
        assert case["shift"] == 0 and ((case["ltot"] - 1) >> case["shift"]) + 1 == 33
    dump = run_case(stage_driver, case, tmp_path)
    sc.compare_stage_dump(case, dump)
    assert dump["returncode"] == 0
