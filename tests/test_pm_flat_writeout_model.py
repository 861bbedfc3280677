"""The flat write-out's host restatement (tests/pm_flat_writeout_model.py: stage slot = padded base + stable rank, then
the flat copy of [0, ptot)) against the pass-major host model (tests/pass_major_model.py): equal on every record slot,
nothing written outside the slices' padded groups, and the padded pass inside the stage whenever its digits span at
most 32 ranges."""
import numpy as np
import pytest

import pass_major_model as pm
import pm_flat_writeout_model as fw

PASS = pm.PASS


def _worst_padding(heavy_at):
    """31 digits of 257 records (63 slots of padding each) and one of 225 (31): ptot = 10 176"""
    counts = [257] * 32
    counts[heavy_at] = 225
    return np.repeat(np.arange(32), counts)


def _ragged(seed, n, shift, d_lo, width):
    """reads whose digits lie in [d_lo, d_lo + width), each pass on its own ragged subset of them"""
    rng = np.random.default_rng(seed)
    g = np.empty(n, np.int64)
    for lo in range(0, n, PASS):
        k = min(PASS, n - lo)
        live = rng.choice(width, size=rng.integers(1, width + 1), replace=False)
        weights = rng.random(live.size) ** 3 + 1e-3
        d = d_lo + rng.choice(live, size=k, p=weights / weights.sum())
        g[lo:lo + k] = (d << shift) | rng.integers(0, 1 << shift, size=k)
    return g


CASES = {
    "one_read": (np.array([5]), 0, 32, (0, 31)),
    "ragged_shift0": (_ragged(1, 3 * PASS + 5, 0, 0, 32), 0, 32, (0, 31)),
    "ragged_shift7_high_digits": (_ragged(2, 5 * PASS - 77, 7, 224, 32), 7, 256, (224, 255)),
    "ragged_narrow_interval": (_ragged(3, 2 * PASS + 63, 4, 10, 3), 4, 40, (10, 12)),
    "worst_padding_heavy_first": (_worst_padding(0), 0, 32, (0, 31)),
    "worst_padding_heavy_last": (_worst_padding(31), 0, 32, (0, 31)),
    "worst_padding_shuffled": (np.random.default_rng(4).permutation(_worst_padding(13)), 0, 32, (0, 31)),
    "no_padding": (np.arange(2 * PASS) % 32, 0, 32, (0, 31)),
    "one_digit": (np.full(PASS, 7), 0, 32, (0, 31)),
    "padding_of_1_and_63": (np.concatenate([np.full(PASS - 1, 3), [9]]), 0, 32, (0, 31)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_flat_writeout_is_the_models_producer_on_every_record_slot(name):
    g, shift, n_ranges, (d_lo, d_hi) = CASES[name]
    g = np.asarray(g, np.int64)
    keys16, idx16, cntp, lstw = pm.producer(g, shift, n_ranges)
    fk, fi, written, ptots = fw.producer_flat(g, shift, n_ranges, lambda P: (d_lo, d_hi))
    stride = pm.stride_for(n_ranges)
    rec = np.zeros(keys16.size, bool)
    grp = np.zeros(keys16.size, bool)
    for d, P in zip(*np.nonzero(lstw >> 16)):
        at = int(P) * stride + int(lstw[d, P] & 0xFFFF) * 64
        rec[at:at + int(lstw[d, P] >> 16)] = True
        grp[at:at + int(cntp[d, P])] = True
    assert rec.sum() == g.size
    assert np.array_equal(fk[rec], keys16[rec]) and np.array_equal(fi[rec], idx16[rec])
    # inside padded groups only -- and all of them, the padding included: a pass's groups are one run from P stride on
    assert np.array_equal(written, grp)
    assert (fk[~written] == 0xFFFF).all() and (fi[~written] == 0xFFFF).all()
    assert (ptots == cntp.sum(axis=0)[:ptots.size]).all()
    assert (ptots % 64 == 0).all() and ptots.max() <= fw.STAGE_WORDS


def test_worst_padding_sits_at_the_top_of_the_stage():
    _, ptot, pbase, c = fw.stage_pass(_worst_padding(31), np.zeros(PASS, np.int64))
    assert ptot == 10176 == 31 * 320 + 256 and ptot <= fw.STAGE_WORDS
    assert (pbase % 64 == 0).all() and c.sum() == PASS


def test_any_pass_of_at_most_32_digits_fits_the_stage():
    # the bound itself: k occupied digits pad at most 63 slots each, and 8 192 records leave no room for more padding
    # than 63 k; random count vectors come nowhere near it, so the extremal ones are built
    for k in range(1, 33):
        counts = np.full(k, 1, np.int64)            # as many slices as possible one past a multiple of 64
        spare = PASS - k
        counts += 64 * (spare // (64 * k))
        counts[0] += spare - 64 * k * (spare // (64 * k))
        assert counts.sum() == PASS
        _, ptot, _, _ = fw.stage_pass(np.repeat(np.arange(k), counts), np.zeros(PASS, np.int64))
        assert ptot <= PASS + 63 * k <= fw.STAGE_WORDS
    rng = np.random.default_rng(7)
    for _ in range(50):
        n = int(rng.integers(1, PASS + 1))
        digits = rng.integers(0, 32, size=n) + int(rng.integers(0, 225))
        _, ptot, _, _ = fw.stage_pass(digits, np.zeros(n, np.int64))
        assert ptot <= fw.STAGE_WORDS


def test_33_digits_keep_the_slice_write_out():
    assert fw.takes_flat_form(0, 31) and fw.takes_flat_form(224, 255) and fw.takes_flat_form(9, 9)
    assert not fw.takes_flat_form(0, 32) and not fw.takes_flat_form(5, 4)
    g = np.arange(PASS) % 33
    _, _, written, ptots = fw.producer_flat(g, 0, 33, lambda P: (0, 32))
    assert ptots.tolist() == [-1] and not written.any()
