"""The per-lane-count rank (tests/pm_lane_rank_model.py, the host restatement of csrc/kernels/pm_lane_rank.inc.hip)
against a stable argsort over the same digits: the in-lane count, plus the lane prefix, plus the wave prefix is the
read's position in the pass sorted stably by digit."""
import numpy as np
import pytest

import pm_lane_rank_model as lr


def _check(digits, d_lo, n_pairs):
    digits = np.asarray(digits, np.int64)
    pos = lr.rank_pass(digits, d_lo, n_pairs)
    order = np.argsort(digits, kind="stable")
    want = np.empty(digits.size, np.int64)
    want[order] = np.arange(digits.size)
    assert np.array_equal(pos, want)


@pytest.mark.parametrize("count", [1, 15, 16, 17, 1023, 1024, 1025, 8191, 8192])
def test_random_digits_at_the_ownership_edges(count):
    rng = np.random.default_rng(count)
    _check(7 + rng.integers(0, 32, size=count), 7, 16)


def test_one_digit_fills_every_counter_to_its_maximum():
    for rel in (0, 1, 30, 31):
        _check(np.full(8192, 100 + rel), 100, 16)
    old, words, totals = lr.wave_words(np.full(1024, 5), np.ones(1024, bool))
    assert totals[5] == 1024 and totals.sum() == 1024
    assert (words[2] >> 16).max() == 1008 and old.max() >> 16 == 15


def test_alternating_digits():
    i = np.arange(8192)
    _check(3 + (i & 1), 3, 1)                   # both fields of one word, per read
    _check(3 + 2 * (i & 1), 3, 2)               # two words, per read
    _check(3 + ((i >> 4) & 1), 3, 1)            # per lane: a lane holds one digit only
    _check(3 + 31 * ((i >> 4) & 1), 3, 16)


def test_fewer_pairs_than_sixteen_and_odd_digit_counts():
    rng = np.random.default_rng(5)
    for n_digits in (1, 2, 3, 7, 8, 9, 31, 32):
        _check(200 + rng.integers(0, n_digits, size=5000), 200, (n_digits + 1) // 2)


def test_sorted_digits():
    rng = np.random.default_rng(6)
    _check(np.sort(rng.integers(0, 32, size=8192)), 0, 16)
    _check(np.sort(rng.integers(0, 32, size=8192))[::-1], 0, 16)
