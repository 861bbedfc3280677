"""The by-contig family's characterisation grid (tests/by_contig_grid.py): every case gives the outcome recorded in
tests/golden/by_contig_grid.json -- the hashes of its output arrays, the integer fields of its stats, or its error and
the caller's buffer afterwards, and the sequence of its timing spans."""
import json
import os

import pytest

import by_contig_grid as grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = json.load(open(os.path.join(ROOT, "tests", "golden", "by_contig_grid.json")))

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", grid.SMALL_CASES, ids=grid.key_of)
def test_a_small_case_does_what_it_did_before(pkg, case):
    want = RECORD[grid.key_of(case)]
    if case[0] == "budget" and case[1] == "device" and case[2] in grid.REFUSALS:
        assert want["buffer_untouched"]  # a refused budget call leaves the caller's mask alone
    if case[2] in grid.REFUSALS:
        assert "error" in want
    assert grid.outcome(pkg, case) == want


@pytest.mark.parametrize("case", grid.BATCH_CASES, ids=grid.key_of)
def test_a_case_of_several_batches_does_what_it_did_before(pkg, case):
    assert grid.outcome(pkg, case) == RECORD[grid.key_of(case)]
