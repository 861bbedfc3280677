"""downsample_bam's characterisation grid (tests/downsample_grid.py), the cases that run: each returns the counts, writes
the records (hashed after decoding) and the report texts recorded in tests/golden/downsample_grid.json."""
import json
import os

import pytest

import downsample_grid as grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = json.load(open(os.path.join(ROOT, "tests", "golden", "downsample_grid.json")))
RAN = [combo for combo in grid.CASES if "returned" in RECORD[grid.key_of(combo)]]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return grid.make_inputs(str(tmp_path_factory.mktemp("grid_inputs")))


@pytest.mark.gpu
@pytest.mark.parametrize("combo", RAN, ids=grid.key_of)
def test_a_case_that_ran_writes_what_it_wrote_before(pkg, inputs, tmp_path, combo):
    assert grid.outcome(pkg, combo, inputs, str(tmp_path)) == RECORD[grid.key_of(combo)]
