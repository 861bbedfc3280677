"""The plain solve's characterisation grid (tests/solve_route_grid.py): every case gives the outcome recorded in
tests/golden/solve_route_grid.json -- per call the hash of its mask, the integer fields of its stats, or its error and
the caller's buffer afterwards, and the sequence of its timing spans -- and the record itself is of the routes the
cases are named for."""
import json
import os

import pytest

import solve_route_grid as grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = json.load(open(os.path.join(ROOT, "tests", "golden", "solve_route_grid.json")))["cases"]

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(grid.CASES))
def test_a_case_does_what_it_did_before(pkg, name):
    want = RECORD[name]
    assert grid.route_misses(name, want) == []
    if name in grid.SAME_AS_BLOCKING:
        blocking, part = grid.SAME_AS_BLOCKING[name]
        assert want == RECORD[blocking][part]  # begin / end does what the blocking call does
    assert all(call.get("guard_intact", True) for call in want)
    assert grid.outcome(pkg, name) == want
