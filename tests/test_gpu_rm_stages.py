"""Every range-major kernel of the range-ranked route against the host model, one stage at a time, with guard bands
(tests/cpp/rm_stage_driver.hip): k_prepare (one to eight tiles per workgroup) with k_nu_count_groups, the three scan
launches, k_range_partition in one level and in two (with k_seg_tables, k_seg_hist, k_seg_range_table), k_range_offsets,
and k_rank_mark under quota vectors no sweep produced -- at sizes from one read on, which the public entry (ranked route
from 128 Ki reads) never reaches.  One driver process per case, one after another; rm_stage_compare.compare_stage_dump
names the stage, the buffer and the index of the first difference, over every buffer's whole extent.

What is compared other than by plain equality (rm_stage_compare's docstring has the rules): an exception group's slots on
a tile off k_prepare's lean path and the overflow region are filled in atomic order and are compared as sets -- and
where such a group meets more than 128 exceptions, which 128 of them it lists is that order's as well: the lists and the
overflow region together must be exactly the exceptions.  The span statistics of a call with an invalid read follow the
kernel: a whole one-contig tile takes every read's span, the other tiles only the valid reads'.  The tiles_per_block
cases of one n share their reads, so "equal to the library's own choice" is equality of each with the one model."""
import os
import subprocess

import pytest

import rm_stage_compare as rc
from rm_stage_cases import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "rm_stage_driver")
TIMEOUT_S = 120                   # a cap that ends a hang, not a speed assertion
_device_trouble = []              # once a driver run faulted, hung or met a HIP error: no further process is started


@pytest.fixture(scope="module")
def stage_driver():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", ROOT, "rm_stage_driver"], check=True)
    return EXE


def run_case(exe, case, directory):
    """-> the dump; raises where the driver did not end in a way a dump can be compared after"""
    if _device_trouble:
        pytest.fail("not started: an earlier driver run ended badly (%s)" % _device_trouble[0])
    jpath, bpath = rc.write_case(case, directory)
    dj, db = os.path.join(str(directory), "dump.json"), os.path.join(str(directory), "dump.bin")
    try:
        out = subprocess.run([exe, jpath, bpath, dj, db], capture_output=True, text=True, timeout=TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _device_trouble.append("%s: no end after %d s" % (case["name"], TIMEOUT_S))
        pytest.fail(_device_trouble[0])
    finally:
        os.unlink(bpath)
    if out.returncode < 0 or out.returncode in (134, 137, 139):
        _device_trouble.append("%s: driver ended with status %d: %s" % (case["name"], out.returncode, out.stderr[-500:]))
        pytest.fail(_device_trouble[0])
    assert os.path.exists(dj), "no manifest (status %d): %s" % (out.returncode, out.stderr[-500:])
    dump = rc.load_dump(dj, db)
    os.unlink(db)
    if dump["hip_error"]:
        _device_trouble.append("%s: %s" % (case["name"], dump["hip_error"]))
    dump["returncode"] = out.returncode
    return dump


@pytest.mark.parametrize("name", list(CASES))
def test_stage_buffers_match_the_model(name, stage_driver, tmp_path):
    case = rc.plan_case(CASES[name]())
    dump = run_case(stage_driver, case, tmp_path)
    rc.compare_stage_dump(case, dump)
    assert dump["returncode"] == 0
