"""Every pass-major kernel against the host model, one stage at a time, with guard bands (tests/cpp/pm_stage_driver.hip):
k_pm_prepare_sort, k_pm_row_sums + k_pm_tables, k_pm_offsets, and k_pm_walk with its settling tail under quota vectors
no sweep produced -- at sizes from one read on, which the public entry (ranked route from 128 Ki reads) never reaches.
One driver process per case; pm_stage_compare.compare_stage_dump names the stage, the buffer and the index of the first
difference.  (Note on the issue's wording: lst_tab's rows at and beyond the grid's ranges are not all zero -- the
kernel and the model both store the pass's padded end there as the slot group, with a record count of zero; the
comparison requires equality with the model over the whole extent, zero counts there, and zeros in the padding passes.)"""
import os
import subprocess

import pytest

import pm_grid_model as gm
import pm_stage_compare as sc
from pm_stage_cases import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "pm_stage_driver")
TIMEOUT_S = 120                   # a cap that ends a hang, not a speed assertion
_device_trouble = []              # once a driver run faulted, hung or met a HIP error: no further process is started


@pytest.fixture(scope="module")
def stage_driver():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", ROOT, "pm_stage_driver"], check=True)
    return EXE


@pytest.fixture(scope="module")
def grid_driver(tmp_path_factory):
    return gm.build_driver(tmp_path_factory.mktemp("pm_grid_plan"))


def run_case(exe, case, directory):
    """-> the dump; raises where the driver did not end in a way a dump can be compared after"""
    if _device_trouble:
        pytest.fail("not started: an earlier driver run ended badly (%s)" % _device_trouble[0])
    jpath, bpath = sc.write_case(case, directory)
    dj, db = os.path.join(str(directory), "dump.json"), os.path.join(str(directory), "dump.bin")
    try:
        out = subprocess.run([exe, jpath, bpath, dj, db], capture_output=True, text=True, timeout=TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _device_trouble.append("%s: no end after %d s" % (case["name"], TIMEOUT_S))
        pytest.fail(_device_trouble[0])
    finally:
        os.unlink(bpath)          # (the quota vectors of a long genome: tens of megabytes)
    if out.returncode < 0 or out.returncode in (134, 137, 139):
        _device_trouble.append("%s: driver ended with status %d: %s" % (case["name"], out.returncode, out.stderr[-500:]))
        pytest.fail(_device_trouble[0])
    assert os.path.exists(dj), "no manifest (status %d): %s" % (out.returncode, out.stderr[-500:])
    dump = sc.load_dump(dj, db)
    os.unlink(db)
    if dump["hip_error"]:
        _device_trouble.append("%s: %s" % (case["name"], dump["hip_error"]))
    dump["returncode"] = out.returncode
    return dump


@pytest.mark.parametrize("name", list(CASES))
def test_stage_buffers_match_the_model(name, stage_driver, grid_driver, tmp_path):
    case = sc.plan_case(CASES[name](), grid_driver)
    dump = run_case(stage_driver, case, tmp_path)
    sc.compare_stage_dump(case, dump)
    assert dump["returncode"] == 0
    want_stages = {"A": 1, "B": 2, "C": 3, "D": 3 + len(case["quotas"])}[case["stop_after"]]
    assert len({stage for stage, _ in dump["buffers"]} - {"in", "end"}) == want_stages
