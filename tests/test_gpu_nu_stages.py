"""Every kernel of the near-uniform route against the device-shaped host model, round by round, with guard bands
(tests/cpp/nu_stage_driver.hip): launch_nu_setup, the sweep of the case's form under nadj (event-driven with its restart
block and checkpoints; block-scan over whole contigs; block-scan under a cut-point table with the round before's marks),
launch_nu_round (k_nu_diff, k_nu_verify, k_nu_bin, both k_nu_replay launches, k_nu_select_apply) and
launch_nu_mark_selected -- on a few hundred to a few thousand reads, which the public entry's gates never let through to
the route.  One driver process per case, one after another; nu_stage_compare.compare_stage_dump names the stage, the
buffer and the index of the first difference (its docstring has the rules for what is filled in atomic order).

Beside it every case that is no give-up case goes through the public entry on a fresh Solver with rank_min_reads=1: the
mask must be the oracle's whatever route the call takes."""
import os
import subprocess

import numpy as np
import pytest

import nu_stage_compare as nsc
from nu_stage_cases import CASES, GIVE_UP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "nu_stage_driver")
TIMEOUT_S = 120                   # a cap that ends a hang, not a speed assertion
_device_trouble = []              # once a driver run faulted, hung or met a HIP error: no further process is started


@pytest.fixture(scope="module")
def stage_driver():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", ROOT, "nu_stage_driver"], check=True)
    return EXE


def run_case(exe, case, directory):
    """-> the dump; raises where the driver did not end in a way a dump can be compared after"""
    if _device_trouble:
        pytest.fail("not started: an earlier driver run ended badly (%s)" % _device_trouble[0])
    jpath, bpath = nsc.write_case(case, directory)
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
    dump = nsc.load_dump(dj, db)
    os.unlink(db)
    if dump["hip_error"]:
        _device_trouble.append("%s: %s" % (case["name"], dump["hip_error"]))
    dump["returncode"] = out.returncode
    return dump


@pytest.mark.parametrize("name", list(CASES))
def test_stage_buffers_match_the_model(name, stage_driver, tmp_path):
    case = CASES[name]()
    dump = run_case(stage_driver, case, tmp_path)
    ended = nsc.compare_stage_dump(case, dump)
    print("\n%s: device rounds %s flags %s settled %s | model rounds %d flags %d settled %d" % (
        name, ended["rounds"], ended["flags"], ended["settled"], ended["model_rounds"], ended["model_flags"], ended["model_settled"]))
    assert dump["returncode"] == (2 if GIVE_UP.get(name) == "refused" else 0)


@pytest.mark.parametrize("name", [n for n in CASES if n not in GIVE_UP])
def test_public_entry_gives_the_oracles_mask(name, pkg, oracle):
    if _device_trouble:
        pytest.fail("not started: an earlier driver run ended badly (%s)" % _device_trouble[0])
    case = CASES[name]()
    s, e, lengths, offs = case["starts"].astype(np.uint32), case["ends"].astype(np.uint32), case["lengths"], case["roff"]
    with pkg.Solver(0) as solver:
        solver.set_options(rank_min_reads=1)
        got = solver.solve(s, e, lengths, case["M"], contig_read_offsets=offs)
        path = solver.last_stats.path
    want = oracle.solve(s, e, lengths, case["M"], offs)
    assert np.array_equal(got, want), "path %s: %d mask words differ" % (path, int((np.asarray(got) != want).sum()))
