"""compare_stage_dump (tests/pm_stage_compare.py) on the CPU: it accepts the dump the host model itself describes, for
three of the stage tests' cases -- a size edge, the ragged genome on the aligned grid, the filter with overflowing
waves --, and rejects every one of the single-word mutations a subtly wrong kernel would amount to.  This is how "the GPU
test would fail" is checked on a machine without a GPU."""
import numpy as np
import pytest

import pm_grid_model as gm
import pm_stage_compare as sc
from pm_stage_cases import CASES

NAMES = ["size_8193", "genome_ragged_aligned", "filter_run"]


@pytest.fixture(scope="module")
def grid_driver(tmp_path_factory):
    return gm.build_driver(tmp_path_factory.mktemp("pm_grid_plan"))


@pytest.fixture(scope="module")
def planned(grid_driver):
    out = {}
    for name in NAMES:
        case = sc.plan_case(CASES[name](), grid_driver)
        out[name] = (case, sc.model_dump(case))
    return out


def _with(dump, key, edit):
    """a copy of the dump with one buffer edited"""
    buffers = dict(dump["buffers"])
    buffers[key] = buffers[key].copy()
    edit(buffers[key])
    return dict(dump, buffers=buffers)


def _first_slice_of_two(m):
    for d, P in zip(*np.nonzero((m["lstw"] >> 16) >= 2)):
        return int(P) * m["stride"] + int(m["lstw"][d, P] & 0xFFFF) * 64
    raise AssertionError("no slice of two records")


def swap_neighbours(case, dump):
    at = _first_slice_of_two(sc.model_of(case))
    def edit(a):
        a[at], a[at + 1] = a[at + 1], a[at]
    return _with(dump, ("A", "idx16"), edit)


def desc_count(case, dump):
    def edit(a):
        a[0] ^= 1
    return _with(dump, ("B", "desc"), edit)


def padding_pass_entry(case, dump):
    m = sc.model_of(case)
    assert m["n_pass"] < m["pitch"]
    def edit(a):
        a[3 * m["pitch"] + m["n_pass"]] = 64
    return _with(dump, ("A", "cnt_tab"), edit)


def padding_pass_list_entry(case, dump):
    m = sc.model_of(case)
    def edit(a):
        a[3 * m["pitch"] + m["pitch"] - 1] = 1
    return _with(dump, ("A", "lst_tab"), edit)


def tp_total(case, dump):
    m = sc.model_of(case)
    def edit(a):
        a[256 * m["pitch"]] += 64
    return _with(dump, ("B", "cnt_tab"), edit)


def range_start_k(case, dump):
    def edit(a):
        a[sc.model_of(case)["n_ranges"] // 2] += 1
    return _with(dump, ("B", "range_start"), edit)


def max_load_slots(case, dump):
    def edit(a):
        a[1] += 1
    return _with(dump, ("B", "max_load"), edit)


def max_load_records(case, dump):
    def edit(a):
        a[0] -= 1
    return _with(dump, ("B", "max_load"), edit)


def boff_range_first(case, dump):
    g = case["grid"]
    r = max(k for k in range(g["n_ranges"]) if g["live"][k] > 0)
    def edit(a):
        a[int(g["pos0"][r])] += 1
    return _with(dump, ("C", "boff"), edit)


def boff_total(case, dump):
    def edit(a):
        a[case["ltot"]] -= 1
    return _with(dump, ("C", "boff"), edit)


def empty_positions(case, dump):
    def edit(a):
        a[3] += 1
    return _with(dump, ("C", "stats"), edit)


def mask_bit(case, dump):
    def edit(a):
        a[a.size // 2] ^= np.uint64(1 << 17)
    return _with(dump, ("D5", "mask"), edit)


def mask_bit_at_n(case, dump):
    n = sc.model_of(case)["n"]
    assert n % 64 != 0
    def edit(a):
        a[-1] |= np.uint64(1 << (n % 64))
    return _with(dump, ("D0", "mask"), edit)


def kept_total(case, dump):
    def edit(a):
        a[0] += 1
    return _with(dump, ("D3", "scalars"), edit)


def canary_outside_groups(case, dump):
    slot = int(np.nonzero(~sc.model_of(case)["grp"])[0][-1])
    def edit(a):
        a[slot] = 0
    return _with(dump, ("A", "keys16"), edit)


def descriptor_beyond_the_last(case, dump):
    G = int(sc.model_of(case)["Tp"][-1]) // 64
    def edit(a):
        a[G] = 0
    return _with(dump, ("B", "desc"), edit)


def guard_violation(case, dump):
    return dict(dump, violations=[{"stage": "A", "buffer": "keys16", "side": "high", "offset": 0}])


def input_changed(case, dump):
    return dict(dump, inputs_changed=["starts"])


MUTATIONS = [swap_neighbours, desc_count, padding_pass_list_entry, tp_total, range_start_k, max_load_slots, max_load_records,
             boff_range_first, boff_total, empty_positions, mask_bit, mask_bit_at_n, kept_total, canary_outside_groups,
             descriptor_beyond_the_last, guard_violation, input_changed]
# (the ragged case's reads fill its passes' pitch: no padding pass there)
PAIRS = [(name, mut) for name in NAMES for mut in MUTATIONS] + [("size_8193", padding_pass_entry), ("filter_run", padding_pass_entry)]


@pytest.mark.parametrize("name", NAMES)
def test_the_models_own_dump_is_accepted(planned, name):
    case, dump = planned[name]
    sc.compare_stage_dump(case, dump)


@pytest.mark.parametrize("name,mutation", PAIRS, ids=["%s-%s" % (n, f.__name__) for n, f in PAIRS])
def test_a_single_word_mutation_is_rejected(planned, name, mutation):
    case, dump = planned[name]
    with pytest.raises(sc.StageMismatch):
        sc.compare_stage_dump(case, mutation(case, dump))


def test_exception_list_mutations_are_rejected(planned):
    case, dump = planned["filter_run"]
    cap = dump["derived"]["exc_cap"]
    m = sc.model_of(case)
    g = next(g for g, ent in m["exc_groups"].items() if ent.shape[0] == 128)
    def swap_listed(a):        # the per-wave lists match in order
        a[2 * cap + g * 128], a[2 * cap + g * 128 + 1] = a[2 * cap + g * 128 + 1], a[2 * cap + g * 128]
    def overflow_entry(a):     # the overflow region matches as a set
        a[cap - sc.NU_OVERFLOW] += 1
    def count(a):
        a[6 * cap + g] -= 1
    def written_behind_a_list(a):
        a[g * 128 + 128 * 3] = 0 if (g + 3) not in m["exc_groups"] else a[g * 128 + 128 * 3] + 1
    for edit in (swap_listed, overflow_entry, count, written_behind_a_list):
        with pytest.raises(sc.StageMismatch):
            sc.compare_stage_dump(case, _with(dump, ("A", "exc"), edit))
    def listed_total(a):
        a[4] += 1
    with pytest.raises(sc.StageMismatch):
        sc.compare_stage_dump(case, _with(dump, ("A", "stats"), listed_total))
