"""The host model of the range-major form (tests/range_major_model.py) against direct numpy -- a stable argsort by range,
bincount, searchsorted, "the S(p) lowest read indices" --, every case of tests/rm_stage_cases.py below 2 M positions
through the model with all its indices in bounds, and rm_stage_compare.compare_stage_dump on dumps built from the model,
unmodified and with single words changed.  No device."""
import numpy as np
import pytest

import range_major_model as rm
import rm_stage_compare as rc
from rm_stage_cases import CASES

SMALL = [name for name, build in CASES.items() if int(np.sum(build()["lengths"])) < 2_000_000]


def _ragged(seed, lengths, counts, ell_reg=0):
    rng = np.random.default_rng(seed)
    lengths, counts = np.asarray(lengths, np.int64), np.asarray(counts, np.int64)
    contig = np.repeat(np.arange(lengths.size), counts)
    starts = np.concatenate([rng.integers(0, max(int(L) - 40, 1), size=int(k)) for L, k in zip(lengths, counts)])
    span = np.where(rng.random(starts.size) < (0.05 if ell_reg else 0.0), 17, 30)
    ends = np.minimum(starts + span - 1, np.maximum(lengths - 1, 0)[contig])
    return rc.make_case("ragged_%d" % seed, lengths, counts, starts, ends, ell_reg=ell_reg, seed=seed,
                        n_quota=3 if rm.range_path_two_level(int(lengths.sum())) else 6)


def _lowest(gs, regular, S):
    """bit i iff read i is among the S[p] lowest regular read indices of its start position p -- no sort by range"""
    mask = np.zeros(gs.size, bool)
    seen = {}
    for i in np.nonzero(regular)[0]:
        p = int(gs[i])
        seen[p] = seen.get(p, 0) + 1
        mask[i] = seen[p] <= int(S[p])
    return mask


RAGGED = [(1, [70_001, 33_333, 250_000, 1_000], [9_000, 11_011, 30_000, 5], 0),
          (2, [500, 0, 123_456, 77], [3_000, 0, 20_000, 130], 0),
          (3, [1_000_003], [40_001], 30),
          (4, [9_000_001, 5_000_000, 8_388_613, 123], [9_000, 4_800, 8_500, 0], 0),
          (5, [(1 << 23) + 5, 3_000_000], [17_000, 8_000], 30)]


@pytest.mark.parametrize("seed,lengths,counts,ell_reg", RAGGED)
def test_model_against_direct_numpy(seed, lengths, counts, ell_reg):
    case = rc.plan_case(_ragged(seed, lengths, counts, ell_reg))
    m = rc.model_of(case)
    ltot, shift, n = case["ltot"], case["shift"], m["n"]
    gs, regular = m["gs"], m["regular"]
    reg = np.nonzero(regular)[0]
    # the table: reads per (digit, pass)
    part_shift = shift + 8 if case["two_level"] else shift
    flat = np.bincount(((gs[reg] >> part_shift) & 255) * m["pitch"] + reg // rm.PASS, minlength=256 * m["pitch"])
    assert np.array_equal(m["table"].reshape(-1), flat)
    assert np.array_equal(m["scanned"], np.concatenate([[0], np.cumsum(flat)]))
    # the streams: a stable sort of the regular reads by range
    order = reg[np.argsort(gs[reg] >> shift, kind="stable")]
    assert np.array_equal(m["idx"], order)
    assert np.array_equal(m["keys16"], gs[order] & ((1 << shift) - 1))
    n_r = 65536 if case["two_level"] else 256
    assert np.array_equal(m["range_start"], np.concatenate([[0], np.cumsum(np.bincount(gs[reg] >> shift, minlength=n_r))]))
    assert m["max_load"] == np.bincount(gs[reg] >> shift).max()
    if case["two_level"]:
        by_super = reg[np.argsort(gs[reg] >> (shift + 8), kind="stable")]
        assert np.array_equal(m["recs"][:, 1], by_super) and np.array_equal(m["recs"][:, 0], gs[by_super])
        assert np.array_equal(m["super_start"], np.concatenate([[0], np.cumsum(np.bincount(gs[reg] >> (shift + 8), minlength=256))]))
        assert int(m["hist"].sum()) == reg.size and not m["hist"][256 * int(m["tile_base"][256]):].any()
    # bucket offsets and empty positions
    assert np.array_equal(m["boff"], np.searchsorted(np.sort(gs[reg]), np.arange(ltot + 1), side="left"))
    assert m["empty"] == ltot - np.unique(gs[reg]).size
    # the ranking
    for q, bits in zip(case["quotas"], rc.expected_masks(case)):
        assert np.array_equal(bits, _lowest(gs, regular, rc.dense_of(q, ltot)))
    assert not rc.expected_masks(case)[0].any()


@pytest.mark.parametrize("name", SMALL)
def test_cases_run_through_the_model_in_bounds(name):
    """(the model asserts every index it forms; a dump built from it passes the comparison)"""
    case = rc.plan_case(CASES[name]())
    m = rc.model_of(case)
    assert m["stats012"][2] == case["expect_bad"]
    if case["stop_after"] == "E":
        masks = rc.expected_masks(case)
        assert len(masks) == case["n_quota"]
        exact = rc.dense_of(case["quotas"][3 if case["n_quota"] == 6 else 1], case["ltot"])
        assert np.array_equal(masks[3 if case["n_quota"] == 6 else 1], m["regular"])     # exactly enough keeps every regular read
        assert np.array_equal(masks[-1], _lowest(m["gs"], m["regular"], rc.dense_of(case["quotas"][-1], case["ltot"])))
        assert int(exact.sum()) == int(m["regular"].sum())
    rc.compare_stage_dump(case, rc.model_dump(case))


def test_case_list_meets_its_own_conditions():
    """what the issue's list asks of the shapes, shown on the model"""
    seen_bits = set()
    for k in (1, 2, 3, 5, 9, 17, 33, 65, 129):
        case = rc.plan_case(CASES["digit_span_%d" % k]())
        poff, shift = case["poff"], case["shift"]
        d_lo, d_hi = int(poff[1]) >> shift, int(poff[2]) >> shift       # pass 1 is contig 1's reads alone
        assert list(case["roff"][:3]) == [0, rm.PASS, 2 * rm.PASS] and d_hi - d_lo == k - 1
        seen_bits.add(0 if d_hi == d_lo else int(d_hi - d_lo).bit_length())
    assert seen_bits == set(range(9))
    for below in range(4):
        m = rc.model_of(rc.plan_case(CASES["heavy_first_record_%d" % below]()))
        assert int(m["range_start"][5]) & 3 == below and int(m["range_start"][6] - m["range_start"][5]) == 3 * rm.PASS + 67
    for records in (32_767, 32_768, 32_769, 4 * 32_768 + 2):
        m = rc.model_of(rc.plan_case(CASES["heavy_%d" % records]()))
        assert int(m["range_start"][6] - m["range_start"][5]) == records
    for kind, tile, lean in (("lean", 2, True), ("partial", 3, False), ("twocontig", 1, False)):
        for count in (128, 129):
            m = rc.model_of(rc.plan_case(CASES["filter_%s_%d_one_level" % (kind, count)]()))
            assert bool(m["lean"][tile]) == lean and int(m["exc_total"][4 * tile + 1]) == count and int(m["exc_total"].sum()) == count
    m = rc.model_of(rc.plan_case(CASES["contigs_five_in_a_pass"]()))
    assert np.unique(m["contig"][:rm.PASS]).size == 5
    for n in (8 * rm.TILE + 5, 16 * rm.TILE):        # one input per n under every tiles_per_block: one model for all
        builds = [CASES["tiles_per_block_%d_n%d" % (tpb, n)]() for tpb in (0, 2, 4, 6, 8)]
        assert [b["tiles_per_block"] for b in builds] == [0, 2, 4, 6, 8]
        assert all(np.array_equal(b["starts"], builds[0]["starts"]) and np.array_equal(b["ends"], builds[0]["ends"]) for b in builds)
    case = rc.plan_case(CASES["genome_4095_both_lists"]())
    assert rc.expected_derived(case)["other_fits"] == 1 and len(rc.rank_stages(case)) == 12
    # k_range_offsets' positions per thread: below one (range width 512), one (1 024), two (2 048)
    assert [rc.plan_case(CASES["genome_" + tag]())["shift"] for tag in ("511x256", "1023x256", "1024x256")] == [9, 10, 11]


def _mutated(case, key, index, value):
    dump = rc.model_dump(case)
    dump["buffers"][key] = dump["buffers"][key].copy()
    dump["buffers"][key][index] = value
    return dump


@pytest.mark.parametrize("key,index,value,names", [
    (("A", "table"), 5, 7, "stage A buffer table"),
    (("B", "table"), -3, 0, "stage B buffer table"),           # a word behind the total
    (("C", "keys16"), -1, 0, "stage C buffer keys16"),         # the stream's last slot: canary
    (("C", "ranges"), 256, 1, "stage C buffer ranges"),
    (("C", "ranges"), rm.MAX_LOAD_AT, 0, "stage C buffer ranges"),
    (("D", "boff"), 1000, 0xFFFFFFFF, "stage D buffer boff"),
    (("D", "stats"), 3, 0, "stage D buffer stats"),
    (("E4", "mask"), 0, 0, "stage E4 buffer mask"),
    (("A", "exc"), 128 + 3, 0, "stage A buffer exc"),          # a slot never filled
])
def test_comparison_names_stage_and_buffer_of_a_changed_word(key, index, value, names):
    case = rc.plan_case(CASES["filter_three_one_level"]())
    rc.compare_stage_dump(case, rc.model_dump(case))
    with pytest.raises(rc.StageMismatch, match=names):
        rc.compare_stage_dump(case, _mutated(case, key, index, value))
