"""The range-major kernels one stage at a time: the case and dump files of tests/cpp/rm_stage_driver.hip, and
compare_stage_dump(), which holds every buffer the driver hands back, over its whole extent, against the host model
(tests/range_major_model.py).  The generic parts -- the files' formats, load_dump, the naming of stage, buffer and first
differing index, pack_mask, the six quota vectors -- are those of tests/pm_stage_compare.py.

A dump is {"derived", "violations", "inputs_changed", "hip_error", "refused", "buffers": {(stage, name): array}}; the
stages are "A" (k_prepare), "B" (the scan), "C" (the partition, one or two levels), "D" (bucket offsets), "E0", "E1", ...
(k_rank_mark, one per quota vector; "E0o", ...: once more with the list kept the other way, where the scratch buffer
holds either).  What the later stages only read the driver itself holds against its last dump ("inputs_changed").

Unspecified content, and how it is compared (everything else is equality with the model, never-written words = canary):
  * An exception group's slots on a tile off the lean path (a partial tile, or one that holds two contigs) are given out
    in LDS-atomic order: the group's listed triples are compared as a set.  Where such a group meets more than its 128
    slots hold, WHICH 128 it lists is that order's too: the listed ones must be distinct members of the group, the count
    exactly 128, and the listed triples of all groups together with the overflow region exactly the exceptions.
  * The overflow region's order is one global atomic's: compared as a set.
  * On a lean tile the slot order is read-index order and is compared as such."""
import numpy as np

import pm_stage_compare as sc
import range_major_model as rm
from pm_stage_compare import (CANARY16, CANARY32, StageMismatch, _fail, _get, _same, load_dump, pack_mask)  # noqa: F401

BIG_QUOTA = sc.BIG_QUOTA
DENSE_LIMIT = 1 << 20       # genomes beyond this take their quota vectors in sparse form


# ---------------------------------------------------------------------------------------------------------------- cases
def make_case(name, lengths, counts, starts, ends, ell_reg=0, stop_after="E", expect_bad=0, seed=0, tiles_per_block=0,
              n_quota=6):
    """starts / ends: contig-local coordinates of every read, the reads of contig c at [roff[c], roff[c + 1])"""
    case = sc.make_case(name, lengths, counts, starts, ends, wish=0, ell_reg=ell_reg, stop_after=stop_after,
                        expect_bad=expect_bad, seed=seed)
    return adopt(case, tiles_per_block=tiles_per_block, n_quota=n_quota)


def adopt(case, stop_after=None, tiles_per_block=0, n_quota=6):
    """a case of the pass-major tests (pm_stage_compare.make_case) as one of these"""
    case["wish"] = 0
    case["tiles_per_block"] = int(tiles_per_block)
    case["n_quota"] = int(n_quota)
    if stop_after is not None:
        case["stop_after"] = stop_after
    return case


def sparse(default, pos=(), val=()):
    return {"default": int(default), "pos": np.asarray(pos, np.int64), "val": np.asarray(val, np.int64)}


def dense_of(q, ltot):
    if not isinstance(q, dict):
        return np.asarray(q, np.uint32)
    out = np.full(ltot, q["default"], np.uint32)
    out[q["pos"]] = q["val"]
    return out


def quota_vectors(gs_regular, ltot, seed, n_quota):
    """six: those of the pass-major tests (0, 2^20, 1, exactly enough, one short, random); three (two partition levels):
    0, exactly enough, random in 0 .. size + 1.  Beyond DENSE_LIMIT positions in sparse form: a default, and values at the
    positions that start a read and as many other ones"""
    gs_regular = np.asarray(gs_regular, np.int64)
    if ltot <= DENSE_LIMIT and n_quota == 6:
        return sc.quota_vectors(gs_regular, ltot, seed)
    rng = np.random.default_rng(1000 + seed)
    pos, count = np.unique(gs_regular, return_counts=True)
    other = np.setdiff1d(rng.integers(0, ltot, size=pos.size + 16), pos)
    rand_pos = np.concatenate([pos, other])
    rand_size = np.concatenate([count, np.zeros(other.size, np.int64)])
    if n_quota == 3:
        return [sparse(0), sparse(0, pos, count), sparse(3, rand_pos, rng.integers(0, rand_size + 2))]
    assert n_quota == 6
    return [sparse(0), sparse(BIG_QUOTA), sparse(1), sparse(0, pos, count), sparse(0, pos, np.maximum(count - 1, 0)),
            sparse(0, rand_pos, rng.choice([0, 0, 1, 1, 2, 5, BIG_QUOTA], size=rand_pos.size))]


def plan_case(case):
    """the geometry, the model and the quota vectors of stage E"""
    ltot = int(case["poff"][-1])
    case["ltot"] = ltot
    case["shift"] = rm.range_shift_for(ltot)
    case["two_level"] = rm.range_path_two_level(ltot)
    m = model_of(case)
    case["quotas"] = []
    if case["stop_after"] == "E":
        case["quotas"] = quota_vectors(m["gs"][m["regular"]], ltot, case["seed"], case["n_quota"])
    return case


def _write_quota(f, q):
    if isinstance(q, dict):
        f.write(np.array([1, q["default"], q["pos"].size], "<u4").tobytes())
        f.write(q["pos"].astype("<u4").tobytes())
        f.write(q["val"].astype("<u4").tobytes())
    else:
        f.write(np.array([0], "<u4").tobytes())
        f.write(np.asarray(q).astype("<u4").tobytes())


def write_case(case, directory):
    return sc.write_case(case, directory, more={"tiles_per_block": case["tiles_per_block"]}, write_quota=_write_quota)


# ---------------------------------------------------------------------------------------------------------- the model
def model_of(case):
    """everything the stages are expected to write (cached in the case)"""
    if "_rm_model" in case:
        return case["_rm_model"]
    ltot, shift, two = case["ltot"], case["shift"], case["two_level"]
    prep = rm.prepare(case["starts"], case["ends"], case["roff"], case["lengths"], case["ell_reg"], shift + 8 if two else shift)
    n = prep["n"]
    m = dict(prep)
    m["scanned"], m["spine2"] = rm.scan_table(prep["table"])
    m["total"] = int(m["scanned"][-1])
    if case["stop_after"] >= "C":
        if two:
            m.update(rm.partition_two_levels(prep, m["scanned"], shift, rm.seg_tile_bound(n)))
        else:
            m["keys16"], m["idx"], m["range_start"], m["max_load"] = rm.partition_one_level(prep, m["scanned"], shift)
    if case["stop_after"] >= "D":
        m["boff"], m["empty"] = rm.offsets(m["keys16"], m["range_start"], shift, ltot)
    case["_rm_model"] = m
    return m


def expected_masks(case):
    """the keep mask every quota vector of the case asks for, through the model's own streams (cached)"""
    m = model_of(case)
    if "masks" not in m:
        m["masks"] = []
        boff = m["boff"].astype(np.int64)
        for q in case["quotas"]:
            selend = boff[:case["ltot"]] + dense_of(q, case["ltot"])
            m["masks"].append(rm.rank_mask(m["keys16"], m["idx"], m["range_start"], case["shift"], case["ltot"], boff, selend, m["n"])[0])
    return m["masks"]


def expected_derived(case):
    m = model_of(case)
    n, ltot, shift = m["n"], case["ltot"], case["shift"]
    by_records = rm.rank_scratch_by_records(shift, ltot, n)
    scratch = rm.rank_scratch_bytes(shift, ltot, n)
    other = (rm.rank_by_pos_slots(shift, ltot) if by_records else n) * 8 <= scratch
    return {"shift": shift, "two_level": int(case["two_level"]), "pitch": m["pitch"], "sort_tiles": rm.sort_tiles(n),
            "seg_tile_bound": rm.seg_tile_bound(n), "spine_bytes": rm.spine_bytes(n, ltot), "prepare_exc_slots": rm.prepare_exc_slots(n),
            "scratch_bytes": scratch, "by_records": int(by_records), "other_fits": int(other)}


def rank_stages(case):
    """the names of the case's E stages, in the driver's order"""
    other = expected_derived(case)["other_fits"]
    return [s for k in range(len(case["quotas"])) for s in (["E%d" % k, "E%do" % k] if other else ["E%d" % k])]


def _tail_is_canary(stage, name, got, at, canary, what):
    _same(stage, name, got[at:], np.full(got.size - at, canary, got.dtype), what)


def _rows_sorted(rows):
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    return rows[np.lexsort((rows[:, 1], rows[:, 0], rows[:, 2]))]


def _compare_exceptions(case, m, exc, cap, stats):
    n = m["n"]
    if cap < rm.prepare_exc_slots(n) or exc.size != 7 * cap + 2 * (cap // rm.EXC_PER_GROUP + 4) + 8:
        _fail("A", "exc", "capacity %d / %d words" % (cap, exc.size))
    groups = rm.sort_tiles(n) * 4
    want = np.full(exc.size, CANARY32, np.uint32)
    want[6 * cap:6 * cap + cap // rm.EXC_PER_GROUP + 4] = 0           # (cleared ahead of the launch, as the solve does)
    want[6 * cap:6 * cap + groups] = np.minimum(m["exc_total"], rm.EXC_PER_GROUP)
    _same("A", "exc", exc[6 * cap:6 * cap + groups], want[6 * cap:6 * cap + groups], "group counts: ")
    n_over = int(np.maximum(m["exc_total"] - rm.EXC_PER_GROUP, 0).sum())
    assert n_over <= rm.NU_OVERFLOW
    listed = []
    for g, ent in m["exc_of"].items():
        k = min(ent.shape[0], rm.EXC_PER_GROUP)
        at = g * rm.EXC_PER_GROUP
        got = np.stack([exc[a * cap + at:a * cap + at + k] for a in range(3)], axis=1).astype(np.int64)
        if m["lean"][g // 4]:
            _same("A", "exc", got.reshape(-1), ent[:k].reshape(-1), "group %d (lean tile: read-index order), (start, end, index) x slot: " % g)
        else:
            mine = {tuple(r) for r in ent.tolist()}
            rows = [tuple(r) for r in got.tolist()]
            if len(set(rows)) != k or not set(rows) <= mine:
                _fail("A", "exc", "group %d: its %d listed triples are not distinct exceptions of the group" % (g, k))
        listed.append(got)
        for a in range(3):
            want[a * cap + at:a * cap + at + k] = exc[a * cap + at:a * cap + at + k]
    o0 = cap - rm.NU_OVERFLOW
    got_over = np.stack([exc[a * cap + o0:a * cap + o0 + n_over] for a in range(3)], axis=1).astype(np.int64)
    listed.append(got_over)
    everything = np.concatenate([ent for ent in m["exc_of"].values()]) if m["exc_of"] else np.zeros((0, 3), np.int64)
    if not np.array_equal(_rows_sorted(np.concatenate(listed)), _rows_sorted(everything)):
        _fail("A", "exc", "the groups' lists and the overflow region's %d entries together are not the exceptions" % n_over)
    for a in range(3):
        want[a * cap + o0:a * cap + o0 + n_over] = exc[a * cap + o0:a * cap + o0 + n_over]
    _same("A", "exc", exc, want, "lists, counts and never-written slots: ")
    return int(m["exc_total"].sum()), n_over


# ------------------------------------------------------------------------------------------------------ the comparison
def compare_stage_dump(case, dump):
    """raises StageMismatch on the first difference, naming the stage and the buffer"""
    if dump["refused"]:
        raise StageMismatch("stage setup buffer -: the driver refused the case: %s" % dump["refused"])
    if dump["hip_error"]:
        raise StageMismatch("stage ? buffer -: HIP error: %s" % dump["hip_error"])
    for v in dump["violations"]:
        _fail(v["stage"], v["buffer"], "guard band touched on the %s side, first at byte %d" % (v["side"], v["offset"]))
    m = model_of(case)
    n, pitch, ltot, shift, two = m["n"], m["pitch"], case["ltot"], case["shift"], case["two_level"]
    stop, filt = case["stop_after"], case["ell_reg"] != 0
    der = dump["derived"]
    for key, want in expected_derived(case).items():
        if int(der[key]) != int(want):
            _fail("setup", "derived", "%s is %d, expected %d" % (key, der[key], want))

    # ---- stage A: k_prepare
    tab = _get(dump, "A", "table")
    if tab.size != 256 * pitch + 4:
        _fail("A", "table", "%d words, expected %d" % (tab.size, 256 * pitch + 4))
    _same("A", "table", tab[:256 * pitch], m["table"].reshape(-1), "[digit][pass] counts: ")
    _tail_is_canary("A", "table", tab, 256 * pitch, CANARY32, "behind the table: ")
    want_stats = np.array(list(m["stats012"]) + [0, 0, 0, 0, 0] + [CANARY32] * 4, np.uint32)
    stats = _get(dump, "A", "stats")
    if filt:
        exc = _get(dump, "A", "exc")
        n_exc, n_over = _compare_exceptions(case, m, exc, int(der["exc_cap"]), stats)
        want_stats[4], want_stats[6] = n_exc, n_over
    _same("A", "stats", stats, want_stats)
    if int(stats[2]) != case["expect_bad"]:
        _fail("A", "stats", "the error flag is %d, the case expects %d" % (int(stats[2]), case["expect_bad"]))
    _same("A", "mask", _get(dump, "A", "mask"), np.zeros((n + 63) // 64, np.uint64), "cleared words: ")
    if stop == "A":
        return _finish(case, dump, 1)

    # ---- stage B: the scan
    tab = _get(dump, "B", "table")
    _same("B", "table", tab[:256 * pitch + 1], m["scanned"], "exclusive scan, the total at [256 pitch]: ")
    _tail_is_canary("B", "table", tab, 256 * pitch + 1, CANARY32, "behind the total: ")
    if filt and int(tab[256 * pitch]) != n - int(stats[4]):
        _fail("B", "table", "the total %d is not n - listed exceptions = %d" % (int(tab[256 * pitch]), n - int(stats[4])))
    spine = _get(dump, "B", "spine2")
    if spine.size * 4 != rm.spine_bytes(n, ltot):
        _fail("B", "spine2", "%d bytes, expected %d" % (spine.size * 4, rm.spine_bytes(n, ltot)))
    _same("B", "spine2", spine[:m["spine2"].size], m["spine2"], "tile sums scanned, the total behind them: ")
    _tail_is_canary("B", "spine2", spine, m["spine2"].size, CANARY32, "behind the spine: ")
    if stop == "B":
        return _finish(case, dump, 2)

    # ---- stage C: the partition
    total = m["total"]
    keys16 = _get(dump, "C", "keys16")
    idx = _get(dump, "C", "idx")
    if keys16.size != 4 * n or idx.size != n:
        _fail("C", "keys16", "%d / %d slots, expected %d / %d" % (keys16.size, idx.size, 4 * n, n))
    _same("C", "keys16", keys16[:total], m["keys16"], "position inside the range, ranges in read-index order: ")
    _tail_is_canary("C", "keys16", keys16, total, CANARY16, "from the listed total on: ")
    _same("C", "idx", idx[:total], m["idx"], "read index, ranges in read-index order: ")
    _tail_is_canary("C", "idx", idx, total, CANARY32, "from the listed total on: ")
    want = np.full(rm.RANGES_WORDS, CANARY32, np.uint32)
    want[:m["range_start"].size] = m["range_start"]
    want[rm.MAX_LOAD_AT] = m["max_load"]
    if two:
        for k, name in enumerate(("super_start", "tile_base", "pass_base")):
            want[rm.SEG_TABLES_AT + 257 * k:rm.SEG_TABLES_AT + 257 * (k + 1)] = m[name]
    ranges = _get(dump, "C", "ranges")
    _same("C", "ranges", ranges[:m["range_start"].size], m["range_start"], "range_start: ")
    _same("C", "ranges", ranges[rm.MAX_LOAD_AT:rm.MAX_LOAD_AT + 1], want[rm.MAX_LOAD_AT:rm.MAX_LOAD_AT + 1], "max_load[0] (word 65540): ")
    _same("C", "ranges", ranges, want, "range_start | max_load | super_start, tile_base, pass_base | canary: ")
    if int(ranges[m["range_start"].size - 1]) != total:
        _fail("C", "ranges", "the last range start is %d, the listed total %d" % (int(ranges[m["range_start"].size - 1]), total))
    if two:
        recs = _get(dump, "C", "recs")
        if recs.size != 2 * n:
            _fail("C", "recs", "%d words, expected %d" % (recs.size, 2 * n))
        _same("C", "recs", recs[:2 * total], m["recs"].reshape(-1), "level-1 records {global start, index} x record, stable by super-range: ")
        _tail_is_canary("C", "recs", recs, 2 * total, CANARY32, "from the listed total on: ")
        _same("C", "hist", _get(dump, "C", "hist"), m["hist_scanned"], "level-2 histogram [super-range][digit][tile], scanned: ")
    if stop == "C":
        return _finish(case, dump, 3)

    # ---- stage D: bucket offsets
    _same("D", "boff", _get(dump, "D", "boff"), m["boff"])
    want_stats[3] = m["empty"]
    _same("D", "stats", _get(dump, "D", "stats"), want_stats, "word 3 = positions that start no read: ")
    if stop == "D":
        return _finish(case, dump, 4)

    # ---- stage E: the ranking, per quota vector (and per way of keeping the list)
    if not case["quotas"]:
        _fail("E0", "mask", "the case has no quota vector")
    masks = expected_masks(case)
    for stage in rank_stages(case):
        want_bits = masks[int(stage[1:].rstrip("o"))]
        got = _get(dump, stage, "mask")
        if got.size != (n + 63) // 64:
            _fail(stage, "mask", "%d words, expected %d" % (got.size, (n + 63) // 64))
        bits = np.unpackbits(got.astype("<u8").view(np.uint8), bitorder="little").astype(bool)
        if bits[n:].any():
            _fail(stage, "mask", "bit %d is set, at or above n = %d" % (n + int(np.nonzero(bits[n:])[0][0]), n))
        _same(stage, "mask", bits[:n], want_bits, "read ")
        want_sc = np.zeros(16, np.uint32)
        want_sc[0] = int(bits.sum())
        _same(stage, "scalars", _get(dump, stage, "scalars"), want_sc, "kept total = popcount of the mask: ")
    return _finish(case, dump, 4 + len(rank_stages(case)))


def _finish(case, dump, n_stages):
    if dump["inputs_changed"]:
        _fail("end", dump["inputs_changed"][0], "a buffer the later stages only read was changed")
    have = {stage for stage, _ in dump["buffers"]}
    if len(have) != n_stages:
        _fail("end", "-", "the dump holds %d stages, expected %d" % (len(have), n_stages))


# -------------------------------------------------------------------------------------- a dump built from the model
def model_dump(case):
    """the dump a correct device would hand back (for tests without a device)"""
    m = model_of(case)
    n, pitch, ltot, two = m["n"], m["pitch"], case["ltot"], case["two_level"]
    stop, filt = case["stop_after"], case["ell_reg"] != 0
    der = expected_derived(case)
    der["exc_cap"] = 0
    buf = {}
    stats = np.array(list(m["stats012"]) + [0, 0, 0, 0, 0] + [CANARY32] * 4, np.uint32)
    if filt:
        cap = der["exc_cap"] = rm.prepare_exc_slots(n)
        exc = np.full(7 * cap + 2 * (cap // rm.EXC_PER_GROUP + 4) + 8, CANARY32, np.uint32)
        exc[6 * cap:6 * cap + cap // rm.EXC_PER_GROUP + 4] = 0
        exc[6 * cap:6 * cap + m["exc_total"].size] = np.minimum(m["exc_total"], rm.EXC_PER_GROUP)
        over = []
        for g, ent in m["exc_of"].items():
            k = min(ent.shape[0], rm.EXC_PER_GROUP)
            for a in range(3):
                exc[a * cap + g * rm.EXC_PER_GROUP:a * cap + g * rm.EXC_PER_GROUP + k] = ent[:k, a]
            over.append(ent[k:])
        over = np.concatenate(over) if over else np.zeros((0, 3), np.int64)
        for a in range(3):
            exc[a * cap + cap - rm.NU_OVERFLOW:a * cap + cap - rm.NU_OVERFLOW + over.shape[0]] = over[:, a]
        stats[4], stats[6] = int(m["exc_total"].sum()), over.shape[0]
        buf[("A", "exc")] = exc
    buf.update({("A", "table"): np.concatenate([m["table"].reshape(-1), np.full(4, CANARY32, np.uint32)]).astype(np.uint32),
                ("A", "stats"): stats.copy(), ("A", "mask"): np.zeros((n + 63) // 64, np.uint64)})
    if stop >= "B":
        spine = np.full(rm.spine_bytes(n, ltot) // 4, CANARY32, np.uint32)
        spine[:m["spine2"].size] = m["spine2"]
        buf.update({("B", "table"): np.concatenate([m["scanned"], np.full(3, CANARY32, np.uint32)]).astype(np.uint32), ("B", "spine2"): spine})
    if stop >= "C":
        total = m["total"]
        keys16 = np.full(4 * n, CANARY16, np.uint16)
        keys16[:total] = m["keys16"]
        idx = np.full(n, CANARY32, np.uint32)
        idx[:total] = m["idx"]
        ranges = np.full(rm.RANGES_WORDS, CANARY32, np.uint32)
        ranges[:m["range_start"].size] = m["range_start"]
        ranges[rm.MAX_LOAD_AT] = m["max_load"]
        buf.update({("C", "keys16"): keys16, ("C", "idx"): idx, ("C", "ranges"): ranges})
        if two:
            for k, name in enumerate(("super_start", "tile_base", "pass_base")):
                ranges[rm.SEG_TABLES_AT + 257 * k:rm.SEG_TABLES_AT + 257 * (k + 1)] = m[name]
            recs = np.full(2 * n, CANARY32, np.uint32)
            recs[:2 * total] = m["recs"].reshape(-1)
            buf.update({("C", "recs"): recs, ("C", "hist"): m["hist_scanned"].copy()})
    if stop >= "D":
        stats_d = stats.copy()
        stats_d[3] = m["empty"]
        buf.update({("D", "boff"): m["boff"].copy(), ("D", "stats"): stats_d})
    if stop >= "E":
        masks = expected_masks(case)
        for stage in rank_stages(case):
            bits = masks[int(stage[1:].rstrip("o"))]
            scal = np.zeros(16, np.uint32)
            scal[0] = int(bits.sum())
            buf[(stage, "mask")] = pack_mask(bits)
            buf[(stage, "scalars")] = scal
    return {"derived": der, "violations": [], "inputs_changed": [], "hip_error": None, "refused": None, "buffers": buf}
