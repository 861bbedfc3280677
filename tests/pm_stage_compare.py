"""The pass-major kernels one stage at a time: cases, the case and dump files of tests/cpp/pm_stage_driver.hip, and
compare_stage_dump(), which holds every buffer the driver hands back against the host model (tests/pass_major_model.py)
and against plain numpy references.  Shared by tests/test_gpu_pm_stages.py (dumps from the device) and
tests/test_pm_stage_compare_cpu.py (dumps built from the model, unmodified and with single-word mutations).

A dump is {"derived", "violations", "inputs_changed", "hip_error", "refused", "buffers": {(stage, name): array}}; the
stages are "in" (the grid words as uploaded), "A" (producer), "B" (row sums + tables), "C" (bucket offsets), "D0", "D1",
... (the walk, one per quota vector) and "end" (what the walk only reads, once more)."""
import json
import os

import numpy as np

import pass_major_model as pm
import pm_grid_model as gm

CANARY16 = 0xA5A5
CANARY32 = 0xA5A5A5A5
NU_OVERFLOW = 1 << 20          # slots of the exception list's overflow region (its last ones)
TABLE_PARTS = 8                # parts a [range][pass] row is cut into by the table stage
DTYPES = {"u16": np.uint16, "u32": np.uint32, "u64": np.uint64}
BIG_QUOTA = 1 << 20


class StageMismatch(AssertionError):
    pass


# ---------------------------------------------------------------------------------------------------------------- cases
def make_case(name, lengths, counts, starts, ends, wish=-1, ell_reg=0, stop_after="D", expect_aligned=None, expect_bad=0,
              seed=0):
    """starts / ends: contig-local coordinates of every read, the reads of contig c at [roff[c], roff[c + 1])"""
    lengths = np.asarray(lengths, np.int64)
    counts = np.asarray(counts, np.int64)
    starts = np.asarray(starts, np.int64)
    assert starts.size == int(counts.sum()) and starts.size == np.asarray(ends).size and starts.size >= 1
    return {"name": name, "lengths": lengths, "roff": np.concatenate([[0], np.cumsum(counts)]),
            "poff": np.concatenate([[0], np.cumsum(lengths)]), "starts": starts.astype(np.uint32),
            "ends": np.asarray(ends, np.int64).astype(np.uint32), "wish": int(wish), "ell_reg": int(ell_reg),
            "stop_after": stop_after, "expect_aligned": expect_aligned, "expect_bad": int(expect_bad), "seed": int(seed)}


def plan_case(case, grid_driver):
    """the grid the host would cut (csrc/pm_grid_plan.h through its g++ driver) and the quota vectors of stage D"""
    ltot = int(case["poff"][-1])
    case["ltot"] = ltot
    case["shift"] = pm.range_shift_for(ltot)
    case["grid"] = gm.plan(grid_driver, case["lengths"], np.diff(case["roff"]), case["shift"], case["wish"])
    m = model_of(case)
    case["quotas"] = quota_vectors(m["gs"][m["regular"]], ltot, case["seed"]) if case["stop_after"] == "D" else []
    return case


def quota_vectors(gs_regular, ltot, seed):
    """all 0; all 2^20; all 1; exactly enough; one short of enough; random from [0, 0, 1, 1, 2, 5, 2^20]"""
    count = np.bincount(np.asarray(gs_regular, np.int64), minlength=ltot)[:ltot]
    rng = np.random.default_rng(1000 + seed)
    vectors = [np.zeros(ltot), np.full(ltot, BIG_QUOTA), np.ones(ltot), count, np.maximum(count - 1, 0),
               rng.choice([0, 0, 1, 1, 2, 5, BIG_QUOTA], size=ltot)]
    return [np.asarray(v, np.int64).astype(np.uint32) for v in vectors]


def write_case(case, directory, more=None, write_quota=None):
    """-> paths of case.json, case.bin.  more: further flat fields of case.json; write_quota(file, vector): how a driver
    takes a quota vector (default: one u32 per global position)"""
    jpath, bpath = os.path.join(str(directory), "case.json"), os.path.join(str(directory), "case.bin")
    with open(bpath, "wb") as f:
        f.write(case["starts"].astype("<u4").tobytes())
        f.write(case["ends"].astype("<u4").tobytes())
        f.write(case["lengths"].astype("<u8").tobytes())
        f.write(case["roff"].astype("<u8").tobytes())
        for q in case["quotas"]:
            if write_quota is None:
                f.write(q.astype("<u4").tobytes())
            else:
                write_quota(f, q)
    with open(jpath, "w") as f:
        fields = {"n": int(case["starts"].size), "n_contigs": int(case["lengths"].size), "ltot": int(case["ltot"]),
                  "wish": case["wish"], "ell_reg": case["ell_reg"], "stop_after": case["stop_after"],
                  "n_quota": len(case["quotas"])}
        fields.update(more or {})
        json.dump(fields, f)
    return jpath, bpath


def load_dump(json_path, bin_path):
    with open(json_path) as f:
        man = json.load(f)
    raw = np.fromfile(bin_path, np.uint8)
    buffers = {}
    for ent in man["entries"]:
        dt = np.dtype(DTYPES[ent["dtype"]]).newbyteorder("<")
        buffers[(ent["stage"], ent["name"])] = np.frombuffer(raw, dt, ent["count"], ent["offset"]).copy()
    return {"derived": man["derived"], "violations": man["violations"], "inputs_changed": man["inputs_changed"],
            "hip_error": man["hip_error"], "refused": man["refused"], "buffers": buffers}


# ---------------------------------------------------------------------------------------------------------- the model
def model_of(case):
    """everything the stages are expected to write, from tests/pass_major_model.py (cached in the case)"""
    if "_model" in case:
        return case["_model"]
    g, shift, ltot = case["grid"], case["shift"], case["ltot"]
    lengths, poff = case["lengths"], case["poff"]
    n, n_ranges = int(case["starts"].size), int(g["n_ranges"])
    contig = pm.contig_of_reads(case["roff"])
    cs, ce = pm.clamped(case["starts"], contig, lengths), pm.clamped(case["ends"], contig, lengths)
    gs, ge = (poff[contig] + cs).astype(np.int64), (poff[contig] + ce).astype(np.int64)
    vs = (g["vbase"][contig] + cs).astype(np.uint32)              # the grid's axis
    regular = pm.regular_reads(case["starts"], case["ends"], case["ell_reg"])
    keys16, idx16, cntp, lstw = pm.producer(vs, shift, n_ranges, regular)
    Tp = pm.scan_table(cntp)
    desc, range_start = pm.descriptors(Tp, lstw, n, n_ranges)
    pitch, stride = pm.pitch_for(n), pm.stride_for(n_ranges)
    # record slots and slots inside a slice's padded group
    rec = np.zeros(pitch * stride, bool)
    grp = np.zeros(pitch * stride, bool)
    for d, P in zip(*np.nonzero(lstw >> 16)):
        at = int(P) * stride + int(lstw[d, P] & 0xFFFF) * 64
        rec[at:at + int(lstw[d, P] >> 16)] = True
        grp[at:at + int(cntp[d, P])] = True
    # the table stage's working words: per (range, part of the row) the padded and the true record count
    per = (pitch + TABLE_PARTS - 1) // TABLE_PARTS
    work = np.zeros((256, TABLE_PARTS, 2), np.uint32)
    for y in range(TABLE_PARTS):
        lo, hi = min(pitch, y * per), min(pitch, (y + 1) * per)
        work[:, y, 0] = cntp[:, lo:hi].sum(axis=1)
        work[:, y, 1] = (lstw[:, lo:hi] >> 16).sum(axis=1)
    m = {"n": n, "n_ranges": n_ranges, "pitch": pitch, "stride": stride, "n_pass": (n + pm.PASS - 1) // pm.PASS,
         "gs": gs, "ge": ge, "regular": regular, "keys16": keys16, "idx16": idx16, "cntp": cntp, "lstw": lstw, "rec": rec,
         "grp": grp, "Tp": Tp, "desc": desc, "range_start": range_start, "work": work.reshape(-1),
         "max_load": pm.loads(cntp, lstw), "stats012": pm.statistics(case["starts"], case["ends"], contig, lengths),
         "boff": pm.bucket_offsets(gs[regular], ltot), "empty": pm.empty_positions(gs[regular], ltot)}
    if case["ell_reg"]:
        m["exc_cnt"], m["exc_groups"], m["exc_over"] = pm.exception_lists(gs, ge, regular)
    words = np.zeros(3 * 256 + lengths.size + 1, np.uint32)
    for k, name in enumerate(("pos0", "live", "contig")):
        words[256 * k:256 * k + n_ranges] = g[name].astype(np.uint32)
    words[768:] = g["vbase"].astype(np.uint32)
    m["grid_words"] = words
    case["_model"] = m
    return m


def expected_masks(case):
    """the keep mask every quota vector of the case asks for (cached: the plain reference is computed once)"""
    m = model_of(case)
    if "masks" not in m:
        m["masks"] = [pm.expected_mask(m["gs"], q, m["regular"]) for q in case["quotas"]]
    return m["masks"]


def pack_mask(bits):
    """bool per read -> the keep mask's 64-bit words"""
    n = bits.size
    padded = np.zeros((n + 63) // 64 * 64, np.uint8)
    padded[:n] = bits
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def model_dump(case, exc_cap=None):
    """the dump a correct device would hand back (padding slots inside a group: zero; never-written words: the canary)"""
    m = model_of(case)
    n, pitch = m["n"], m["pitch"]
    stop = case["stop_after"]
    buf = {("in", "grid"): m["grid_words"].copy()}
    keys16 = np.where(m["rec"], m["keys16"], np.where(m["grp"], 0, CANARY16)).astype(np.uint16)
    idx16 = np.where(m["rec"], m["idx16"], np.where(m["grp"], 0, CANARY16)).astype(np.uint16)
    cnt_a = np.concatenate([m["cntp"].reshape(-1), np.full(4, CANARY32, np.uint32)]).astype(np.uint32)
    stats = np.array([m["stats012"][0], m["stats012"][1], m["stats012"][2], 0, 0, 0, 0, 0] + [CANARY32] * 4, np.uint32)
    derived = {"shift": case["shift"], "n_ranges": m["n_ranges"], "aligned": int(case["grid"]["aligned"]), "pitch": pitch,
               "stride": m["stride"], "slots": pitch * m["stride"], "exc_cap": 0}
    if case["ell_reg"]:
        cap = exc_cap if exc_cap is not None else pitch * 8 * pm.EXC_PER_WAVE + NU_OVERFLOW
        derived["exc_cap"] = cap
        exc = np.full(cap * 7 + 2 * (cap // pm.EXC_PER_WAVE + 4) + 8, CANARY32, np.uint32)
        for g, ent in m["exc_groups"].items():
            for a in range(3):
                exc[a * cap + g * pm.EXC_PER_WAVE:a * cap + g * pm.EXC_PER_WAVE + ent.shape[0]] = ent[:, a]
        over = m["exc_over"][::-1]                       # (any order)
        for a in range(3):
            exc[a * cap + cap - NU_OVERFLOW:a * cap + cap - NU_OVERFLOW + over.shape[0]] = over[:, a]
        exc[6 * cap:6 * cap + pitch * 8] = m["exc_cnt"]
        stats[4], stats[6] = int(m["exc_cnt"].sum()) + over.shape[0], over.shape[0]
        buf[("A", "exc")] = exc
    buf.update({("A", "keys16"): keys16, ("A", "idx16"): idx16, ("A", "cnt_tab"): cnt_a, ("A", "lst_tab"): m["lstw"].reshape(-1).copy(),
                ("A", "stats"): stats.copy(), ("A", "mask"): np.zeros((n + 63) // 64, np.uint64)})
    if stop >= "B":
        G = int(m["Tp"][-1]) // 64
        desc = np.full(pitch * m["stride"] // 64, CANARY32, np.uint32)
        desc[:G] = m["desc"]
        buf.update({("B", "cnt_tab"): np.concatenate([m["Tp"], np.full(3, CANARY32, np.uint32)]).astype(np.uint32), ("B", "desc"): desc,
                    ("B", "work"): m["work"].copy(), ("B", "range_start"): m["range_start"].copy(),
                    ("B", "max_load"): np.array(m["max_load"], np.uint32), ("B", "scalars"): np.zeros(16, np.uint32)})
    if stop >= "C":
        stats_c = stats.copy()
        stats_c[3] = m["empty"]
        buf.update({("C", "boff"): m["boff"].copy(), ("C", "stats"): stats_c})
    if stop >= "D":
        for k, bits in enumerate(expected_masks(case)):
            sc = np.zeros(16, np.uint32)
            sc[0] = int(bits.sum())
            buf[("D%d" % k, "mask")] = pack_mask(bits)
            buf[("D%d" % k, "scalars")] = sc
        for name, src in (("keys16", ("A", "keys16")), ("idx16", ("A", "idx16")), ("cnt_tab", ("B", "cnt_tab")), ("desc", ("B", "desc")),
                          ("boff", ("C", "boff"))):
            buf[("end", name)] = buf[src].copy()
    return {"derived": derived, "violations": [], "inputs_changed": [], "hip_error": None, "refused": None, "buffers": buf}


# ------------------------------------------------------------------------------------------------------ the comparison
def _fail(stage, name, what):
    raise StageMismatch("stage %s buffer %s: %s" % (stage, name, what))


def _same(stage, name, got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        _fail(stage, name, "%s%d words, expected %d" % (what, got.size, want.size))
    bad = np.nonzero(got != want)[0]
    if bad.size:
        i = int(bad[0])
        _fail(stage, name, "%sindex %d is %d (0x%x), expected %d (0x%x); %d differ" % (what, i, int(got[i]), int(got[i]), int(want[i]),
                                                                                     int(want[i]), bad.size))


def _get(dump, stage, name):
    if (stage, name) not in dump["buffers"]:
        _fail(stage, name, "not in the dump")
    return dump["buffers"][(stage, name)]


def compare_stage_dump(case, dump):
    """raises StageMismatch on the first difference, naming the stage and the buffer"""
    if dump["refused"]:
        raise StageMismatch("stage setup buffer -: the driver refused the case: %s" % dump["refused"])
    if dump["hip_error"]:
        raise StageMismatch("stage ? buffer -: HIP error: %s" % dump["hip_error"])
    for v in dump["violations"]:
        _fail(v["stage"], v["buffer"], "guard band touched on the %s side, first at byte %d" % (v["side"], v["offset"]))
    m = model_of(case)
    n, pitch, stride, n_ranges, n_pass = m["n"], m["pitch"], m["stride"], m["n_ranges"], m["n_pass"]
    stop, filt = case["stop_after"], case["ell_reg"] != 0
    der = dump["derived"]
    for key, want in (("shift", case["shift"]), ("n_ranges", n_ranges), ("aligned", int(case["grid"]["aligned"])), ("pitch", pitch),
                      ("stride", stride), ("slots", pitch * stride)):
        if int(der[key]) != int(want):
            _fail("setup", "derived", "%s is %d, expected %d" % (key, der[key], want))
    if case["expect_aligned"] is not None and int(der["aligned"]) != case["expect_aligned"]:
        _fail("setup", "derived", "the plan took grid %d, the case expects %d" % (der["aligned"], case["expect_aligned"]))
    _same("in", "grid", _get(dump, "in", "grid"), m["grid_words"])

    # ---- stage A: the producer
    cnt = _get(dump, "A", "cnt_tab")
    _same("A", "cnt_tab", cnt[:256 * pitch], m["cntp"].reshape(-1))
    _same("A", "cnt_tab", cnt[256 * pitch:], np.full(4, CANARY32, np.uint32), "behind the table: ")
    lst = _get(dump, "A", "lst_tab")
    _same("A", "lst_tab", lst, m["lstw"].reshape(-1))
    # (the model's own tables: nothing in a padding pass, no records in a row at or beyond the grid's ranges)
    assert not m["cntp"][:, n_pass:].any() and not m["lstw"][:, n_pass:].any()
    assert not m["cntp"][n_ranges:].any() and not (m["lstw"][n_ranges:] >> 16).any()
    for name in ("keys16", "idx16"):
        got = _get(dump, "A", name)
        if got.size != pitch * stride:
            _fail("A", name, "%d slots, expected %d" % (got.size, pitch * stride))
        at = np.nonzero(m["rec"])[0]
        _same("A", name, got[at], m[name][at], "record slots (stable by read index): ")
        out = np.nonzero(~m["grp"])[0]
        bad = out[got[out] != CANARY16]
        if bad.size:
            _fail("A", name, "slot %d, outside every slice's padded group, was written (0x%x); %d such slots" % (int(bad[0]), int(got[bad[0]]), bad.size))
    stats = _get(dump, "A", "stats")
    want_stats = np.array(list(m["stats012"]) + [0, 0, 0, 0, 0] + [CANARY32] * 4, np.uint32)
    if filt:
        n_over = m["exc_over"].shape[0]
        want_stats[4], want_stats[6] = int(m["exc_cnt"].sum()) + n_over, n_over
    _same("A", "stats", stats, want_stats)
    if int(stats[2]) != case["expect_bad"]:
        _fail("A", "stats", "the bad flag is %d, the case expects %d" % (int(stats[2]), case["expect_bad"]))
    _same("A", "mask", _get(dump, "A", "mask"), np.zeros((n + 63) // 64, np.uint64))
    if filt:
        exc = _get(dump, "A", "exc")
        cap = int(der["exc_cap"])
        if cap < pitch * 8 * pm.EXC_PER_WAVE + NU_OVERFLOW or exc.size < 7 * cap:
            _fail("A", "exc", "capacity %d / %d words" % (cap, exc.size))
        want = np.full(exc.size, CANARY32, np.uint32)
        for g, ent in m["exc_groups"].items():
            for a in range(3):
                want[a * cap + g * pm.EXC_PER_WAVE:a * cap + g * pm.EXC_PER_WAVE + ent.shape[0]] = ent[:, a]
        want[6 * cap:6 * cap + pitch * 8] = m["exc_cnt"]
        o0 = cap - NU_OVERFLOW
        got_over = np.stack([exc[a * cap + o0:a * cap + o0 + n_over] for a in range(3)], axis=1).astype(np.int64)
        want_over = m["exc_over"]
        key = lambda rows: rows[np.lexsort((rows[:, 1], rows[:, 0], rows[:, 2]))]
        if got_over.shape != want_over.shape or not np.array_equal(key(got_over), key(want_over)):
            _fail("A", "exc", "the overflow region's %d entries are not the model's set" % n_over)
        for a in range(3):
            want[a * cap + o0:a * cap + o0 + n_over] = exc[a * cap + o0:a * cap + o0 + n_over]
        _same("A", "exc", exc, want, "lists, counts and never-written slots: ")
    if stop == "A":
        return _finish(case, dump)

    # ---- stage B: row sums and tables
    tab = _get(dump, "B", "cnt_tab")
    _same("B", "cnt_tab", tab[:256 * pitch + 1], m["Tp"], "Tp (exclusive scan, the total at [256 pitch]): ")
    _same("B", "cnt_tab", tab[256 * pitch + 1:], np.full(3, CANARY32, np.uint32), "behind the total: ")
    desc = _get(dump, "B", "desc")
    G = int(m["Tp"][-1]) // 64
    if desc.size != pitch * stride // 64:
        _fail("B", "desc", "%d words, expected %d" % (desc.size, pitch * stride // 64))
    _same("B", "desc", desc[:G], m["desc"])
    _same("B", "desc", desc[G:], np.full(desc.size - G, CANARY32, np.uint32), "beyond the last wave-slot: ")
    _same("B", "work", _get(dump, "B", "work"), m["work"])
    _same("B", "range_start", _get(dump, "B", "range_start"), m["range_start"])
    _same("B", "max_load", _get(dump, "B", "max_load"), np.array(m["max_load"], np.uint32))
    _same("B", "scalars", _get(dump, "B", "scalars"), np.zeros(16, np.uint32))
    if stop == "B":
        return _finish(case, dump)

    # ---- stage C: bucket offsets
    _same("C", "boff", _get(dump, "C", "boff"), m["boff"])
    want_stats[3] = m["empty"]
    _same("C", "stats", _get(dump, "C", "stats"), want_stats)
    if stop == "C":
        return _finish(case, dump)

    # ---- stage D: the walk and its settling tail, per quota vector
    for k, want_bits in enumerate(expected_masks(case)):
        stage = "D%d" % k
        got = _get(dump, stage, "mask")
        if got.size != (n + 63) // 64:
            _fail(stage, "mask", "%d words, expected %d" % (got.size, (n + 63) // 64))
        bits = np.unpackbits(got.astype("<u8").view(np.uint8), bitorder="little").astype(bool)
        if bits[n:].any():
            _fail(stage, "mask", "bit %d is set, at or above n = %d" % (n + int(np.nonzero(bits[n:])[0][0]), n))
        _same(stage, "mask", bits[:n], want_bits, "read ")
        sc = _get(dump, stage, "scalars")
        want_sc = np.zeros(16, np.uint32)
        want_sc[0] = int(bits.sum())
        _same(stage, "scalars", sc, want_sc, "kept total = popcount of the mask: ")
    if not case["quotas"]:
        _fail("D0", "mask", "the case has no quota vector")
    for name, src in (("keys16", "A"), ("idx16", "A"), ("cnt_tab", "B"), ("desc", "B"), ("boff", "C")):
        _same("end", name, _get(dump, "end", name), _get(dump, src, name), "changed by the walk: ")
    return _finish(case, dump)


def _finish(case, dump):
    if dump["inputs_changed"]:
        _fail("end", dump["inputs_changed"][0], "a read-only input was changed")
