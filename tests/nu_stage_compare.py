"""The near-uniform route's kernels one stage at a time: the case and dump files of tests/cpp/nu_stage_driver.hip, and
compare_stage_dump(), which holds every buffer the driver hands back against the device-shaped host model
(tests/nu_stage_model.py), stage after stage.  load_dump and the naming of stage, buffer and first differing index are
those of tests/pm_stage_compare.py.

A dump is {"derived", "violations", "inputs_changed", "hip_error", "refused", "buffers": {(stage, name): array}}; the
stages are "0" (the route's two looks at the spans: four words), "S" (launch_nu_setup), "cuts" (form gen_cuts: the exact
stretch table), "1.sweep", "1.round", "2.sweep", ... and "mark" (after a round that applied nothing).  Of the list's pick
and key the driver dumps the groups' slots and the used part of the overflow region; that no other slot lost its canary,
and that the list's inputs are what they were, it checks itself and reports as a violation / among "inputs_changed".

Comparison is plain equality with the model over each buffer's whole extent (never-written words = the canary) -- ce,
nadj, selend_prev, pick, key (per exception), viol_key (per contig), viol_idx, both sweep_from, both marks, both dirty,
the cells' counts and starts, goff, dense, the segment table, the mask -- except:
  * suspects, the cells' sorted slots (per cell), replay_list and far_list are filled in atomic order: each is compared
    as a multiset of exception ids (a slot of the suspects list is read through that list).  Their counts -- state[4],
    [14], [15] and the cells' starts -- are exact.  Behind a list's used part earlier rounds' entries may remain, up to
    the most any round so far has written; from there on the canary must stand.
  * state[5] and state[8..13] are debug words written without ordering: not compared.
 Three more, which the buffers' own layout forces (DESIGN.md 4.3 "Stage test" lists them too):
  * selend has spare words behind position ltot that idle lanes write: positions [0, ltot) are compared, and before the
    first sweep the whole buffer must be the canary.
  * scalars: the kept total (words 0, 1); the sweeps' iteration statistics behind it hold clock readings.
  * After flag 2 (suspects list full) which suspects were listed is that order's: flag 2 itself, state[4] and the guards
    are compared, and the case ends there.
A failure names the stage, the buffer and the first differing index."""
import json
import os

import numpy as np

import nu_stage_model as nm
from pm_stage_compare import CANARY32, NU_OVERFLOW, StageMismatch, _fail, _get, _same, load_dump  # noqa: F401

STATE_FREE = (5, 8, 9, 10, 11, 12, 13)
PLAIN = ("ce", "nadj", "selend_prev", "pick", "pick_over", "key", "key_over", "viol_key", "viol_idx", "sweep_from0",
         "sweep_from1", "marks0", "marks1", "dirty0", "dirty1", "bins_count", "bins_start", "goff", "goff_total", "dense", "mask")
NOMINAL_CAP = 8 * nm.GROUP + NU_OVERFLOW     # the smallest list the product sizes (the CPU tests' stand-in)


def write_case(case, directory):
    """-> paths of case.json, case.bin (tests/cpp/nu_stage_driver.hip has the format)"""
    jpath, bpath = os.path.join(str(directory), "case.json"), os.path.join(str(directory), "case.bin")
    with open(bpath, "wb") as f:
        f.write(np.asarray(case["starts"]).astype("<u4").tobytes())
        f.write(np.asarray(case["ends"]).astype("<u4").tobytes())
        f.write(np.asarray(case["lengths"]).astype("<u8").tobytes())
        f.write(np.asarray(case["boff"]).astype("<u4").tobytes())
        f.write(np.asarray(case["cnt"]).astype("<u4").tobytes())
        for rows in (case["slots"], case["over"]):
            for a in range(3):
                f.write(rows[:, a].astype("<u4").tobytes())
    with open(jpath, "w") as f:
        json.dump({"n": case["n"], "n_contigs": int(len(case["lengths"])), "ltot": int(np.sum(case["lengths"])), "ell": case["ell"],
                   "M": case["M"], "n_groups": int(len(case["cnt"])), "n_over": int(case["over"].shape[0]),
                   "suspects_cap": case["suspects_cap"], "rounds_max": case["rounds_max"], "form": case["form"]}, f)
    return jpath, bpath


def model_of(case, cap=NOMINAL_CAP):
    """the model's run of the case under a list of `cap` slots (cached in the case)"""
    if case.get("_nu_cap") != cap:
        case["gcap"] = cap - NU_OVERFLOW
        case["_nu_run"] = nm.run(case)
        case["_nu_cap"] = cap
    return case["_nu_run"]


def model_dump(case, cap=NOMINAL_CAP):
    """the dump a correct device would hand back (lists in the model's order)"""
    run = model_of(case, cap)
    buf = {}
    for stage, buffers, _ in run["stages"]:
        for name, arr in buffers.items():
            buf[(stage, name)] = arr.copy()
    flags = run["flags"]
    derived = {"cap": cap, "rounds": run["rounds"], "flags": flags, "settled": int(run["settled"])}
    return {"derived": derived, "violations": [], "inputs_changed": [], "hip_error": None,
            "refused": "the sweep does not take this span and cap" if run["refused"] else None, "buffers": buf}


def _ids(stage, name, suspects, slots, n_sus):
    slots = np.asarray(slots, np.int64)
    bad = np.nonzero(slots >= n_sus)[0]
    if bad.size:
        _fail(stage, name, "index %d is %d, no slot of the %d suspects" % (int(bad[0]), int(slots[bad[0]]), n_sus))
    return np.sort(suspects[slots, 0])


def _compare_lists(stage, got_all, want_all, counts, cap, starts, n_cells):
    got, want = got_all.reshape(-1), want_all.reshape(-1)
    if got.shape != want.shape:
        _fail(stage, "lists", "%d words, expected %d" % (got.size, want.size))
    n_sus, n_rep, n_far, high = counts["suspects"], counts["replay"], counts["far"], counts["high"]
    gs, ws = got[:2 * n_sus].reshape(-1, 2), want[:2 * n_sus].reshape(-1, 2)
    order = lambda a: a[np.lexsort((a[:, 1], a[:, 0]))]  # noqa: E731
    _same(stage, "suspects", order(gs).reshape(-1), order(ws).reshape(-1), "(pairs of exception and contig, sorted) ")
    _same(stage, "suspects", got[2 * high["suspects"]:2 * cap], np.full(2 * (cap - high["suspects"]), CANARY32, np.uint32),
          "behind the most any round listed (%d): " % high["suspects"])
    for name, at, used, hw in (("replay_list", 3 * cap, n_rep, high["replay"]), ("far_list", 4 * cap, n_far, high["far"])):
        _same(stage, name, _ids(stage, name, gs, got[at:at + used], n_sus), _ids(stage, name, ws, want[at:at + used], n_sus),
              "(exception ids, sorted) ")
        _same(stage, name, got[at + hw:at + cap], np.full(cap - hw, CANARY32, np.uint32), "behind the most any round listed (%d): " % hw)
    for cc in range(n_cells):
        a, b = int(starts[cc]), int(starts[cc + 1])
        if a == b:
            continue
        _same(stage, "bins.sorted", _ids(stage, "bins.sorted", gs, got[2 * cap + a:2 * cap + b], n_sus),
              _ids(stage, "bins.sorted", ws, want[2 * cap + a:2 * cap + b], n_sus), "cell %d (exception ids, sorted) " % cc)
    hw = high["sorted"]
    _same(stage, "bins.sorted", got[2 * cap + hw:3 * cap], np.full(cap - hw, CANARY32, np.uint32), "behind the most any round listed (%d): " % hw)


def compare_stage_dump(case, dump):
    """raises StageMismatch on the first difference, naming the stage and the buffer; -> how the device and the model
    ended: {"rounds", "flags", "settled"} of either"""
    if dump["hip_error"]:
        raise StageMismatch("stage ? buffer -: HIP error: %s" % dump["hip_error"])
    for v in dump["violations"]:
        raise StageMismatch("stage %s buffer %s: guard violation, %s side, offset %d" % (v["stage"], v["buffer"], v["side"], v["offset"]))
    if dump["inputs_changed"]:
        raise StageMismatch("stage ? buffer %s: an input was written" % dump["inputs_changed"][0])
    cap = int(dump["derived"]["cap"]) if "cap" in dump["derived"] else NOMINAL_CAP
    run = model_of(case, cap)
    m = run["model"]
    ltot, scap = m.ltot, m.cap_sus
    swept = False
    for stage, want, counts in run["stages"]:
        if stage == "0":
            _same(stage, "span_stats", _get(dump, stage, "span_stats"), want["span_stats"])
            continue
        state_g, state_w = _get(dump, stage, "state"), want["state"]
        if counts["flag2"]:
            _same(stage, "state", [int(state_g[2]) & 2, int(state_g[4])], [2, int(state_w[4])], "(flag 2, suspects) ")
            break
        keep = np.array([i for i in range(16) if i not in STATE_FREE])
        if state_g.size != 16:
            _fail(stage, "state", "%d words, expected 16" % state_g.size)
        bad = [int(i) for i in keep if int(state_g[i]) != int(state_w[i])]
        if bad:
            _fail(stage, "state", "index %d is %d, expected %d" % (bad[0], int(state_g[bad[0]]), int(state_w[bad[0]])))
        for name in PLAIN:
            _same(stage, name, _get(dump, stage, name), want[name])
        if "segs" in want:
            _same(stage, "segs", _get(dump, stage, "segs"), want["segs"])
        swept = swept or stage.endswith(".sweep")
        sel = _get(dump, stage, "selend")
        if swept:
            _same(stage, "selend", sel[:ltot], want["selend"][:ltot])
            if sel.size != ltot + 8:
                _fail(stage, "selend", "%d words, expected %d" % (sel.size, ltot + 8))
        else:
            _same(stage, "selend", sel, want["selend"])
        _same(stage, "kept_total", _get(dump, stage, "scalars")[:2], want["scalars"][:2])
        _compare_lists(stage, _get(dump, stage, "lists"), want["lists"], counts, scap, want["bins_start"], m.n_cells)
    # how it ended
    if run["refused"] != bool(dump["refused"]):
        raise StageMismatch("stage end buffer -: the driver %s the case (%s), the model %s" % (
            "refused" if dump["refused"] else "ran", dump["refused"], "expects a refusal" if run["refused"] else "does not"))
    d = dump["derived"]
    ended = {"rounds": d.get("rounds", run["rounds"] if run["refused"] else None), "flags": d.get("flags", 0), "settled": d.get("settled", 0),
             "model_rounds": run["rounds"], "model_flags": run["flags"], "model_settled": int(run["settled"])}
    if not run["refused"]:
        flags_g, flags_w = int(ended["flags"]), int(run["flags"])
        if m.stopped_at_flag2:
            flags_g, flags_w = flags_g & 2, flags_w & 2
        _same("end", "derived", [int(ended["rounds"]), flags_g, int(ended["settled"])], [run["rounds"], flags_w, int(run["settled"])],
              "(rounds, flags, settled) ")
    stages_w = [s for s, _, _ in run["stages"]]
    extra = sorted({s for s, _ in dump["buffers"]} - set(stages_w))
    if extra and not m.stopped_at_flag2:
        _fail(extra[0], "-", "a stage the model does not reach")
    return ended
