"""The host side of the near-uniform stage test (tests/test_gpu_nu_stages.py), without a GPU: the device-shaped model
(tests/nu_stage_model.py) ends on the oracle's selection on every case that is no give-up case, every case shows the
edge it is there for, and the comparer (tests/nu_stage_compare.py) accepts the model's own dump and rejects a dump with
one word changed in any buffer it compares -- which is how the GPU test would fail.  The model's event-driven sweep is a
transcription of the chain's recurrence; it is pinned here to the independent greedy: equal on every sweep in which the
greedy holds no surplus and on every last round, and different only in the listed rounds, in the listed direction."""
import numpy as np
import pytest

import nu_stage_compare as nsc
import nu_stage_model as nm
from nu_stage_cases import CASES, GIVE_UP

_built = {}


def built(name):
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]


def _slots_of(m, s, e):
    return [x for x in range(m.n_exc) if m.gs[x] == s and m.ge[x] == e]


def _unselects(m):
    return sum(1 for q in m.questions for a in q if a[1] == "unselect")


def _moved_earlier(m):
    return sum(1 for q in m.questions for a in q if a[1] == "earlier")


def _check_ties(run):
    m = run["model"]
    for s in (2100, 900):
        lot = sorted(_slots_of(m, s, s + 40), key=lambda x: m.idx[x])
        assert len(lot) == 9
        picks = [m.pick[x] for x in lot]
        if s == 2100:
            assert picks == [s] * 4 + [nm.UNPICKED] * 5     # the four smallest indices, at one time
        else:                                               # (among other reads: whatever is wanted, the smallest indices)
            k = sum(1 for p in picks if p != nm.UNPICKED)
            assert picks[k:] == [nm.UNPICKED] * (9 - k)
    assert m.seen.get("cut", 0) > 0


def _check_prepick(run):
    m = run["model"]
    picks = dict((st, w) for st, w, _ in run["stages"])["S"]["pick"]
    (a,), (b,) = _slots_of(m, 103, 120), _slots_of(m, 203, 220)
    assert m.cov_regular(103) + m.ce[104] == m.M and m.cov_regular(203) + m.ce[204] == m.M + 1
    assert picks[m.place[a][1]] == 103 and picks[m.place[b][1]] == nm.UNPICKED


def _check_restart_ev(run):
    m = run["model"]
    assert m.lengths[0] >= 200 * m.ell and m.restarts[0][0] in (64, 128), m.restarts


def _check_restart_cuts(run):
    m = run["model"]
    assert m.ltot >= 128 * m.ell and len(m.seg) > 2 and any(q != nm.NONE32 for q in m.cuts)
    marked = dict((st, w) for st, w, _ in run["stages"])["1.round"]["marks1"][:len(m.seg)]
    assert marked.any() and not marked.all(), marked      # questions in only some stretches


def _check_layout(run):
    m = run["model"]
    name = m.case["name"]
    assert {0, 1, 127, 128} <= set(m.cnt)
    assert m.n_over == {"layout_over0": 0, "layout_over1": 1}.get(name, m.n_over)
    if name == "layout_over_many":
        assert m.n_over >= 200 and any(m.place[x][0] == "o" for q in m.questions for x, _ in q)


def _check_contigs(run):
    m = run["model"]
    buckets = [(m.ge[x] - m.ell + 1, m.poff[m.contig[x]]) for x in range(m.n_exc)]
    assert any(b < 0 for b, _ in buckets) and any(0 <= b < c0 for b, c0 in buckets)
    assert m.lengths[1] == 0 and m.lengths[2] < m.ell and max(m.ge) == m.ltot - 1
    assert sum(1 for x in range(m.n_exc) if m.contig[x] == 2) > m.M


def _check_none_later(run):
    """round 1 leaves unresolved keys that are not the contig's earliest (no flag, four questions applied); round 2
    replays those exceptions again although no cell they read is dirty -- the key they kept says so -- and one of them
    is now the earliest: flag 1.  (k_nu_verify keeps a key WITHOUT a replay only for an exception that ends before the
    block the round swept from; its release then lies before every applied question's time, so it was the earliest the
    round before and the route had given up: that branch cannot be met from the host's loop, and no case meets it.)"""
    m = run["model"]
    assert run["rounds"] == 2 and run["flags"] == 1 and len(m.questions[0]) == 4
    assert m.seen.get("unresolved", 0) == 14 and m.seen.get("unresolved_again_no_dirty_cell", 0) == 7
    assert "unresolved_key_kept" not in m.seen


EXPECT = {
    "rounds_ev": lambda r: (r["rounds"] >= 3 and _unselects(r["model"]) >= 1 and _moved_earlier(r["model"]) >= 1) or pytest.fail("too few rounds"),
    "rounds_gen": lambda r: (r["rounds"] >= 3 and _unselects(r["model"]) >= 1) or pytest.fail("too few rounds"),
    "ties": _check_ties, "prepick": _check_prepick, "restart_ev": _check_restart_ev, "restart_cuts": _check_restart_cuts,
    "layout_over0": _check_layout, "layout_over1": _check_layout, "layout_over_many": _check_layout,
    "contigs_ev": _check_contigs, "contigs_gen": _check_contigs,
    "reach_far": lambda r: r["model"].seen.get("far_anchor", 0) > 0 or pytest.fail("no far replay"),
    "reach_cut": lambda r: r["model"].seen.get("far_cut", 0) > 0 or pytest.fail("no far replay from a cut point"),
    "reach_none": lambda r: (r["model"].seen.get("unresolved", 0) > 0 and r["flags"] == 1) or pytest.fail("no unresolved key"),
    "reach_none_later": lambda r: _check_none_later(r),
    "limit_others": lambda r: r["flags"] == 4 or pytest.fail("flag 4 not set"),
    "limit_suspects": lambda r: (r["flags"] & 2) == 2 or pytest.fail("flag 2 not set"),
    "span256_ev_M63_refused": lambda r: r["refused"] or pytest.fail("not refused"),
    "span256_ev_M62": lambda r: (not r["refused"] and r["settled"]) or pytest.fail("refused"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_model_ends_on_the_oracles_selection(name, oracle):
    case = built(name)
    assert case["n"] <= 8000
    run = nsc.model_of(case)
    if name in EXPECT:
        EXPECT[name](run)
    if name in GIVE_UP:
        assert not run["settled"]
        return
    m = run["model"]
    assert run["settled"] and run["flags"] == 0 and run["rounds"] <= case["rounds_max"]
    want = np.unpackbits(oracle.solve(case["starts"], case["ends"], case["lengths"], case["M"], case["roff"]).view(np.uint8),
                         bitorder="little")[:case["n"]].astype(bool)
    kept = np.zeros(case["n"], bool)
    for x in range(m.n_exc):
        kept[m.idx[x]] = m.pick[x] != nm.UNPICKED
    exc = ~case["regular"]
    assert np.array_equal(kept[exc], want[exc]), "selected exceptions: first difference at read %d" % np.flatnonzero(exc & (kept != want))[0]
    S = np.array(m.selend, np.int64) - np.array(m.boff[:-1], np.int64)
    S_want = np.bincount(case["gs"][case["regular"] & want], minlength=m.ltot)
    assert np.array_equal(S, S_want), "S(p): first difference at position %d" % np.flatnonzero(S != S_want)[0]
    # ... and the mask of the last stage is those exceptions
    assert run["stages"][-1][0] == "mark"
    bits = np.unpackbits(run["stages"][-1][1]["mask"].view(np.uint8), bitorder="little")[:case["n"]].astype(bool)
    assert np.array_equal(bits, want & exc)


# The event-driven form's sweeps against the independent greedy (nu_stage_model.sweep_contig_events has the rule): the
# rounds in which the two may differ, and whether the chain keeps more reads (+1) or fewer (-1) than the greedy there.
# Every other sweep of every event-driven case must equal the greedy.
EV_DIFFERS = {
    "span33_ev": {2: +1},
    "rounds_ev": {2: +1, 3: +1, 5: +1, 6: +1, 7: +1, 8: +1, 9: +1},
    "layout_over0": {2: +1, 3: -1, 5: +1}, "layout_over1": {2: +1, 3: -1, 5: +1}, "layout_over_many": {2: +1, 3: -1, 5: +1},
    "restart_ev": {2: +1},
}


@pytest.mark.parametrize("name", [n for n in CASES if built(n)["form"] == "ev" and GIVE_UP.get(n) != "refused"])
def test_event_recurrence_is_the_greedy_but_for_a_surplus(name):
    case = built(name)
    assert case["form"] == "ev"
    run = nsc.model_of(case)
    sweeps = run["model"].sweeps
    assert len(sweeps) == run["rounds"]
    differs = {}
    for r, log in enumerate(sweeps, 1):
        if log["surplus"] == 0:
            assert log["equal"], "round %d: no surplus in the greedy, and yet the recurrence differs from it" % r
        if not log["equal"]:
            differs[r] = (log["kept_more"] > 0) - (log["kept_more"] < 0)
    assert differs == EV_DIFFERS.get(name, {})
    if run["settled"]:
        assert sweeps[-1]["surplus"] == 0 and sweeps[-1]["equal"], "the last round's sweep is not the greedy's"


def _mutations(case, dump):
    m = nsc.model_of(case)["model"]
    key = dump["buffers"][("1.round", "key")]
    asked = int(np.flatnonzero((key != nm.NOKEY) & (key != nm.CANARY64))[0])
    picked = int(np.flatnonzero(dump["buffers"][("1.round", "pick")] < m.ltot)[0])
    return {
        "key with the kind flipped": (("1.round", "key"), asked, lambda v: v ^ np.uint64(1)),
        "pick off by one": (("1.round", "pick"), picked, lambda v: v + np.uint32(1)),
        "one nadj entry": (("1.round", "nadj"), m.ltot // 2, lambda v: v + np.uint32(1)),
        "one selend entry": (("2.sweep", "selend"), m.ltot // 3, lambda v: v + np.uint32(1)),
        "a mark": (("1.round", "marks1"), 1, lambda v: v ^ np.uint32(1)),
        "a dirty cell": (("1.round", "dirty1"), 3, lambda v: v ^ np.uint32(1)),
        "a sweep_from not rounded to 64": (("1.round", "sweep_from1"), 0, lambda v: np.uint32(65)),
        "a mask bit": (("mark", "mask"), 2, lambda v: v ^ np.uint64(1 << 17)),
        "a viol_key": (("1.round", "viol_key"), 0, lambda v: v + np.uint64(2)),
        "a state word": (("1.round", "state"), 14, lambda v: v + np.uint32(1)),
        "a suspect": (("1.round", "lists"), 0, lambda v: v + np.uint32(1)),
        "a word behind the lists": (("1.round", "lists"), 2 * m.cap_sus - 1, lambda v: np.uint32(0)),
        "a cell's start": (("1.round", "bins_start"), 2, lambda v: v + np.uint32(1)),
        "a stretch of the table": (("cuts", "segs"), m.windows + 2, lambda v: v + np.uint32(1)),
        "ce": (("S", "ce"), 5, lambda v: v + np.uint32(1)),
        "the fullest bin's span": (("0", "span_stats"), 3, lambda v: v + np.uint32(1)),
        "selend_prev": (("1.round", "selend_prev"), 7, lambda v: v + np.uint32(1)),
    }


MUTATIONS = ["key with the kind flipped", "pick off by one", "one nadj entry", "one selend entry", "a mark", "a dirty cell",
             "a sweep_from not rounded to 64", "a mask bit", "a viol_key", "a state word", "a suspect", "a word behind the lists",
             "a cell's start", "a stretch of the table", "ce", "selend_prev", "the fullest bin's span"]


def test_comparer_accepts_the_models_dump():
    for name in ("restart_cuts", "contigs_ev", "limit_suspects", "span256_ev_M63_refused", "reach_none"):
        case = built(name)
        ended = nsc.compare_stage_dump(case, nsc.model_dump(case))
        assert ended["rounds"] == ended["model_rounds"]


@pytest.mark.parametrize("what", MUTATIONS)
def test_comparer_rejects_one_changed_word(what):
    case = built("restart_cuts")
    dump = nsc.model_dump(case)
    where, index, change = _mutations(case, dump)[what]
    dump["buffers"][where][index] = change(dump["buffers"][where][index])
    with pytest.raises(nsc.StageMismatch) as err:
        nsc.compare_stage_dump(case, dump)
    assert "stage %s" % where[0] in str(err.value)


def test_comparer_rejects_violations_and_wrong_ends():
    case = built("restart_cuts")
    dump = nsc.model_dump(case)
    dump["violations"] = [{"stage": "1.round", "buffer": "nadj", "side": "high", "offset": 0}]
    with pytest.raises(nsc.StageMismatch, match="guard violation"):
        nsc.compare_stage_dump(case, dump)
    dump = nsc.model_dump(case)
    dump["violations"] = [{"stage": "S", "buffer": "exc.pick", "side": "slot", "offset": 4000}]
    with pytest.raises(nsc.StageMismatch, match="exc.pick"):
        nsc.compare_stage_dump(case, dump)
    dump = nsc.model_dump(case)
    dump["inputs_changed"] = ["exc"]
    with pytest.raises(nsc.StageMismatch, match="input"):
        nsc.compare_stage_dump(case, dump)
    dump = nsc.model_dump(case)
    dump["derived"]["rounds"] += 1
    with pytest.raises(nsc.StageMismatch, match="rounds"):
        nsc.compare_stage_dump(case, dump)
    dump = nsc.model_dump(case)                      # a give-up the model does not know: the last stages are missing
    for k in [k for k in dump["buffers"] if k[0] == "mark"]:
        del dump["buffers"][k]
    with pytest.raises(nsc.StageMismatch, match="stage mark"):
        nsc.compare_stage_dump(case, dump)
    flagged = built("limit_suspects")
    dump = nsc.model_dump(flagged)
    dump["buffers"][("1.round", "state")][2] = 0
    with pytest.raises(nsc.StageMismatch, match="flag 2"):
        nsc.compare_stage_dump(flagged, dump)
    refused = built("span256_ev_M63_refused")
    dump = nsc.model_dump(refused)
    dump["refused"] = None
    with pytest.raises(nsc.StageMismatch, match="refus"):
        nsc.compare_stage_dump(refused, dump)
