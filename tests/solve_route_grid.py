"""The characterisation grid of the plain solve (csrc/api/solve_head.inc.hip, solve_tail.inc.hip): one case per route
the tail can take -- trivial, one span sorted, one span ranked (range-major and pass-major), one span ranked in the head
and sorted in the tail, mixed spans (every sweep form, both key widths), near-uniform as sequences of calls on one
Solver, and the refusals.  `outcome` runs one case on a fresh Solver with profiling on; a case is one call or a short
sequence of calls, every call through the device entry (qmcp_hip_solve_device, or _begin / _end) on a mask buffer
pre-filled with a pattern.  For every call it returns
  - the SHA-256 of the mask words and whether the guard word behind them still holds the pattern
  - every integer field of Stats (no ms_* field)
  - the span sequence of kernel_times() as [name, launches], in the order returned -- first seen first
  - for a call that raises: the exception's type, code and message, and the SHA-256 of the whole buffer afterwards
Run as a script on a GPU it records the whole grid, with the commit it ran on:

    python tests/solve_route_grid.py tests/golden/solve_route_grid.json

and refuses to write a record in which a case did not take the route it is named for (`EXPECT`: stats.path,
near_uniform_giveup, sort_passes, and spans that must or must not be there).  tests/test_gpu_solve_route_grid.py replays
the record.

Routes that need "large" calls are reached with rank_min_reads=1 and pass_major=+-1, not with large inputs; the
near-uniform instances are those of tests/test_gpu_near_uniform.py, which the route takes only at their size."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

import by_contig_grid as bcg

M = 7
MASK_PATTERN = 0x5A5A5A5A5A5A5A5A
PATH_NONE, PATH_UNIFORM, PATH_GENERAL, PATH_NEAR_UNIFORM = 0, 1, 2, 3

u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)


# ------------------------------------------------------------------------------------------ instances
def _tables(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def _grouped(s, e, ids, lengths):
    """shuffled reads with contig ids -> the plain entry's form: placed reads only, grouped by contig (stable)"""
    placed = np.flatnonzero(ids != bcg.NO_CONTIG)
    order = placed[np.argsort(ids[placed], kind="stable")]
    counts = np.bincount(ids[order], minlength=len(lengths))
    return u32(s[order]), u32(e[order]), u32(lengths), _tables(counts)


def _one_span(seed, lengths, counts, span, inside=None):
    """counts[c] reads of one span on contig c, starts uniform (or within `inside` = (lo, width) of the contig)"""
    rng = np.random.default_rng(seed)
    ss = []
    for L, k in zip(lengths, counts):
        lo, width = inside if inside else (0, L - span + 1)
        ss.append(lo + rng.integers(0, width, size=k))
    s = np.concatenate(ss)
    return u32(s), u32(s + span - 1), u32(lengths), _tables(counts)


def _mixed(seed, lengths, counts, max_span):
    """reads of spans 1 .. max_span (both present on the first contig)"""
    rng = np.random.default_rng(seed)
    ss, ee = [], []
    for L, k in zip(lengths, counts):
        span = rng.integers(1, min(max_span, L) + 1, size=k)
        if not ss:
            span[0], span[1] = max_span, 1
        s = (rng.random(k) * (L - span + 1)).astype(np.int64)
        ss.append(s); ee.append(s + span - 1)
    return u32(np.concatenate(ss)), u32(np.concatenate(ee)), u32(lengths), _tables(counts)


RANKED_GENOME = [40_000, 20_000]
STRETCHED = [200_000, 1, 120_000]  # `small` with room for cut-point windows (128 spans at least) and speculative run-ins
LONG_GENOME = [(1 << 23) + 1_000]
GIVE_WAY = {"longer_reads": 0, "too_many": 1, "too_shallow": 2}


@functools.lru_cache(maxsize=None)
def _give_way():
    """the three instances of test_gives_way_to_the_mixed_route, drawn from its one generator in its order"""
    import test_gpu_near_uniform as tnu

    rng = np.random.default_rng(11)
    out = []
    for kwargs, m, n, L in ((dict(fraction=0.01, max_clip=30, longer=5), 100, 330_000, 40_000),
                            (dict(fraction=0.2, max_clip=30), 100, 330_000, 40_000),
                            (dict(fraction=0.01, max_clip=30), 10, 250_000, 3_000_000)):
        s, e, offs = tnu._contigs(rng, [L], [n], 150, **kwargs)
        out.append((s, e, u32([L]), offs, m))
    return out


@functools.lru_cache(maxsize=None)
def _queued_unseen():
    """the two read sets of test_rounds_queued_unseen_and_a_call_that_needs_more, and a third of the same shape with so many
    clipped reads that it needs more rounds than the first two settled in"""
    import test_gpu_near_uniform as tnu

    rng = np.random.default_rng(2024)
    lengths = u32([400_000])
    sa, ea, offs = tnu._contigs(rng, lengths, [1_200_000], 150, 0.001, 10)
    sb, eb, _ = tnu._contigs(rng, lengths, [1_200_000], 150, 0.05, 60)
    sc, ec, _ = tnu._contigs(rng, lengths, [1_200_000], 150, 0.08, 100)
    return dict(a=(sa, ea, lengths, offs), b=(sb, eb, lengths, offs), c=(sc, ec, lengths, offs))


@functools.lru_cache(maxsize=None)
def instance(name):
    """-> (starts, ends, contig lengths, contig read offsets)"""
    z = u32([])
    if name == "none_100":
        return z, z, u32([100]), _tables([0])
    if name == "none_0":
        return z, z, u32([0]), _tables([0])
    if name in ("small1", "small"):
        sh = bcg.shape(name)
        ids = sh["ids"]
        if name == "small1":  # (without the reads on contig 1's single position: their span is 1, and the case is one span)
            ids = np.where(ids == 1, bcg.NO_CONTIG, ids)
        return _grouped(sh["s"], sh["e"], ids, sh["lengths"])
    if name in ("small1_stretched", "small_stretched"):
        # the reads of `small1` / `small` -- 1 820 and 1 140 of one or two lengths, 24 on contig 1's single position (two
        # lengths only) -- on contigs long enough for the sweeps to look for cut points
        rng = np.random.default_rng(13 if name == "small1_stretched" else 14)
        counts = [1_820, 0 if name == "small1_stretched" else 24, 1_140]
        ss, ee = [], []
        for L, k in zip(STRETCHED, counts):
            span = rng.choice([100] if name == "small1_stretched" else [100, 150], size=k) if L > 1 else np.ones(k, np.int64)
            s = rng.integers(0, L - span + 1)
            ss.append(s); ee.append(s + span - 1)
        return u32(np.concatenate(ss)), u32(np.concatenate(ee)), u32(STRETCHED), _tables(counts)
    if name == "balanced":
        return _one_span(21, RANKED_GENOME, [13_334, 6_666], 100)
    if name == "balanced_long":
        return _one_span(22, LONG_GENOME, [20_000], 100)
    if name == "heavy":
        return _one_span(23, RANKED_GENOME, [13_334, 6_666], 100, inside=(1_000, 100))
    if name == "past_end":
        s, e, lengths, offs = (a.copy() for a in instance("balanced"))
        e[15_000] = lengths[1]
        return s, e, lengths, offs
    if name == "to_2000":
        return _mixed(31, [12_000, 8_000], [1_800, 1_200], 2_000)
    if name == "to_5000":
        return _mixed(32, [12_000, 8_000], [1_800, 1_200], 5_000)
    if name == "to_20000":
        return _mixed(33, [60_000, 40_000], [1_800, 1_200], 20_000)
    if name == "wide5":
        import test_gpu_sort_passes as tsp

        lengths, live = tsp.WIDE[5]
        return _grouped(*tsp.island_reads(905, lengths, 20_000, live))
    if name == "too_long":
        return u32([0, 5]), u32([(1 << 24) - 1, 104]), u32([(1 << 24) + 1_000]), _tables([2])
    if name in ("near", "near_other_span"):
        import test_gpu_near_uniform as tnu

        # the smallest instance of test_near_uniform_equals_the_oracle (clips down to one base), with its seed; M = 60
        rng = np.random.default_rng(400_000 % 9973 + 100)
        s, e, offs = tnu._contigs(rng, [50_000], [400_000], 100, 0.01, 99)
        if name == "near_other_span":
            s, e, offs = tnu._contigs(rng, [50_000], [400_000], 120, 0.0, 1)
        return s, e, u32([50_000]), offs
    if name in GIVE_WAY:
        return _give_way()[GIVE_WAY[name]][:4]
    return _queued_unseen()[name[-1]]


# ------------------------------------------------------------------------------------------ cases
# name -> (options, calls); a call is (instance, M, form) with form "device" (blocking) or "begin_end"
def _one(inst, m=M, form="device", **options):
    return options, [(inst, m, form)]


RANKED_RM = dict(rank_min_reads=1, pass_major=-1)
RANKED_PM = dict(rank_min_reads=1, pass_major=1)
NEAR_CALLS = [("near", 60, "device")] * 3 + [("near_other_span", 60, "device")]
CASES = {
    "trivial/no_reads": _one("none_100"),
    "trivial/length_0": _one("none_0"),
    "sorted/small1": _one("small1"),
    "sorted/stretched/cuts": _one("small1_stretched", cut_points=1),
    "sorted/stretched/cuts_spec": _one("small1_stretched", cut_points=1, speculation=1),
    "ranked_rm/balanced": _one("balanced", **RANKED_RM),
    "ranked_rm/two_levels": _one("balanced_long", **RANKED_RM),
    "ranked_pm/balanced": _one("balanced", **RANKED_PM),
    # (whole contigs, cut_points=-1: the ranking reads the event sweep's own output only where no stretch table is in the way)
    "ranked_pm/ev": _one("balanced", sweep="ev", cut_points=-1, **RANKED_PM),
    "ranked_pm/ev_keep_expand": _one("balanced", sweep="ev", cut_points=-1, keep_expand=1, **RANKED_PM),
    "ranked_pm/gen": _one("balanced", sweep="gen", **RANKED_PM),
    "ranked_then_sorted/rm_heavy": _one("heavy", **RANKED_RM),
    "ranked_then_sorted/pm_heavy": _one("heavy", **RANKED_PM),
    "ranked_then_sorted/rm_forced": _one("balanced", force_sort_route=1, **RANKED_RM),
    "ranked_then_sorted/pm_forced": _one("balanced", force_sort_route=1, **RANKED_PM),
    "refused/rm_past_end": _one("past_end", **RANKED_RM),
    "refused/pm_past_end": _one("past_end", **RANKED_PM),
    "refused/span_2_24": _one("too_long"),
    "mixed/small": _one("small"),
    "mixed/small/lds": _one("small", mixed_sweep_in_lds=1),
    "mixed/stretched/cuts": _one("small_stretched", cut_points=1),
    "mixed/stretched/cuts_spec": _one("small_stretched", cut_points=1, speculation=1),
    "mixed/to_2000": _one("to_2000"),
    "mixed/to_5000": _one("to_5000"),
    "mixed/to_20000": _one("to_20000"),
    "mixed/wide5": _one("wide5", 4),
    "near_uniform/pm": (dict(pass_major=1), NEAR_CALLS),
    "near_uniform/rm": (dict(pass_major=-1), NEAR_CALLS),
    "near_uniform/gives_way/longer_reads": _one("longer_reads", 100),
    "near_uniform/gives_way/too_many": _one("too_many", 100),
    "near_uniform/gives_way/too_shallow": _one("too_shallow", 10),
    "near_uniform/queued_unseen": ({}, [("queued_" + x, 40, "device") for x in "aaabbba"]),
    # (the third call's rounds are queued unseen, as many as the first two needed; it needs more: solved again when collected)
    "near_uniform/needs_more": ({}, [("queued_" + x, 40, "device") for x in "aac"]),
    "begin_end/ranked_rm": _one("balanced", form="begin_end", **RANKED_RM),
    "begin_end/ranked_pm": _one("balanced", form="begin_end", **RANKED_PM),
    "begin_end/near_uniform/pm": (dict(pass_major=1), NEAR_CALLS[:2] + [("near", 60, "begin_end")]),
    "begin_end/near_uniform/rm": (dict(pass_major=-1), NEAR_CALLS[:2] + [("near", 60, "begin_end")]),
}
# a begin / end case and the blocking case whose record it must equal (all of it, or the given calls)
SAME_AS_BLOCKING = {
    "begin_end/ranked_rm": ("ranked_rm/balanced", slice(None)),
    "begin_end/ranked_pm": ("ranked_pm/balanced", slice(None)),
    "begin_end/near_uniform/pm": ("near_uniform/pm", slice(0, 3)),
    "begin_end/near_uniform/rm": ("near_uniform/rm", slice(0, 3)),
}

# What makes a call the route its case is named for, per call: stats fields, spans that must be there ("has", a name or
# (name, launches)) and spans that must not ("lacks").  An "error" call must raise with that code.
SPEC_TIER_2 = "second tier, where the first disagreed"
SORTED = dict(path=PATH_UNIFORM, has=["k_radix_hist_rec", "k_bucket_heads", "k_mark"],
              lacks=["k_range_partition", "k_pm_prepare_sort", "k_rank_mark", "k_pm_walk"])
RM = dict(path=PATH_UNIFORM, sort_passes=1, has=["k_range_partition", "k_rank_mark"],
          lacks=["k_mark", "k_radix_hist_rec", "k_pm_prepare_sort"])
PM = dict(path=PATH_UNIFORM, sort_passes=1, has=["k_pm_prepare_sort", "k_pm_walk"],
          lacks=["k_mark", "k_radix_hist_rec", "k_range_partition", "k_rank_mark"])
VIA_SORT = dict(path=PATH_UNIFORM, has=["k_gstart", "k_radix_hist_rec", "k_mark"],
                lacks=["k_bucket_heads", "k_rank_mark", "k_pm_walk"])
MIXED = dict(path=PATH_GENERAL, has=["k_general_keys", "k_radix_hist_rec", "k_bucket_heads", "k_mark"], lacks=["k_gstart"])


def _with(base, has=(), lacks=(), **fields):
    out = dict(base, **fields)
    out["has"] = list(base.get("has", [])) + list(has)
    out["lacks"] = list(base.get("lacks", [])) + list(lacks)
    return out


def _near(head, launches):
    return dict(path=PATH_NEAR_UNIFORM, near_uniform_giveup=0, has=[(head, launches), "k_nu_mark_selected"], lacks=["k_mark"])


def _near_calls(head, rank):
    other = dict(path=PATH_UNIFORM, sort_passes=1, has=[(head, 2), rank], lacks=["k_mark", "k_nu_mark_selected"])
    return [_near(head, 2), _near(head, 1), _near(head, 1), other]


EXPECT = {
    "trivial/no_reads": [dict(path=PATH_NONE, no_spans=True)],
    "trivial/length_0": [dict(path=PATH_NONE, no_spans=True)],
    "sorted/small1": [SORTED],
    "sorted/stretched/cuts": [_with(SORTED, has=["k_find_cuts"], lacks=[SPEC_TIER_2])],
    "sorted/stretched/cuts_spec": [_with(SORTED, has=["k_find_cuts", SPEC_TIER_2])],
    "ranked_rm/balanced": [RM],
    "ranked_rm/two_levels": [dict(RM, has=["k_range_partition(level 1)", "k_rank_mark"], lacks=RM["lacks"] + ["k_range_partition"])],
    "ranked_pm/balanced": [PM],
    "ranked_pm/ev": [_with(PM, has=["k_sweep_uniform_ev"], lacks=["k_sweep_expand"])],
    "ranked_pm/ev_keep_expand": [_with(PM, has=["k_sweep_uniform_ev", "k_sweep_expand"])],
    "ranked_pm/gen": [_with(PM, has=["k_sweep_uniform_gen"])],
    "ranked_then_sorted/rm_heavy": [_with(VIA_SORT, has=["k_range_partition"])],
    "ranked_then_sorted/pm_heavy": [_with(VIA_SORT, has=["k_pm_prepare_sort"])],
    "ranked_then_sorted/rm_forced": [_with(VIA_SORT, has=["k_range_partition"])],
    "ranked_then_sorted/pm_forced": [_with(VIA_SORT, has=["k_pm_prepare_sort"])],
    "refused/rm_past_end": [dict(error=-2)],
    "refused/pm_past_end": [dict(error=-2)],
    "refused/span_2_24": [dict(error=-3)],
    "mixed/small": [_with(MIXED, has=["k_sweep_general_reg"])],
    "mixed/small/lds": [_with(MIXED, has=["k_sweep_general_cached"], lacks=["k_sweep_general_reg"])],
    "mixed/stretched/cuts": [_with(MIXED, has=["k_find_cuts", "k_sweep_general_reg"], lacks=[SPEC_TIER_2])],
    "mixed/stretched/cuts_spec": [_with(MIXED, has=["k_find_cuts", "k_sweep_general_reg", SPEC_TIER_2])],
    "mixed/to_2000": [_with(MIXED, has=["k_sweep_general_cached"], lacks=["k_sweep_general"])],
    "mixed/to_5000": [_with(MIXED, has=["k_sweep_general"], lacks=["k_sweep_general_cached", "k_group_heads"])],
    "mixed/to_20000": [_with(MIXED, has=["k_sweep_general"], lacks=["k_sweep_general_cached", "k_group_heads"])],
    "mixed/wide5": [dict(path=PATH_GENERAL, sort_passes=5, has=[("k_radix_hist", 5), "k_mark"], lacks=["k_radix_hist_rec"])],
    "near_uniform/pm": _near_calls("k_pm_prepare_sort", "k_pm_walk"),
    "near_uniform/rm": _near_calls("k_prepare", "k_rank_mark"),
    "near_uniform/gives_way/longer_reads": [dict(path=PATH_GENERAL, near_uniform_giveup=2, has=["k_mark"])],
    "near_uniform/gives_way/too_many": [dict(path=PATH_GENERAL, near_uniform_giveup=3, has=["k_mark"])],
    "near_uniform/gives_way/too_shallow": [dict(path=PATH_GENERAL, near_uniform_giveup=1, has=["k_mark"])],
    "near_uniform/queued_unseen": [dict(path=PATH_NEAR_UNIFORM, near_uniform_giveup=0, has=["k_nu_mark_selected"])] * 7,
    "near_uniform/needs_more": [_near("k_prepare", 2), _near("k_prepare", 1), dict(has=[("k_prepare", 2)])],
    "begin_end/ranked_rm": [RM],
    "begin_end/ranked_pm": [PM],
    "begin_end/near_uniform/pm": _near_calls("k_pm_prepare_sort", "k_pm_walk")[:3],
    "begin_end/near_uniform/rm": _near_calls("k_prepare", "k_rank_mark")[:3],
}


def route_misses(name, calls):
    """why the recorded calls of a case are not the route it is named for ([] if they are)"""
    out = []
    for i, (got, want) in enumerate(zip(calls, EXPECT[name])):
        where = f"{name}[{i}]"
        if "error" in want:
            if got.get("code") != want["error"]:
                out.append(f"{where}: expected an error with code {want['error']}, got {got}")
            continue
        if "error" in got:
            out.append(f"{where}: raised {got['message']}")
            continue
        spans = dict(map(tuple, got["spans"]))
        for field in ("path", "near_uniform_giveup", "sort_passes"):
            if field in want and got["stats"][field] != want[field]:
                out.append(f"{where}: stats.{field} is {got['stats'][field]}, expected {want[field]}")
        if want.get("no_spans") and spans:
            out.append(f"{where}: spans {sorted(spans)} on a trivial call")
        for h in want.get("has", []):
            h_name, launches = h if isinstance(h, tuple) else (h, None)
            if h_name not in spans or (launches is not None and spans[h_name] != launches):
                out.append(f"{where}: span {h_name!r} x {launches or '>= 1'} expected, spans are {got['spans']}")
        for l_name in want.get("lacks", []):
            if l_name in spans:
                out.append(f"{where}: span {l_name!r} must not be there, spans are {got['spans']}")
    if len(calls) != len(EXPECT[name]):
        out.append(f"{name}: {len(calls)} calls recorded, {len(EXPECT[name])} expected")
    return out


# ------------------------------------------------------------------------------------------ one case
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def outcome(pkg, name):
    """run one case on a Solver of its own -> the list of its calls' outcomes as JSON-ready data"""
    import torch

    options, calls = CASES[name]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    with pkg.Solver(0) as solver:
        solver.set_options(**options)  # (once: setting options makes a context forget what it learnt from earlier calls)
        for inst, m, form in calls:
            s, e, lengths, offs = instance(inst)
            n = int(s.size)
            words = pkg.mask_words(n)
            d_s, d_e = dev(s), dev(e)
            out = torch.full((words + 1,), MASK_PATTERN, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            solver.set_profiling(True)  # (resets the spans: one call's worth)
            try:
                if form == "device":
                    st = solver.solve_device(d_s.data_ptr(), d_e.data_ptr(), n, lengths, m, out.data_ptr(),
                                             contig_read_offsets=offs, stream=stream)
                else:
                    solver.solve_device_begin(d_s.data_ptr(), d_e.data_ptr(), n, lengths, m, out.data_ptr(),
                                              contig_read_offsets=offs, stream=stream)
                    st = solver.solve_end()
                torch.cuda.synchronize()
                after = out.cpu().numpy().view(np.uint64)
                result = dict(mask=_sha(after[:words]), guard_intact=bool(after[words] == MASK_PATTERN),
                              stats=bcg._ints(st))
            except pkg.QmcpError as err:
                torch.cuda.synchronize()
                result = dict(error=type(err).__name__, code=err.code, message=str(err), buffer=_sha(out.cpu().numpy()))
            result["spans"] = [[k, launches] for k, (launches, _) in solver.kernel_times().items()]
            results.append(result)
    return results


def main(argv):
    import importlib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    pkg = importlib.import_module("genome-downsampler_amd")
    commit = argv[2] if len(argv) > 2 else subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True,
                                                           text=True).stdout.strip()
    record, misses = {}, []
    for name in CASES:
        record[name] = outcome(pkg, name)
        misses += route_misses(name, record[name])
        print(name, [r.get("error", "ran") for r in record[name]], flush=True)
    for name, (blocking, part) in SAME_AS_BLOCKING.items():
        if record[name] != record[blocking][part]:
            misses.append(f"{name}: differs from {blocking}")
    if misses:
        print("not recorded -- cases that missed their route:", *misses, sep="\n  ")
        if len(argv) > 3 and argv[3] == "--dump":  # (what the cases did, for adjusting them: not a record)
            json.dump(record, open(argv[1] + ".rejected", "w"), indent=0, sort_keys=True)
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(argv[1])), exist_ok=True)
    with open(argv[1], "w") as f:
        json.dump(dict(commit=commit, cases=record), f, indent=0, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
