"""The characterisation grid of the by-contig family: by-contig, ladder, stratified, profile, ceiling, budget, pairs,
templates, templates under caps and replicates, each through its host and its device entry, plus one case each of the
entries that call the plain by-contig driver (targets, dedup, quality by contig, filter_solve_by_contig).  `outcome`
runs one case on a fresh Solver with profiling on and returns what it did:
  - a call that returns: the SHA-256 of every output array and every integer field of every stats struct it fills
  - a call that raises: the exception's type, code and message, and for a device entry the SHA-256 of the caller's
    pre-filled output buffer afterwards (and whether it still holds the pattern)
  - the span sequence: (span name, launches) of kernel_times(), in the order returned -- first seen first -- which
    pins the order of the launches
Every ms_* value is left out.  Run as a script on a GPU it records the whole grid:

    python tests/by_contig_grid.py tests/golden/by_contig_grid.json

tests/test_gpu_by_contig_grid.py replays the record.

Shapes: `small` (three contigs of 4 000, 1 and 2 500 positions, about 3 000 shuffled reads of two lengths at about eight
times the cap, a few unplaced, contig 1's reads on its single position), `small1` (the same with one read length),
`zero` (no read), three refused variants of `small`, and two shapes of more than one position batch, which cost seconds
and have a test function of their own: `two_batch` (the island instance of tests/test_gpu_pairs.py and
tests/test_gpu_replicates.py) and `edge` (an empty contig, the batch with the most reads second).
A single contig above one call's read limit (2^30 reads) cannot be expressed without allocating its columns (12 GiB)
and is left out."""
import contextlib
import functools
import hashlib
import json
import os
import sys

import numpy as np

import replicates_model as rm

NO_CONTIG = 0xFFFFFFFF
NO_STRATUM = 0xFFFFFFFF
M = 7
LADDER = [7, 4, 2]
STAGES = [2, 4, 7]
REPLICATES = [7, 5, 3]
STRATA_CAPS = [5, 0, 3]
MASK_PATTERN = 0x5A5A5A5A5A5A5A5A
BYTE_PATTERN = 0xA5
TWO_BATCH_LENGTHS = [1_200_000_000, 1_150_000_123, 5_000]
EDGE_LENGTHS = [1_200_000_000, 9, 1_150_000_123, 5_000]
ENTRIES = ("by_contig", "ladder", "stratified", "profile", "ceiling", "budget", "pairs", "templates",
           "templates_profile", "replicates")

u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)


# ------------------------------------------------------------------------------------------ shapes
def _extras(rng, n):
    """a stratum (0 .. 2, a few without), a template (pairs, a triple, singles) and a quality for every read"""
    assert n % 2 == 0 and n >= 8
    strata = rng.integers(0, 3, size=n).astype(np.int64)
    strata[rng.choice(n, size=5, replace=False)] = NO_STRATUM
    tids = np.arange(n) // 2
    top = int(tids[n - 7])
    tids[n - 6:] = [top + 1, top + 1, top + 1, top + 2, top + 3, top + 3]
    return dict(strata=u32(strata), tids=u32(tids), n_templates=top + 4, q=u32(rng.integers(0, 41, size=n)))


def _finish(rng, s, e, ids, lengths, big):
    perm = rng.permutation(s.size)
    return dict(s=u32(s[perm]), e=u32(e[perm]), ids=u32(ids[perm]), lengths=u32(lengths), big=big, **_extras(rng, s.size))


def _small(seed, read_lengths):
    rng = np.random.default_rng(seed)
    lengths = [4000, 1, 2500]
    ss, ee, ii = [], [], []
    for c, count in ((0, 1820), (2, 1140)):
        span = rng.choice(read_lengths, size=count)
        start = rng.integers(0, lengths[c] - span + 1)
        ss.append(start); ee.append(start + span - 1); ii.append(np.full(count, c))
    ss.append(np.zeros(24, np.int64)); ee.append(np.zeros(24, np.int64)); ii.append(np.full(24, 1))
    ss.append(rng.integers(0, 100, size=16)); ee.append(rng.integers(100, 200, size=16)); ii.append(np.full(16, NO_CONTIG))
    return _finish(rng, *(np.concatenate(x) for x in (ss, ee, ii)), lengths, False)


def _refused(what):
    sh = dict(shape("small"))
    s, e, ids = sh["s"].copy(), sh["e"].copy(), sh["ids"].copy()
    i = int(np.flatnonzero(ids == 2)[3])
    if what == "bad_id":
        ids[i] = 3
    elif what == "start_gt_end":
        s[i] = e[i] + 1
    else:
        e[i] = sh["lengths"][2]
    sh.update(s=s, e=e, ids=ids)
    return sh


def _edge():
    """contig 0 and the empty contig 1 are the first position batch, contigs 2 and 3 the second, which has the most reads"""
    rng = np.random.default_rng(57)
    ss, ee, ii = [], [], []
    for c, count, lo, width in ((0, 120, 1000, 400), (2, 600, EDGE_LENGTHS[2] - 700, 700), (3, 900, 0, 5000)):
        span = rng.choice([100, 150], size=count)
        start = lo + rng.integers(0, width - span + 1)
        ss.append(start); ee.append(start + span - 1); ii.append(np.full(count, c))
    ss.append(rng.integers(0, 100, size=10)); ee.append(rng.integers(100, 200, size=10)); ii.append(np.full(10, NO_CONTIG))
    return _finish(rng, *(np.concatenate(x) for x in (ss, ee, ii)), EDGE_LENGTHS, True)


def _two_batch():
    s, e, ids, lengths = rm.island_pairs(83, TWO_BATCH_LENGTHS, 300, per_island=40)
    return dict(s=s, e=e, ids=ids, lengths=lengths, big=True, **_extras(np.random.default_rng(84), s.size))


@functools.lru_cache(maxsize=None)
def shape(name):
    if name == "small":
        return _small(11, [100, 150])
    if name == "small1":
        return _small(12, [100])
    if name == "zero":
        z = u32([])
        return dict(s=z, e=z, ids=z, lengths=u32([4000, 1, 2500]), strata=z, tids=z, n_templates=0, q=z, big=False)
    if name == "edge":
        return _edge()
    if name == "two_batch":
        return _two_batch()
    return _refused(name)


def regions(lengths, contigs):
    """two regions (caps 2 and 1) at the two ends of every contig in `contigs` -> (offsets, starts, ends, caps)"""
    offs, r0, r1, caps = [0], [], [], []
    for c, L in enumerate(int(x) for x in lengths):
        if c in contigs and L > 1200:
            r0 += [0, L - 600]; r1 += [499, L - 1]; caps += [2, 1]
        offs.append(len(r0))
    return u32(offs), u32(r0), u32(r1), u32(caps)


def paired_on_one_contig(sh):
    """the shape with every odd read moved onto its mate's contig, so that pairs can pass the amplicon FILTER"""
    s, e, ids = (sh[k].astype(np.int64) for k in ("s", "e", "ids"))
    L = sh["lengths"].astype(np.int64)
    ids[1::2] = ids[0::2]
    placed = ids != NO_CONTIG
    span = np.where(placed, np.minimum(e - s + 1, L[np.where(placed, ids, 0)]), e - s + 1)
    room = np.where(placed, L[np.where(placed, ids, 0)] - span + 1, 1 << 30)
    s = s % room
    return u32(s), u32(s + span - 1), u32(ids)


# ------------------------------------------------------------------------------------------ cases
# parameter sets per entry: the first is the one every shape runs, the others run on `small` only
PARAMS = {
    "by_contig": [("M7", {})],
    "ladder": [("3_levels", dict(coverages=LADDER)), ("1_level", dict(coverages=[M]))],
    "stratified": [("caps_5_0_3", {})],
    "profile": [("regions", dict(default_cap=3, contigs=(0, 2))), ("no_region", dict(default_cap=M, contigs=())),
                ("default_cap_0", dict(default_cap=0, contigs=(0, 2)))],
    "ceiling": [("regions", dict(default_cap=3, contigs=(0, 2), flags=0)),
                ("whole_pairs", dict(default_cap=3, contigs=(0, 2), flags=1)),
                ("nowhere_below", dict(default_cap=100000, contigs=(), flags=0))],
    "budget": [("reads", dict(flags=0)), ("whole_pairs", dict(flags=1))],
    "pairs": [("3_stages", dict(stages=STAGES)), ("1_stage", dict(stages=[M]))],
    "templates": [("3_stages", dict(stages=STAGES)), ("1_stage", dict(stages=[M]))],
    "templates_profile": [("regions_in_one_contig", dict(default_cap=M, contigs=(0,), stages=STAGES)),
                          ("no_region", dict(default_cap=M, contigs=(), stages=STAGES))],
    "replicates": [("K3", dict(coverages=REPLICATES, flags=0)), ("K1", dict(coverages=[M], flags=0)),
                   ("K3_whole_pairs", dict(coverages=REPLICATES, flags=1)),
                   ("K3_shortfall", dict(coverages=REPLICATES, flags=2)),
                   ("K3_whole_pairs_shortfall", dict(coverages=REPLICATES, flags=3))],
}
PLAIN_DRIVER_USERS = ("targets", "dedup", "quality_by_contig", "filter_solve_by_contig")
REFUSALS = ("bad_id", "start_gt_end", "past_end")
REFUSED_ENTRIES = ("by_contig", "budget", "ladder", "replicates")


def _rows():
    small, big = [], []
    for entry in ENTRIES:
        for form in ("host", "device"):
            for pname, _ in PARAMS[entry]:
                small.append((entry, form, "small", pname))
            for shp in ("small1", "zero"):
                small.append((entry, form, shp, PARAMS[entry][0][0]))
            for shp in ("two_batch", "edge"):
                for pname, _ in PARAMS[entry][:2 if entry == "budget" else 1]:
                    big.append((entry, form, shp, pname))
    for entry in REFUSED_ENTRIES:
        for form in ("host", "device"):
            small += [(entry, form, shp, PARAMS[entry][0][0]) for shp in REFUSALS]
    small += [(entry, "host", "small", "M7") for entry in PLAIN_DRIVER_USERS]
    return small, big


SMALL_CASES, BATCH_CASES = _rows()


def key_of(case):
    return "/".join(case)


# ------------------------------------------------------------------------------------------ one case
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _ints(st):
    """every integer field of a ctypes stats struct (arrays as lists); ms_* and other floats are left out"""
    out = {}
    for name, _ in st._fields_:
        v = getattr(st, name)
        if name.startswith("ms_") or isinstance(v, float):
            continue
        out[name] = [int(x) for x in v] if hasattr(v, "__len__") else int(v)
    return out


def _call(pkg, solver, case, held):
    """run the case's call -> (arrays, stats structs); a device entry's output buffer is left in held["buffer"]"""
    entry, form, shp, pname = case
    sh = shape(shp)
    p = dict(PARAMS[entry]).get(pname, {}) if entry in PARAMS else {}
    s, e, ids, L = sh["s"], sh["e"], sh["ids"], sh["lengths"]
    n = int(s.size)
    placed = int(np.count_nonzero(ids != NO_CONTIG))
    regs = regions(L, p["contigs"]) if "contigs" in p else None
    if form == "device":
        import torch

        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")
        cols = [dev(x) for x in (s, e, ids)]
        ptr = [c.data_ptr() for c in cols]
        stream = torch.cuda.current_stream().cuda_stream
        if entry in ("ladder", "replicates"):
            out = torch.full((n + 1,), BYTE_PATTERN, dtype=torch.uint8, device="cuda:0")
        else:
            out = torch.full((pkg.mask_words(n) + 1,), MASK_PATTERN, dtype=torch.int64, device="cuda:0")
        held["buffer"] = out
        torch.cuda.synchronize()
    arrays = {}
    if entry == "by_contig":
        if form == "host":
            arrays["mask"] = solver.solve_by_contig(s, e, ids, L, M)
        else:
            solver.solve_by_contig_device(*ptr, n, L, M, out.data_ptr(), stream=stream)
        stats = [solver.last_stats]
    elif entry == "ladder":
        if form == "host":
            arrays["levels"] = solver.solve_ladder(s, e, ids, L, p["coverages"])
        else:
            solver.solve_ladder_device(*ptr, n, L, p["coverages"], out.data_ptr(), stream=stream)
        stats = [solver.last_stats, solver.last_ladder_stats]
    elif entry == "stratified":
        if form == "host":
            arrays["mask"] = solver.solve_stratified(s, e, ids, sh["strata"], L, STRATA_CAPS)
        else:
            d_strata = dev(sh["strata"])
            solver.solve_stratified_device(*ptr, d_strata.data_ptr(), n, L, STRATA_CAPS, out.data_ptr(), stream=stream)
        arrays["rows"] = np.array([[r.n_reads, r.n_kept, r.bases_in, r.bases_kept] for r in solver.last_stratum_rows],
                                  dtype=np.uint64)
        stats = [solver.last_stats]
    elif entry in ("profile", "ceiling"):
        name = "solve_" + entry
        flags = p.get("flags", 0)
        if form == "host":
            arrays["mask"] = getattr(solver, name)(s, e, ids, L, p["default_cap"], *regs, flags=flags)
        else:
            getattr(solver, name + "_device")(*ptr, n, L, p["default_cap"], out.data_ptr(), *regs, flags=flags,
                                               stream=stream)
        stats = [solver.last_stats, solver.last_profile_stats if entry == "profile" else solver.last_ceiling_stats]
    elif entry == "budget":
        if form == "host":
            got = solver.solve_budget(s, e, ids, L, M, budget_reads=placed // 4, flags=p["flags"], curve=True)
            arrays["mask"] = got[0]
        else:
            got = solver.solve_budget_device(*ptr, n, L, M, out.data_ptr(), budget_reads=placed // 4, flags=p["flags"],
                                             curve=True, stream=stream)
        arrays["curve"] = got[-1]
        stats = [solver.last_stats, solver.last_budget_stats]
    elif entry == "pairs":
        if form == "host":
            arrays["mask"] = solver.solve_pairs(s, e, ids, L, M, p["stages"])[0]
        else:
            solver.solve_pairs_device(*ptr, n, L, M, out.data_ptr(), p["stages"], stream=stream)
        stats = [solver.last_stats, solver.last_pair_stats]
    elif entry == "templates":
        if form == "host":
            arrays["mask"] = solver.solve_templates(s, e, ids, sh["tids"], sh["n_templates"], L, M, p["stages"])[0]
        else:
            d_tids = dev(sh["tids"])
            solver.solve_templates_device(*ptr, d_tids.data_ptr(), n, sh["n_templates"], L, M, out.data_ptr(), p["stages"],
                                          stream=stream)
        stats = [solver.last_stats, solver.last_template_stats]
    elif entry == "templates_profile":
        if form == "host":
            arrays["mask"] = solver.solve_templates_profile(s, e, ids, sh["tids"], sh["n_templates"], L, M, p["default_cap"],
                                                            *regs, stages=p["stages"])[0]
        else:
            d_tids = dev(sh["tids"])
            solver.solve_templates_profile_device(*ptr, d_tids.data_ptr(), n, sh["n_templates"], L, M, p["default_cap"],
                                                  out.data_ptr(), *regs, stages=p["stages"], stream=stream)
        stats = [solver.last_stats, solver.last_template_stats, solver.last_template_profile_stats]
    elif entry == "replicates":
        if form == "host":
            arrays["labels"] = solver.solve_replicates(s, e, ids, L, p["coverages"], p["flags"])
        else:
            solver.solve_replicates_device(*ptr, n, L, p["coverages"], out.data_ptr(), p["flags"], stream=stream)
        stats = [solver.last_stats, solver.last_replicates_stats] + list(solver.last_replicate_solve_stats)
    elif entry == "targets":
        t_offs, t0, t1, _ = regions(L, (0, 2))
        arrays["mask"] = solver.solve_targets(s, e, ids, L, M, t_offs, t0, t1)
        stats = [solver.last_stats, solver.last_target_stats]
    elif entry == "dedup":
        arrays["mask"], arrays["dup"], _, _ = solver.solve_dedup(s, e, ids, L, M)
        stats = [solver.last_stats, solver.last_dedup_stats]
    elif entry == "quality_by_contig":
        arrays["mask"] = solver.solve_quality_by_contig(s, e, ids, sh["q"], L, M)
        stats = [solver.last_stats, solver.last_quality_stats]
    else:
        ps, pe, pids = paired_on_one_contig(sh)
        a_offs, a0, a1 = u32([0, 2, 2, 4]), u32([0, 2000, 0, 1200]), u32([2100, 3999, 1300, 2499])  # two amplicons each
        arrays["mask"], dropped = solver.filter_solve_by_contig(ps, pe, pids, L, M, a_offs, a0, a1)
        arrays["dropped"] = np.array([dropped], dtype=np.uint64)
        stats = [solver.last_stats]
    if form == "device":
        import torch

        torch.cuda.synchronize()
        arrays["device_buffer"] = out.cpu().numpy()
    return arrays, stats


def outcome(pkg, case):
    """run one case on a Solver of its own -> its outcome as JSON-ready data"""
    held = {}
    with pkg.Solver(0) as solver:
        solver.set_profiling(True)
        with (solver.options(cut_points=1) if shape(case[2])["big"] else contextlib.nullcontext()):
            try:
                arrays, stats = _call(pkg, solver, case, held)
                result = dict(arrays={k: _sha(v) for k, v in arrays.items()},
                              stats=[[type(st).__name__, _ints(st)] for st in stats])
            except pkg.QmcpError as err:
                result = dict(error=type(err).__name__, code=err.code, message=str(err))
                if "buffer" in held:
                    import torch

                    torch.cuda.synchronize()
                    after = held["buffer"].cpu().numpy()
                    pattern = BYTE_PATTERN if after.dtype == np.uint8 else MASK_PATTERN
                    result.update(buffer=_sha(after), buffer_untouched=bool((after == pattern).all()))
        result["spans"] = [[name, launches] for name, (launches, _) in solver.kernel_times().items()]
    return result


def main(argv):
    import importlib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    pkg = importlib.import_module("genome-downsampler_amd")
    record = {}
    for case in SMALL_CASES + BATCH_CASES:
        record[key_of(case)] = outcome(pkg, case)
        print(key_of(case), record[key_of(case)].get("error", "ran"), len(record[key_of(case)]["spans"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(argv[1])), exist_ok=True)
    with open(argv[1], "w") as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv)
