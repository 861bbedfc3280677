"""One context through every family of its buffers, through a regrow of all of them, and beside a second context: a
reused, regrown or neighbouring Solver returns what a fresh Solver returns for the same call, and closes cleanly.

The reference of every call is the same call on a Solver of its own (what the grids of tests/test_gpu_by_contig_grid.py
and tests/test_gpu_downsample_grid.py pin), computed once per call and shared.  Output arrays only are compared: a
reused context legitimately differs in arena_grown_mid_solve and in what it remembers about routes.  Every call is valid
and small; what a context must not do here is leak, free twice or hand out a buffer of another size."""
import functools

import numpy as np
import pytest

import by_contig_grid as grid
import workloads

pytestmark = pytest.mark.gpu

M = grid.M
READ = 150


# ------------------------------------------------------------------------------------------ outputs as arrays
def _arrays(out):
    """whatever an entry returns -> a flat list of numpy arrays (stats structs are left out)"""
    if isinstance(out, dict):
        return [a for k in sorted(out) for a in _arrays(out[k])]
    if isinstance(out, (tuple, list)):
        return [a for x in out for a in _arrays(x)]
    if isinstance(out, np.ndarray):
        return [out]
    if isinstance(out, (int, np.integer)):
        return [np.array([out], dtype=np.int64)]
    if hasattr(out, "contig_rows"):  # a DepthReport
        return [out.contig_rows, out.region_rows, out.hist_in, out.hist_kept]
    return []  # a stats struct


def _same(got, want, what):
    assert len(got) == len(want) and len(want) > 0, what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{what}: output {i} differs"


# ------------------------------------------------------------------------------------------ 1. every buffer family
@functools.lru_cache(maxsize=None)
def _plain_inputs():
    s, e, a0, a1, _ = workloads.amplicon_reads(2000, seed=5)  # 4 000 reads in pairs on 29 903 positions
    n = int(s.size)
    rng = np.random.default_rng(6)
    bits = np.flatnonzero(rng.random(n) < 0.4)
    return dict(s=s, e=e, a0=a0, a1=a1, n=n, L=29_903, ids=np.zeros(n, np.uint32), bits=bits)


def _family_calls(pkg):
    """(name, call(solver) -> outputs): the first small case of every by-contig entry, host and device, and the plain
    entries on a few thousand reads"""
    calls = []
    for entry in grid.ENTRIES:
        for form in ("host", "device"):
            case = next(c for c in grid.SMALL_CASES if c[:3] == (entry, form, "small"))
            calls.append((grid.key_of(case), lambda sv, case=case: grid._call(pkg, sv, case, {})[0]))
    p = _plain_inputs()
    s, e, a0, a1, n, L, ids = (p[k] for k in ("s", "e", "a0", "a1", "n", "L", "ids"))
    km = pkg.indices_to_mask(p["bits"], n)
    regions = dict(target_offsets=[0, 2], target_starts=[100, 20_000], target_ends=[5_000, 25_000])
    calls += [
        ("solve", lambda sv: sv.solve(s, e, L, 50)),
        ("solve64", lambda sv: sv.solve64(s.astype(np.uint64), e.astype(np.uint64), L, 50)),
        ("coverage(keep_mask)", lambda sv: sv.coverage(s, e, L, keep_mask=km)),
        ("demand", lambda sv: sv.demand(s, e, L, 50)),
        ("filter_solve", lambda sv: sv.filter_solve(s, e, L, 50, amp_starts=a0, amp_ends=a1, complete_pairs=True)),
        ("amplicon_filter", lambda sv: sv.amplicon_filter(s, e, a0, a1)),
        ("complete_pairs", lambda sv: sv.complete_pairs(km, n)),
        ("depth_report", lambda sv: sv.depth_report(s, e, ids, [L], 50, keep_mask=km, n_bins=64, **regions)),
        ("depth_track", lambda sv: sv.depth_track(s, e, ids, [L], 50, keep_mask=km, **regions)[0]),
    ]
    return calls


_FRESH = {}


def _fresh(pkg, name, call):
    """the call's outputs on a Solver of its own, computed once"""
    if name not in _FRESH:
        with pkg.Solver(0) as sv:
            _FRESH[name] = _arrays(call(sv))
    return _FRESH[name]


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_one_context_serves_every_buffer_family(pkg, order):
    calls = _family_calls(pkg)
    assert len(calls) == 2 * len(grid.ENTRIES) + 9
    if order == "reverse":
        calls = calls[::-1]
    shared = pkg.Solver(0)
    got = [(name, _arrays(call(shared))) for name, call in calls]
    shared.close()
    for (name, call), (_, out) in zip(calls, got):
        _same(out, _fresh(pkg, name, call), f"{name} on the shared context ({order})")


# ------------------------------------------------------------------------------------------ 2. regrow
SIZES = (1_000, 300_000, 1_000)  # 300 000: above the ranked route's 128 Ki reads, every buffer regrown, solve64's staging too
CONTIGS = [30_000, 20_000]


@functools.lru_cache(maxsize=None)
def _reads(n):
    """n reads of one length on two contigs, in no order -> (s, e, ids); and the same reads laid out for the plain
    solve: grouped by contig -> (s, e, read offsets)"""
    rng = np.random.default_rng(1000 + n)
    ids = (rng.random(n) < 0.4).astype(np.uint32)
    lens = np.asarray(CONTIGS, np.int64)[ids]
    s = (rng.random(n) * (lens - READ + 1)).astype(np.int64)
    e = s + READ - 1
    by = np.argsort(ids, kind="stable")
    offs = np.array([0, int(np.count_nonzero(ids == 0)), n], np.uint64)
    return (grid.u32(s), grid.u32(e), ids), (grid.u32(s[by]), grid.u32(e[by]), offs)


def _regrow_calls():
    def plain(sv, n):
        s, e, offs = _reads(n)[1]
        return sv.solve(s, e, CONTIGS, M, contig_read_offsets=offs)

    def plain64(sv, n):
        s, e, offs = _reads(n)[1]
        return sv.solve64(s.astype(np.uint64), e.astype(np.uint64), CONTIGS, M, contig_read_offsets=offs)

    return [
        ("solve", plain),
        ("solve_by_contig", lambda sv, n: sv.solve_by_contig(*_reads(n)[0], CONTIGS, M)),
        ("solve_ladder", lambda sv, n: sv.solve_ladder(*_reads(n)[0], CONTIGS, grid.LADDER)),
        ("solve_replicates", lambda sv, n: sv.solve_replicates(*_reads(n)[0], CONTIGS, grid.REPLICATES)),
        ("solve64", plain64),
    ]


@pytest.mark.parametrize("entry", [name for name, _ in _regrow_calls()])
def test_a_context_regrown_returns_what_a_fresh_one_returns(pkg, entry):
    call = dict(_regrow_calls())[entry]
    assert grid.LADDER == [7, 4, 2] and grid.REPLICATES == [7, 5, 3]
    with pkg.Solver(0) as sv:
        got = [_arrays(call(sv, n)) for n in SIZES]
    for n, out in zip(SIZES, got):
        _same(out, _fresh(pkg, f"regrow/{entry}/{n}", lambda fresh, n=n: call(fresh, n)), f"{entry} at {n} reads")
    _same(got[0], got[2], f"{entry}: the two {SIZES[0]}-read calls")


# ------------------------------------------------------------------------------------------ 3. two contexts
def test_two_contexts_do_not_share_what_one_of_them_frees(pkg):
    calls = [c for c in _family_calls(pkg) if c[0] in ("by_contig/host/small/M7", "replicates/device/small/K3", "solve",
                                                        "filter_solve", "depth_track")]
    assert len(calls) == 5
    first, second = pkg.Solver(0), pkg.Solver(0)
    for name, call in calls:  # interleaved: every call on one, then on the other
        _same(_arrays(call(first)), _fresh(pkg, name, call), f"{name} on the first of two contexts")
        _same(_arrays(call(second)), _fresh(pkg, name, call), f"{name} on the second of two contexts")
    first.close()
    for name, call in calls:
        _same(_arrays(call(second)), _fresh(pkg, name, call), f"{name} after the other context was closed")
    second.close()
    second.close()  # a second close does nothing
    pkg.Solver(0).close()  # created and closed at once, without a call
