"""qmcp_hip_solve_profile_*: a cap per region.  Every mask bit for bit against tests/profile_model.py (the canonical rule
with need(p) = min(cov(p), cap(p))) unless stated: caps == M through the capped route against solve_by_contig, random
profiles under both cut-point settings and the plain walk, stretches on shallow data, the count against solve_targets,
errors, the device entry and the file flow, and the cost of the capped route against the plain mixed-span route."""
import json
import os
import statistics
import time

import numpy as np
import pytest
import torch

import bam_py
import profile_model as pm
import target_model as tm

pytestmark = pytest.mark.gpu

NO_CONTIG = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# The capped route's time over the plain mixed-span route's on the cost test's shape (both one chain per contig).  What the
# profile adds is one pass over the positions and one load per position in the sweep.  First measurement on an MI355X
# (profiles/profile_time.json): plain 75.90 ms, profile 76.00 ms, ratio 1.0012, k_profile_need 0.067 ms of it; the five
# runs of either call spread by 1.0 % (75.32 .. 75.96 and 75.61 .. 76.40 ms).  Both calls are timed in one process on one
# device, so what the margin has to hold is that run-to-run spread on both sides of the ratio (2 %) and a box whose
# walk-to-pass balance differs by the several per cent DESIGN.md section 6 records between boxes: 1.0012 + 0.05, rounded.
COST_MARGIN = 1.05


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")


def spans_reads(rng, n, L, lo, hi):
    hi = min(hi, L)
    lo = min(lo, hi)
    span = rng.integers(lo, hi + 1, size=n, dtype=np.int64)
    start = (rng.random(n) * (L - span + 1)).astype(np.int64)
    return start.astype(np.uint32), (start + span - 1).astype(np.uint32)


def layouts(lengths, M):
    """the three cap layouts of 'every cap equals M': (default, offs, r0, r1, caps, takes the capped route)"""
    lengths = np.atleast_1d(lengths)
    offs, r0, r1 = [0], [], []
    tile_offs, t0, t1 = [0], [], []
    for L in lengths.tolist():
        edges = list(range(0, L, 97))                       # many regions, gaps between them left to the default
        for a in edges:
            r0.append(a); r1.append(min(a + 60, L - 1))
        offs.append(len(r0))
        for a in range(0, L, 64):                           # tiles: every position lies in a region
            t0.append(a); t1.append(min(a + 63, L - 1))
        tile_offs.append(len(t0))
    u = lambda x: np.array(x, np.uint32)
    yield "regions at M", M, u(offs), u(r0), u(r1), np.full(len(r0), M, np.uint32), True
    yield "default 0, tiles at M", 0, u(tile_offs), u(t0), u(t1), np.full(len(t0), M, np.uint32), True
    yield "empty table", M, np.zeros(lengths.size + 1, np.uint32), u([]), u([]), u([]), False


def check_all_caps_M(solver, s, e, ids, lengths, M):
    want = solver.solve_by_contig(s, e, ids, lengths, M)
    for name, default, offs, r0, r1, caps, capped in layouts(lengths, M):
        got = solver.solve_profile(s, e, ids, lengths, default, offs, r0, r1, caps)
        assert np.array_equal(got, want), name
        ps = solver.last_profile_stats
        assert ps.regions_in == ps.regions_used == r0.size, name
        if capped:
            assert solver.last_stats.path == 2, name                            # QMCP_PATH_GENERAL
            d, cp = pm.demand_and_capped(s, e, ids, lengths, default, offs, r0, r1, caps)
            assert (int(ps.demand), int(ps.capped_positions)) == (d, cp), name
        else:
            assert int(ps.demand) == 0 and int(ps.capped_positions) == 0, name


# ------------------------------------------------------------------------------------------ 1. caps == M
def test_one_span_through_the_capped_route(solver):
    rng = np.random.default_rng(71)
    L, n, M = 2000, 5000, 7
    s = rng.integers(0, L - 100 + 1, size=n).astype(np.uint32)
    e = s + 99                                                                   # one span: span_bits == 0
    check_all_caps_M(solver, s, e, np.zeros(n, np.uint32), np.array([L], np.uint32), M)


@pytest.mark.parametrize("max_span", [448, 449])
def test_register_form_limit_and_first_plain_case(solver, max_span):
    rng = np.random.default_rng(72 + max_span)
    lengths = np.array([1, 63, 64, 65, 1000], np.uint32)
    ss, ee, ii = [], [], []
    for c, L in enumerate(lengths.tolist()):
        n = 3 * L + 5
        s, e = spans_reads(rng, n, L, 1, max_span)
        ss.append(s); ee.append(e); ii.append(np.full(n, c, np.uint32))
    s, e, ids = np.concatenate(ss), np.concatenate(ee), np.concatenate(ii)
    s[0], e[0] = 0, max_span - 1                                                 # the longest span is there (contig 4)
    ids[0] = 4
    perm = rng.permutation(s.size)
    check_all_caps_M(solver, s[perm], e[perm], ids[perm], lengths, 5)
    assert solver.last_stats.max_span == max_span


def test_long_reads_put_the_rings_in_global_memory(solver):
    rng = np.random.default_rng(74)
    L, n = 60_000, 300
    s, e = spans_reads(rng, n, L, 17_000, 20_000)
    check_all_caps_M(solver, s, e, np.zeros(n, np.uint32), np.array([L], np.uint32), 4)


# ------------------------------------------------------------------------------------------ 2. random profiles
def random_instance(rng):
    n_contigs = int(rng.integers(1, 5))
    lengths = rng.integers(1, 701 // n_contigs + 1, size=n_contigs).astype(np.uint32)
    lengths[int(rng.integers(0, n_contigs))] = 700 // n_contigs                  # one contig long enough for 64-edges
    n = int(rng.integers(1, 401))
    ids = rng.integers(0, n_contigs, size=n).astype(np.uint32)
    max_len = int(rng.choice([3, 40, 130, 500]))
    Ls = lengths[ids].astype(np.int64)
    span = np.minimum(rng.integers(1, max_len + 1, size=n), Ls)
    s = (rng.random(n) * (Ls - span + 1)).astype(np.int64)
    e = s + span - 1
    ids[rng.random(n) < 0.05] = NO_CONTIG                                        # unplaced reads: any coordinates
    zero_run = int(span.max()) + 1 if rng.random() < 0.5 else 0                  # a cap-0 run longer than the longest read
    offs, r0, r1, caps = pm.random_regions(rng, lengths, 12, zero_run=zero_run)
    if r0.size == 0:                                                             # (the capped route needs a region)
        offs = np.concatenate([[0], np.full(n_contigs, 1)]).astype(np.uint32)
        r0, r1, caps = np.array([0], np.uint32), np.array([int(lengths[0]) - 1], np.uint32), np.array([3], np.uint32)
    if rng.random() < 0.3:
        caps[int(rng.integers(0, caps.size))] = 100_000                          # a cap far above the coverage
    default = int(rng.integers(0, 13))
    return s.astype(np.uint32), e.astype(np.uint32), ids, lengths, default, offs, r0, r1, caps


def test_random_profiles_under_every_setting(solver):
    rng = np.random.default_rng(75)
    changed_inside_a_read = 0
    for _ in range(200):
        s, e, ids, lengths, default, offs, r0, r1, caps = random_instance(rng)
        want = pm.expected_mask(s, e, ids, lengths, default, offs, r0, r1, caps)
        with_regions = [c for c in range(lengths.size) if offs[c + 1] > offs[c]]
        demand, capped = pm.demand_and_capped(s, e, ids, lengths, default, offs, r0, r1, caps)
        for fields in ({"cut_points": -1}, {"cut_points": 1}, {"mixed_sweep_in_lds": 1}):
            with solver.options(**fields):
                got = solver.solve_profile(s, e, ids, lengths, default, offs, r0, r1, caps)
            assert np.array_equal(got, want), (fields, lengths.tolist())
            ps = solver.last_profile_stats
            assert (int(ps.demand), int(ps.capped_positions)) == (demand, capped), fields
            assert solver.last_stats.spec_boundaries == 0
        cap = pm.cap_arrays(lengths, default, offs, r0, r1, caps)
        placed = np.flatnonzero(ids != NO_CONTIG)
        changed_inside_a_read += any(np.unique(cap[ids[i]][s[i]:e[i] + 1]).size > 1 for i in placed.tolist())
        assert with_regions
    assert changed_inside_a_read > 100


# ------------------------------------------------------------------------------------------ 3. stretches
def test_shallow_data_is_swept_in_stretches(solver):
    rng = np.random.default_rng(76)
    L, n = 40_000, 3000
    s, e = spans_reads(rng, n, L, 50, 150)
    ids, lengths = np.zeros(n, np.uint32), np.array([L], np.uint32)
    edges = np.arange(0, L, 500)
    offs = np.array([0, edges.size], np.uint32)
    r0, r1 = edges.astype(np.uint32), np.minimum(edges + 499, L - 1).astype(np.uint32)
    caps = rng.integers(1, 5, size=edges.size).astype(np.uint32)
    with solver.options(cut_points=1):
        got = solver.solve_profile(s, e, ids, lengths, 2, offs, r0, r1, caps)
    st = solver.last_stats
    assert st.sweep_stretches > 1 and st.spec_boundaries == 0, st.as_dict()
    assert np.array_equal(got, pm.expected_mask(s, e, ids, lengths, 2, offs, r0, r1, caps))


# ------------------------------------------------------------------------------------------ 4. against targets
def test_default_zero_with_regions_at_M_keeps_as_many_as_solve_targets(solver, oracle):
    rng = np.random.default_rng(77)
    lengths = np.array([3000, 1200, 500], np.uint32)
    n, M = 4000, 4
    ids = rng.integers(0, 3, size=n).astype(np.uint32)
    Ls = lengths[ids].astype(np.int64)
    span = rng.integers(20, 200, size=n)
    s = (rng.random(n) * (Ls - span + 1)).astype(np.int64)
    e, s = (s + span - 1).astype(np.uint32), s.astype(np.uint32)
    offs, r0, r1, caps = pm.random_regions(rng, lengths, 1, max_regions=6)
    caps[:] = M
    got = solver.solve_profile(s, e, ids, lengths, 0, offs, r0, r1, caps)
    n_profile = int(solver.last_stats.n_kept)
    solver.solve_targets(s, e, ids, lengths, M, offs, r0, r1)
    assert n_profile == int(solver.last_stats.n_kept) == int(pm.unpack(got, n).sum()) > 0
    kept = pm.unpack(got, n)
    for c, tset in enumerate(tm.target_sets(lengths, offs, r0, r1)):
        sel = ids == c
        cov_all = pm.coverage(s[sel].astype(np.int64), e[sel].astype(np.int64), int(lengths[c]))
        cov_kept = pm.coverage(s[sel & kept].astype(np.int64), e[sel & kept].astype(np.int64), int(lengths[c]))
        assert np.all(cov_kept[tset] >= np.minimum(cov_all[tset], M)), c


# ------------------------------------------------------------------------------------------ 5. errors
def test_errors_leave_the_mask_alone(pkg, solver):
    import ctypes as C
    s, e = np.array([0, 5], np.uint32), np.array([9, 20], np.uint32)
    ids, lengths = np.zeros(2, np.uint32), np.array([100], np.uint32)
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    cases = [([0, 2], [10, 20], [20, 30], [1, 1], 3, pkg.QMCP_EINVAL),           # overlap
             ([0, 1], [9], [3], [1], 3, pkg.QMCP_EINVAL),                         # start > end
             ([1, 1], [9], [9], [1], 3, pkg.QMCP_EINVAL),                         # offsets do not start at 0
             ([0, 1], [1], [2], [1 << 31], 3, pkg.QMCP_ERANGE),                   # a cap of 2^31
             ([0, 1], [1], [2], [1], 1 << 31, pkg.QMCP_ERANGE)]                   # default_cap of 2^31
    hip = C.CDLL(pkg.HIP_LIB_PATH)
    hip.qmcp_hip_solve_profile_host.argtypes = pkg._hip.qmcp_hip_solve_profile_host.argtypes
    for offs, r0, r1, caps, default, code in cases:
        mask = np.full(1, 0xDEADBEEF, np.uint64)
        u = [np.array(x, np.uint32) for x in (offs, r0, r1, caps)]
        rc = hip.qmcp_hip_solve_profile_host(solver._ctx, p32(s), p32(e), p32(ids), 2, p32(lengths), 1, p32(u[0]),
                                             p32(u[1]), p32(u[2]), p32(u[3]), default, 0,
                                             mask.ctypes.data_as(C.POINTER(C.c_uint64)), None, None)
        assert rc == code and mask[0] == 0xDEADBEEF, (offs, rc)
    with pytest.raises(pkg.QmcpError) as ex:                                     # unknown flag bits
        solver.solve_profile(s, e, ids, lengths, 3, [0, 1], [1], [2], [1], flags=4)
    assert ex.value.code == pkg.QMCP_EINVAL
    # a bad read: found on the device, the device mask all zero by then
    bad_e = np.array([9, 100], np.uint32)
    d_mask = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    ds, de, di = _dev(s), _dev(bad_e), _dev(ids)
    torch.cuda.synchronize()
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_profile_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), 2, lengths, 3, d_mask.data_ptr(),
                                    [0, 1], [1], [2], [1])
    torch.cuda.synchronize()
    assert ex.value.code == pkg.QMCP_EREAD and int(d_mask.cpu()[0]) == 0


# ------------------------------------------------------------------------------------------ 6. device entry, file flow
def test_device_entry_equals_host_entry(pkg, solver):
    rng = np.random.default_rng(78)
    s, e, ids, lengths, default, offs, r0, r1, caps = random_instance(rng)
    want = solver.solve_profile(s, e, ids, lengths, default, offs, r0, r1, caps)
    host_stats = solver.last_profile_stats.as_dict()
    n = s.size
    ds, de, di = _dev(s), _dev(e), _dev(ids)
    d_mask = torch.full((max(pkg.mask_words(n), 1),), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ps = solver.solve_profile_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, default, d_mask.data_ptr(),
                                     offs, r0, r1, caps)
    torch.cuda.synchronize()
    assert np.array_equal(d_mask.cpu().numpy().view(np.uint64)[:pkg.mask_words(n)], want)
    dev_stats = ps.as_dict()
    for k in ("positions_in_regions", "capped_positions", "demand", "regions_in", "regions_used"):
        assert dev_stats[k] == host_stats[k]


def test_downsample_bam_with_a_profile_writes_the_reads_of_the_mask(pkg, solver, oracle, tmp_path):
    path = os.path.join(GOLDEN, "tiny_other_writer.bam")
    caps_path = os.path.join(GOLDEN, "tiny_profile_caps.bedgraph")
    M = 2
    cols = pkg.read_bam(path, per_reference=True)
    n = cols["starts"].size
    offs, r0, r1, caps = pkg.profile_from_bedgraph(caps_path, pkg.reference_names(path))
    want = pm.expected_mask(cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"], M, offs, r0, r1, caps)
    got = solver.solve_profile(cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"], M, offs, r0, r1, caps)
    assert np.array_equal(got, want)
    kept = pm.unpack(want, n)
    assert 0 < kept.sum() < (cols["contig_ids"] != NO_CONTIG).sum()               # the caps bite
    mask = oracle.find_pairs(want, n)
    kept_ids = np.sort(np.asarray(cols["bam_ids"], np.int64)[pkg.mask_to_indices(mask, n).astype(np.int64)])
    assert np.unique(kept_ids).size == kept_ids.size      # (the file's three-segment template is kept through one pair only)
    out = tmp_path / "out.bam"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, profile=caps_path)
    header, parsed, _ = bam_py.parse(path)
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == kept_ids.size == len(orecs)
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]


# ------------------------------------------------------------------------------------------ 7. cost
def test_capped_route_costs_little_more_than_the_plain_mixed_route(pkg, solver):
    """2^22 reads of two spans (100 and 150) on 8 contigs, shuffled; near_uniform = -1, speculation = -1 and
    cut_points = -1, so the plain by-contig solve takes the sort-based mixed route as one chain per contig, as the profile
    call (every cap M, through the capped route) does.  Wall time of the whole device call, medians of 5 after a warm-up.
    QMCP_PROFILE_TIME_OUT=<file> keeps the figures."""
    n_contigs, L, M = 8, 500_000, 60
    n = 1 << 22
    rng = np.random.default_rng(79)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), n // n_contigs)
    span = np.where(rng.random(n) < 0.5, 100, 150).astype(np.int64)
    s = (rng.random(n) * (L - span + 1)).astype(np.int64)
    e, s = (s + span - 1).astype(np.uint32), s.astype(np.uint32)
    perm = rng.permutation(n)
    s, e, ids = s[perm], e[perm], ids[perm]
    lengths = np.full(n_contigs, L, np.uint32)
    starts_1 = np.arange(0, L, 1000, dtype=np.uint32)
    offs = (np.arange(n_contigs + 1) * starts_1.size).astype(np.uint32)
    r0 = np.tile(starts_1, n_contigs)
    r1 = r0 + 899
    caps = np.full(r0.size, M, np.uint32)
    ds, de, di = _dev(s), _dev(e), _dev(ids)
    d_plain = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device="cuda:0")
    d_prof = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    plain = lambda: solver.solve_by_contig_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M,
                                                  d_plain.data_ptr())
    prof = lambda: solver.solve_profile_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M,
                                               d_prof.data_ptr(), offs, r0, r1, caps)
    with solver.options(near_uniform=-1, speculation=-1, cut_points=-1):
        plain(); prof()                                                          # warm-up: arena growth
        assert solver.last_stats.path == 2
        t_plain, t_prof, ms_need = [], [], []
        for _ in range(5):
            t_plain.append(timed(plain))
            assert solver.last_stats.path == 2 and solver.last_stats.spec_boundaries == 0
            t_prof.append(timed(prof))
            ms_need.append(float(solver.last_profile_stats.ms_profile))
    assert torch.equal(d_plain, d_prof)
    a, b = statistics.median(t_plain), statistics.median(t_prof)
    figures = {"reads": n, "contigs": n_contigs, "positions": int(n_contigs * L), "M": M, "regions": int(r0.size),
               "plain_ms_median": round(a, 3), "plain_ms_runs": [round(x, 3) for x in t_plain],
               "profile_ms_median": round(b, 3), "profile_ms_runs": [round(x, 3) for x in t_prof],
               "k_profile_need_ms_median": round(statistics.median(ms_need), 4),
               "ratio": round(b / a, 4), "margin": COST_MARGIN}
    print("profile_time " + json.dumps(figures))
    out = os.environ.get("QMCP_PROFILE_TIME_OUT")
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(figures, indent=1) + "\n")
    assert b <= COST_MARGIN * a, figures
