"""qmcp_hip_solve_ceiling_*: kept depth never above the cap, the most reads kept.  Every mask is compared bit for bit
with tests/ceiling_model.py (the dropped set as profile_model's canonical selection under max(cov - cap, 0), complemented
over the placed reads), every field of qmcp_hip_ceiling_stats with its numpy restatement, and in the random calls the mask
also with the complement of solve_profile's answer under the dual cap array as regions: the same need by another route."""
import ctypes as C

import numpy as np
import pytest
import torch

import bam_py
import ceiling_model as cm
import multi_reference as mr
import profile_model as pm

pytestmark = pytest.mark.gpu

NO_CONTIG = 0xFFFFFFFF
COUNTS = ["reads_placed", "reads_dropped", "mates_dropped", "over_positions", "over_bases", "short_positions",
          "short_bases", "excess_positions", "max_kept_depth", "regions_in", "regions_used"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")


def reads_on(rng, n, lengths, lo, hi, unplaced=0.0):
    """n reads with spans lo..hi on random contigs (clipped to short contigs), a share of them unplaced"""
    lengths = np.atleast_1d(lengths).astype(np.int64)
    ids = rng.integers(0, lengths.size, n)
    span = np.minimum(rng.integers(lo, hi + 1, n), lengths[ids])
    s = (rng.random(n) * (lengths[ids] - span + 1)).astype(np.int64)
    e = s + span - 1
    ids = ids.astype(np.uint32)
    ids[rng.random(n) < unplaced] = NO_CONTIG
    return s.astype(np.uint32), e.astype(np.uint32), ids


def check(solver, s, e, ids, lengths, default, table=(None, None, None, None), flags=0, via_profile=False, model_lengths=None):
    """the host entry against the model and the restated stats; -> (mask, ceiling stats, stats)"""
    n = s.size
    ml = lengths if model_lengths is None else model_lengths
    got = solver.solve_ceiling(s, e, ids, lengths, default, *table, flags=flags)
    cs, st = solver.last_ceiling_stats, solver.last_stats
    want = cm.expected_mask(s, e, ids, ml, default, *table, whole_pairs=bool(flags & 1), fast=True)
    assert np.array_equal(got, want), int(np.count_nonzero(pm.unpack(got ^ want, n))) if n else 0
    restated = cm.stats(s, e, ids, ml, default, *table, whole_pairs=bool(flags & 1), fast=True)
    assert {k: int(getattr(cs, k)) for k in COUNTS} == restated
    assert cs.excess_positions == 0
    if via_profile:
        dual = cm.dual_regions(s, e, ids, ml, default, *table)
        dropped = pm.unpack(solver.solve_profile(s, e, ids, lengths, 0, *dual), n)
        assert np.array_equal(got, pm.pack((ids != NO_CONTIG) & ~dropped))
    return got, cs, st


def kept_depth_at_most(s, e, ids, lengths, mask, caps):
    kept = pm.unpack(mask, s.size)
    for c, cap in enumerate(caps):
        sel = kept & (ids == c)
        assert np.all(pm.coverage(s[sel].astype(np.int64), e[sel].astype(np.int64), int(lengths[c])) <= cap), c


# ------------------------------------------------------------------------------------------ random calls
@pytest.mark.parametrize("block", range(4))
def test_random_small_calls(solver, block):
    """40 seeded calls in four blocks: 1..5 contigs of 50..3 000 positions (one of them without reads when there are
    several), 0..4 000 reads of spans 1..200, a tenth of them unplaced, caps 0..default + 3 in regions with a cap-0 run"""
    for seed in range(10 * block, 10 * block + 10):
        rng = np.random.default_rng(4100 + seed)
        lengths = rng.integers(50, 3001, int(rng.integers(1, 6))).astype(np.uint32)
        n = int(rng.integers(0, 4001)) if seed % 10 else 0
        s, e, ids = reads_on(rng, n, lengths, 1, 200, unplaced=0.1)
        if lengths.size > 1:
            ids[ids == lengths.size - 1] = NO_CONTIG                             # a contig without reads
        default = [0, 1, 3, 20][seed % 4]
        table = pm.random_regions(rng, lengths, default + 3, zero_run=12)
        got, _, _ = check(solver, s, e, ids, lengths, default, table, via_profile=True)
        kept_depth_at_most(s, e, ids, lengths, got, pm.cap_arrays(lengths, default, *table))


@pytest.mark.parametrize("L", [61, 62, 63, 64])
def test_axis_length_modulo_four(solver, L):
    rng = np.random.default_rng(4200 + L)
    s, e, ids = reads_on(rng, 500, [L], 1, 20)
    cap = rng.integers(0, 40, L)
    cap[L - 1] = 3                                                               # a region that ends on the last position
    check(solver, s, e, ids, [L], 2, pm.regions_of(cap), via_profile=True)
    check(solver, s, e, ids, [L], 50)                                            # no region at all


@pytest.mark.parametrize("n_regions", [4095, 4096, 4097])
def test_region_table_in_lds_and_through_l2(solver, n_regions):
    """one-position regions on one 20 000-position contig: the LDS table at its limit and the L2 path just past it"""
    L = 20_000
    rng = np.random.default_rng(4300 + n_regions)
    s, e, ids = reads_on(rng, 3000, [L], 1, 200)
    r0 = (np.arange(n_regions) * 4 + 1).astype(np.uint32)
    table = (np.array([0, n_regions], np.uint32), r0, r0.copy(), rng.integers(0, 12, n_regions).astype(np.uint32))
    _, cs, _ = check(solver, s, e, ids, [L], 10, table)
    assert cs.regions_used == n_regions and cs.over_positions > 0


# ------------------------------------------------------------------------------------------ caps around the depth
def test_caps_from_zero_to_above_the_depth(solver):
    L = 2000
    rng = np.random.default_rng(4400)
    s, e, ids = reads_on(rng, 1500, [L], 1, 120, unplaced=0.05)
    (cov, _, _), = cm.dual_caps(s, e, ids, [L], 0)
    placed = int((ids != NO_CONTIG).sum())
    _, cs, st = check(solver, s, e, ids, [L], 0, pm.regions_of(cov))             # cap == cov everywhere: nothing to drop
    assert cs.reads_dropped == 0 and st.sweep_stretches == 0 and st.n_kept == 0
    _, cs, _ = check(solver, s, e, ids, [L], 0, pm.regions_of(np.maximum(cov - 1, 0)))
    assert cs.over_positions == int((cov > 0).sum()) and cs.reads_dropped > 0
    _, cs, st = check(solver, s, e, ids, [L], 0, pm.regions_of(cov + 1))
    assert cs.reads_dropped == 0 and st.sweep_stretches == 0
    _, cs, _ = check(solver, s, e, ids, [L], 0)                                  # cap 0 everywhere: the full demand
    assert cs.reads_dropped == placed and cs.max_kept_depth == 0 and cs.over_bases == int(cov.sum())
    solver.set_profiling(True)
    try:
        got, cs, st = check(solver, s, e, ids, [L], int(cov.max()) + 1)         # above the largest depth: no sweep queued
        times = solver.kernel_times()
    finally:
        solver.set_profiling(False)
    assert not any(k.startswith("k_sweep") or k == "k_mark" for k in times), times
    assert times["k_ceiling_need"][0] == times["k_ceiling_check"][0] == times["k_ceiling_finish"][0] == 1
    assert st.sweep_stretches == 0 and cs.reads_dropped == 0 and cs.over_positions == 0
    assert np.array_equal(pm.unpack(got, s.size), ids != NO_CONTIG)


# ------------------------------------------------------------------------------------------ the two capped walks
@pytest.mark.parametrize("max_span, kernel", [(448, "k_sweep_general_reg(capped)"), (600, "k_sweep_general(capped)")])
def test_both_capped_walks(solver, max_span, kernel):
    """spans up to 448: the register-resident walk; up to 600: the plain capped walk; two contigs, depth about 6 x cap"""
    cap, lengths = 5, np.array([6000, 5000], np.uint32)
    rng = np.random.default_rng(4500 + max_span)
    n = int(6 * cap * int(lengths.sum()) / ((max_span + 150) / 2))
    s, e, ids = reads_on(rng, n, lengths, 150, max_span)
    s[1], e[1], ids[1] = 0, max_span - 1, 0                                      # the longest span is there
    solver.set_profiling(True)
    try:
        got, cs, st = check(solver, s, e, ids, lengths, cap, via_profile=True)
        times = solver.kernel_times()
    finally:
        solver.set_profiling(False)
    assert st.max_span == max_span and kernel in times, times
    assert cs.max_kept_depth <= cap and cs.reads_dropped > n // 2
    kept_depth_at_most(s, e, ids, lengths, got, [np.full(int(L), cap) for L in lengths])


# ------------------------------------------------------------------------------------------ cut points
@pytest.mark.parametrize("zero_run", [False, True])
def test_stretches_start_behind_uncovered_and_cap_zero_positions(solver, zero_run):
    """three read islands separated by uncovered gaps on one contig: with cut points on, the sweep runs in more
    stretches than there are contigs and gives the mask of the one-chain walk; the same with a cap-0 run in the middle of
    an island (need == cov there as well)"""
    L, cap = 30_000, 4
    rng = np.random.default_rng(4600)
    parts = []
    for a in (1000, 12_000, 23_000):
        s, e, _ = reads_on(rng, 2500, [5000], 20, 50)
        parts.append((s + a, e + a))
    s = np.concatenate([p[0] for p in parts]).astype(np.uint32)
    e = np.concatenate([p[1] for p in parts]).astype(np.uint32)
    perm = rng.permutation(s.size)
    s, e = s[perm], e[perm]
    ids = np.zeros(s.size, np.uint32)
    table = (np.array([0, 1], np.uint32), np.array([14_000], np.uint32), np.array([14_100], np.uint32),
             np.array([0], np.uint32)) if zero_run else (None, None, None, None)
    with solver.options(cut_points=-1):
        chain, _, st = check(solver, s, e, ids, [L], cap, table)
        assert st.sweep_stretches == 1
    with solver.options(cut_points=1):
        cut, cs, st = check(solver, s, e, ids, [L], cap, table)
        assert st.sweep_stretches > 1
    assert np.array_equal(chain, cut) and cs.max_kept_depth <= cap


# ------------------------------------------------------------------------------------------ batches
def test_several_batches(solver):
    """300 contigs in one call (256 and more: one workgroup per contig, no windows); two of them are empty and as long as
    one solver call allows, so the by-contig layer cuts the call into several batches -- three of them with reads.  The
    model sees the two empty contigs at length 1: a contig without reads decides nothing"""
    rng = np.random.default_rng(4700)
    lengths = rng.integers(100, 400, 300).astype(np.uint32)
    s, e, ids = reads_on(rng, 9000, lengths, 5, 60, unplaced=0.1)
    for c in (100, 200):
        ids[ids == c] = NO_CONTIG
    model_lengths = lengths.copy()
    lengths[[100, 200]] = (1 << 31) - 3
    model_lengths[[100, 200]] = 1
    table = pm.random_regions(rng, model_lengths, 4)
    _, cs, st = check(solver, s, e, ids, lengths, 2, table, model_lengths=model_lengths)
    assert st.n_contigs == 300 and cs.reads_dropped > 0


def test_one_length_deep_data(solver):
    """20 000 positions, reads of 150 at 6 x M, M = 20: the kept depth recomputed in numpy is at most M everywhere"""
    L, M = 20_000, 20
    rng = np.random.default_rng(4800)
    s, e, ids = reads_on(rng, 6 * M * L // 150, [L], 150, 150)
    got, cs, _ = check(solver, s, e, ids, [L], M)
    kept_depth_at_most(s, e, ids, [L], got, [np.full(L, M)])
    assert cs.max_kept_depth <= 20 and cs.excess_positions == 0


# ------------------------------------------------------------------------------------------ whole pairs
def test_whole_pairs(pkg, solver):
    """mates on the same and on other contigs, unplaced mates; the final mask holds whole pairs among the placed reads
    and never an unplaced read; an odd n_reads is refused"""
    rng = np.random.default_rng(4900)
    lengths = np.array([3000, 1500, 800], np.int64)
    first = rng.integers(0, 3, 3000)
    c = np.empty(6000, np.int64)
    c[0::2] = first
    c[1::2] = np.where(rng.random(3000) < 0.6, first, rng.integers(0, 3, 3000))  # most pairs lie on one contig
    span = rng.integers(30, 151, 6000)
    s = (rng.random(6000) * (lengths[c] - span + 1)).astype(np.int64)
    s, e = s.astype(np.uint32), (s + span - 1).astype(np.uint32)
    ids = c.astype(np.uint32)
    ids[rng.random(6000) < 0.08] = NO_CONTIG
    table = pm.random_regions(rng, lengths, 6, zero_run=20)
    got, cs, _ = check(solver, s, e, ids, lengths, 4, table, flags=pkg.CEILING_WHOLE_PAIRS)
    plain, ps, _ = check(solver, s, e, ids, lengths, 4, table)
    kept, placed = pm.unpack(got, s.size), ids != NO_CONTIG
    both = placed[0::2] & placed[1::2]
    assert np.array_equal(kept[0::2][both], kept[1::2][both]) and not kept[~placed].any()
    assert cs.mates_dropped > 0 and cs.reads_dropped == ps.reads_dropped + cs.mates_dropped
    assert (cs.short_positions, cs.short_bases, cs.max_kept_depth) == (ps.short_positions, ps.short_bases, ps.max_kept_depth)
    kept_depth_at_most(s, e, ids, lengths, got, pm.cap_arrays(lengths, 4, *table))
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_ceiling(s[:-1], e[:-1], ids[:-1], lengths, 4, flags=pkg.CEILING_WHOLE_PAIRS)
    assert ex.value.code == pkg.QMCP_EINVAL
    solver.solve_ceiling(s[:-1], e[:-1], ids[:-1], lengths, 4)                   # odd is fine without the flag


# ------------------------------------------------------------------------------------------ entries, errors
def test_device_entry_after_a_callers_stream_equals_the_host_entry(pkg, solver):
    rng = np.random.default_rng(5000)
    lengths = np.array([2500, 900], np.uint32)
    s, e, ids = reads_on(rng, 3001, lengths, 1, 200, unplaced=0.1)               # (an odd count, not a multiple of 4)
    table = pm.random_regions(rng, lengths, 5, zero_run=10)
    want, hs, _ = check(solver, s, e, ids, lengths, 3, table)
    n = s.size
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ds, de = _dev(s), _dev(e)
        di = _dev(np.concatenate([[7], ids]))[1:]                                # the id column off 16-byte alignment
        d_mask = torch.full((pkg.mask_words(n) + 1,), -1, dtype=torch.int64, device="cuda:0")
        cs = solver.solve_ceiling_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, 3, d_mask.data_ptr(),
                                         *table, stream=stream.cuda_stream)
    out = d_mask.cpu().numpy().view(np.uint64)
    assert out[pkg.mask_words(n)] == np.uint64(0xFFFFFFFFFFFFFFFF)               # nothing written past the mask
    assert np.array_equal(out[:pkg.mask_words(n)], want)
    assert {k: int(getattr(cs, k)) for k in COUNTS} == {k: int(getattr(hs, k)) for k in COUNTS}


def test_errors_leave_the_mask_alone(pkg, solver):
    s, e = np.array([0, 5], np.uint32), np.array([9, 20], np.uint32)
    ids, lengths = np.zeros(2, np.uint32), np.array([100], np.uint32)
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    cases = [([0, 2], [10, 20], [20, 30], [1, 1], 3, 0, 2, pkg.QMCP_EINVAL),     # overlap
             ([0, 1], [9], [3], [1], 3, 0, 2, pkg.QMCP_EINVAL),                   # start > end
             ([1, 1], [9], [9], [1], 3, 0, 2, pkg.QMCP_EINVAL),                   # offsets do not start at 0
             ([0, 1], [1], [2], [1 << 31], 3, 0, 2, pkg.QMCP_ERANGE),             # a cap of 2^31
             ([0, 1], [1], [2], [1], 1 << 31, 0, 2, pkg.QMCP_ERANGE),             # default_cap of 2^31
             ([0, 1], [1], [2], [1], 3, 2, 2, pkg.QMCP_EINVAL),                   # an unknown flag bit
             ([0, 1], [1], [2], [1], 3, 1, 1, pkg.QMCP_EINVAL)]                   # whole pairs, an odd n_reads
    for offs, r0, r1, caps, default, flags, n, code in cases:
        mask = np.full(1, 0xDEADBEEF, np.uint64)
        u = [np.array(x, np.uint32) for x in (offs, r0, r1, caps)]
        rc = pkg._hip.qmcp_hip_solve_ceiling_host(solver._ctx, p32(s), p32(e), p32(ids), n, p32(lengths), 1, p32(u[0]),
                                                  p32(u[1]), p32(u[2]), p32(u[3]), default, flags,
                                                  mask.ctypes.data_as(C.POINTER(C.c_uint64)), None, None)
        assert rc == code and mask[0] == 0xDEADBEEF, (offs, flags, rc)
    d_mask = torch.full((1,), 0x5EED, dtype=torch.int64, device="cuda:0")
    ds, de, di = _dev(s), _dev(e), _dev(ids)
    torch.cuda.synchronize()
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_ceiling_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), 2, lengths, 3, d_mask.data_ptr(),
                                    [0, 2], [10, 20], [20, 30], [1, 1])
    torch.cuda.synchronize()
    assert ex.value.code == pkg.QMCP_EINVAL and int(d_mask.cpu()[0]) == 0x5EED


# ------------------------------------------------------------------------------------------ the file flow
def test_downsample_bam_ceiling_writes_whole_pairs_under_the_cap(pkg, solver, tmp_path):
    """a multi-reference paired BAM through downsample_bam(ceiling=True): the records of the model's final mask and no
    others -- no find_pairs follows --, placed mates written together, the depth of the written records at most the cap,
    the statistics in ceiling_report; then the same under a bedGraph of ceilings"""
    path = tmp_path / "in.bam"
    refs = [("chrA", 5000), ("chrB", 3000), ("chrC", 1200)]
    header, parsed, _ = mr.write_multi_reference_bam(path, np.random.default_rng(17), refs, 1500)
    cols = pkg.read_bam(path, per_reference=True)
    s, e, ids, lengths = cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"]
    n = s.size
    assert n % 2 == 0 and n > 2000
    graph = tmp_path / "caps.bedgraph"
    graph.write_text("chrA\t100\t900\t2\nchrA\t2000\t2600\t0\nchrB\t0\t3000\t9\n")
    M = 6
    for profile in (None, graph):
        table = (None,) * 4 if profile is None else pkg.profile_from_bedgraph(profile, pkg.reference_names(path))
        want = cm.expected_mask(s, e, ids, lengths, M, *table, whole_pairs=True, fast=True)
        restated = cm.stats(s, e, ids, lengths, M, *table, whole_pairs=True, fast=True)
        kept = pm.unpack(want, n)
        assert 0 < kept.sum() < (ids != NO_CONTIG).sum()                          # the ceiling bites
        kept_ids = np.sort(np.asarray(cols["bam_ids"], np.int64)[np.flatnonzero(kept)])
        out, report = tmp_path / "out.bam", tmp_path / "ceiling.tsv"
        written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, ceiling=True, profile=profile,
                                     ceiling_report=report)
        oh, orecs, _ = bam_py.parse(out)
        assert oh == header and written == kept_ids.size == len(orecs)
        assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]
        placed = ids != NO_CONTIG
        both = placed[0::2] & placed[1::2]
        assert np.array_equal(kept[0::2][both], kept[1::2][both])                # every written record's placed mate is written
        kept_depth_at_most(s, e, ids, lengths, want, pm.cap_arrays(lengths, M, *table))
        rows = dict(line.split("\t") for line in report.read_text().splitlines() if not line.startswith("#"))
        assert {k: int(rows[k]) for k in COUNTS} == restated and int(rows["records_written"]) == written
