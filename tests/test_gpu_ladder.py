"""qmcp_hip_solve_ladder_*: one by-contig call at several falling coverages, every further level solved on the reads the
level above kept.  The level bytes are compared byte for byte with the model on the oracle (tests/ladder_model.py)."""
import ctypes as C
import time

import numpy as np
import pytest

import ladder_model as lm
import multi_reference as mr

pytestmark = pytest.mark.gpu

COVERAGE_LISTS = [[50, 12, 3, 1], [3], [200, 199], [7, 1], [40, 12, 3, 1], [100, 50, 25, 10], [2, 1], [30, 29, 28, 2]]
SEEDS = 48


def case(seed):
    rng = np.random.default_rng(1000 + seed)
    s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(1, 7)), max_reads_per_contig=2500)
    return s, e, ids, lengths, COVERAGE_LISTS[seed % len(COVERAGE_LISTS)]


@pytest.fixture(scope="module")
def expected(oracle):
    """the model's level bytes of every seed, computed once"""
    return [lm.ladder_levels(oracle, *case(seed)) for seed in range(SEEDS)]


def raw_host(pkg, solver, s, e, ids, lengths, cov, n_levels, levels, null_cov=False):
    """the host entry itself, on a levels buffer the caller owns -> status code"""
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    cov = np.ascontiguousarray(cov, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    return pkg._hip.qmcp_hip_solve_ladder_host(solver._ctx, p(s), p(e), p(ids), s.size, p(lengths), lengths.size,
                                               None if null_cov else p(cov), n_levels, C.c_void_p(levels.ctypes.data),
                                               None, None)


def test_levels_and_counts_equal_the_model(solver, expected):
    for seed in range(SEEDS):
        s, e, ids, lengths, cov = case(seed)
        got = solver.solve_ladder(s, e, ids, lengths, cov)
        assert got.dtype == np.uint8 and np.array_equal(got, expected[seed]), f"seed {seed}: {cov}, {s.size} reads"
        ls = solver.last_ladder_stats
        assert ls.n_levels == len(cov) and list(ls.n_kept[:len(cov)]) == lm.n_kept(expected[seed], len(cov)), f"seed {seed}"
        assert not any(ls.n_kept[len(cov):])
        assert solver.last_stats.n_kept == ls.n_kept[0]


def test_device_entry_aligned_and_one_element_off(pkg, solver, expected):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    for seed in range(0, SEEDS, 4):
        s, e, ids, lengths, cov = case(seed)
        n = s.size
        for shift in (0, 1):
            cols = []
            for x in (s, e, ids):
                t = torch.zeros(n + shift + 4, dtype=torch.int32, device=dev)   # (a base allocation is 256-byte aligned)
                t[shift:shift + n] = torch.from_numpy(x.view(np.int32)).to(dev)
                cols.append(t)
            d_levels = torch.full((n + shift + 4,), 0xFF, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ptr = [t.data_ptr() + 4 * shift for t in cols]
            assert all(p % 16 == 4 * shift for p in ptr)
            ls = solver.solve_ladder_device(ptr[0], ptr[1], ptr[2], n, lengths, cov, d_levels.data_ptr() + shift,
                                            stream=torch.cuda.current_stream().cuda_stream)
            got = d_levels.cpu().numpy()
            assert np.array_equal(got[shift:shift + n], expected[seed]), f"seed {seed}, shift {shift}"
            assert (got[:shift] == 0xFF).all() and (got[shift + n:] == 0xFF).all()   # nothing written outside
            assert list(ls.n_kept[:len(cov)]) == lm.n_kept(expected[seed], len(cov))


def test_one_level_is_the_plain_by_contig_call(pkg, solver):
    for seed in (3, 8, 21):
        s, e, ids, lengths, _ = case(seed)
        for M in (1, 9, 60):
            plain = solver.solve_by_contig(s, e, ids, lengths, M)
            n_kept = solver.last_stats.n_kept
            levels = solver.solve_ladder(s, e, ids, lengths, [M])
            assert int(levels.max(initial=0)) <= 1 and np.array_equal(pkg.ladder_mask(levels, 0), plain)
            assert solver.last_stats.n_kept == n_kept == solver.last_ladder_stats.n_kept[0]
            assert solver.last_stats.n_reads == int((ids != mr.NO_CONTIG).sum())


def test_edge_sizes(pkg, oracle, solver):
    rng = np.random.default_rng(77)
    for n in (0, 1, 63, 64, 65, 129):
        span = rng.integers(1, 60, size=n)
        s = (rng.random(n) * (500 - span + 1)).astype(np.uint32)
        e = (s + span - 1).astype(np.uint32)
        ids = np.zeros(n, np.uint32)
        for cov in ([3, 1], [4], [9, 5, 2]):
            got = solver.solve_ladder(s, e, ids, [500], cov)
            assert got.size == n and np.array_equal(got, lm.ladder_levels(oracle, s, e, ids, [500], cov)), (n, cov)
    # every read unplaced
    n = 200
    s, e = rng.integers(0, 1 << 31, size=n).astype(np.uint32), rng.integers(0, 1 << 31, size=n).astype(np.uint32)
    got = solver.solve_ladder(s, e, np.full(n, mr.NO_CONTIG, np.uint32), [1000, 10], [5, 2])
    assert got.size == n and not got.any() and list(solver.last_ladder_stats.n_kept[:2]) == [0, 0]
    # a contig without reads between two with reads
    n = 700
    ids = np.where(rng.random(n) < 0.5, 0, 2).astype(np.uint32)
    lengths = np.array([1000, 400, 800], np.uint32)
    span = rng.integers(1, 90, size=n)
    s = (rng.random(n) * (lengths[ids] - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    for cov in ([12, 4, 1], [6, 5]):
        got = solver.solve_ladder(s, e, ids, lengths, cov)
        assert np.array_equal(got, lm.ladder_levels(oracle, s, e, ids, lengths, cov)), cov
    # a first coverage above every depth keeps every placed read; the next level is then the plain call
    got = solver.solve_ladder(s, e, ids, lengths, [100_000, 4])
    assert (got >= 1).all() and solver.last_ladder_stats.n_kept[0] == n
    assert np.array_equal(pkg.ladder_mask(got, 1), solver.solve_by_contig(s, e, ids, lengths, 4))


def test_first_level_ranked_later_levels_small(pkg, oracle, solver):
    """one call above rank_min_reads: the first level takes the range-ranked route, the later levels (some 13 000 and
    4 000 reads) the sort-based one"""
    L, n, cov = 20_000, 300_000, [100, 30, 5]
    rng = np.random.default_rng(5)
    s = rng.integers(0, L - 150 + 1, size=n).astype(np.uint32)
    e = (s + 149).astype(np.uint32)
    ids = np.zeros(n, np.uint32)
    got = solver.solve_ladder(s, e, ids, [L], cov)
    st, ls = solver.last_stats, solver.last_ladder_stats
    assert st.sort_passes == 1, st.as_dict()                       # the ranked route, as for the plain call
    assert 0 < ls.n_kept[2] < ls.n_kept[1] < ls.n_kept[0] < (1 << 17)
    assert np.array_equal(got, lm.ladder_levels(oracle, s, e, ids, [L], cov))


def test_errors_leave_the_output_untouched(pkg, solver):
    torch = pytest.importorskip("torch")
    s = np.array([0, 5, 9, 2], np.uint32)
    e = np.array([3, 8, 9, 6], np.uint32)
    ids = np.array([0, 1, 1, 0], np.uint32)
    lengths = [10, 10]
    fresh = lambda: np.full(s.size, 0xFF, np.uint8)
    host_side = [([], 0), (list(range(17, 0, -1)), 17), ([5, 5], 2), ([5, 6], 2), ([9, 4, 4], 3), ([3, 0], 2), ([0], 1)]
    for cov, k in host_side:
        levels = fresh()
        assert raw_host(pkg, solver, s, e, ids, lengths, cov or [1], k, levels) == pkg.QMCP_EINVAL, cov
        assert (levels == 0xFF).all(), cov
    levels = fresh()
    assert raw_host(pkg, solver, s, e, ids, lengths, [3, 1], 2, levels, null_cov=True) == pkg.QMCP_EINVAL
    assert (levels == 0xFF).all()
    for cov in ([5, 5], [], [2, 3]):
        with pytest.raises(pkg.QmcpError) as ex:
            solver.solve_ladder(s, e, ids, lengths, cov)
        assert ex.value.code == pkg.QMCP_EINVAL
    # bad id / bad read: found on the device; the host entry does not write levels_out, the device bytes are all zero
    dev = torch.device("cuda", 0)
    bad = [(np.array([0, 2, 1, 0], np.uint32), [10, 10], pkg.QMCP_EINVAL),      # id 2 of 2 contigs
           (ids, [10, 9], pkg.QMCP_EREAD)]                                     # end 9 on a 9-position contig
    for bad_ids, bad_lengths, code in bad:
        levels = fresh()
        assert raw_host(pkg, solver, s, e, bad_ids, bad_lengths, [3, 1], 2, levels) == code
        assert (levels == 0xFF).all()
        t = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, bad_ids)]
        d_levels = torch.full((s.size + 3,), 0xFF, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with pytest.raises(pkg.QmcpError) as ex:
            solver.solve_ladder_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), s.size, bad_lengths, [3, 1],
                                       d_levels.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        assert ex.value.code == code
        got = d_levels.cpu().numpy()
        assert not got[:s.size].any() and (got[s.size:] == 0xFF).all()
    # the context still works
    assert solver.solve_ladder(s, e, ids, lengths, [2, 1]).size == 4


def test_two_runs_give_identical_bytes(solver):
    s, e, ids, lengths, _ = case(13)
    rng = np.random.default_rng(99)
    s2, e2, ids2, lengths2 = mr.random_by_contig(rng, 5, max_reads_per_contig=40_000)
    for args in ((s, e, ids, lengths, [40, 12, 3, 1]), (s2, e2, ids2, lengths2, [60, 20, 4])):
        a = solver.solve_ladder(*args).copy()
        b = solver.solve_ladder(*args)
        assert np.array_equal(a, b)


def test_the_host_entry_leaves_level_0_in_the_context(pkg, solver):
    s, e, ids, lengths, _ = case(5)
    levels = solver.solve_ladder(s, e, ids, lengths, [9, 2])
    out = np.zeros(s.size, np.uint64)
    n_out = C.c_uint64(0)
    pkg._hip.qmcp_hip_kept_indices_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    rc = pkg._hip.qmcp_hip_kept_indices_host(solver._ctx, s.size, C.c_void_p(out.ctypes.data), out.size, C.byref(n_out))
    assert rc == pkg.QMCP_OK
    assert np.array_equal(out[:n_out.value], np.flatnonzero(levels >= 1))
    assert np.array_equal(pkg.ladder_mask(levels, 0), solver.solve_by_contig(s, e, ids, lengths, 9))


def test_file_to_file_ladder(pkg, oracle, tmp_path):
    """downsample_bam(per_reference=True, ladder=[20, 5]): every written file is find_pairs of the model's level, and
    each file's records are a subset of the file above"""
    import bam_py
    refs = [("chr1", 30_000), ("chr2", 12_000), ("chr3", 5_000), ("chrM", 1_600)]
    path = tmp_path / "multi.bam"
    header, parsed, ref_lengths = mr.write_multi_reference_bam(path, np.random.default_rng(19), refs, 20_000)
    reads, ids, filtered = mr.expected_per_reference_reads(parsed)
    starts = np.array([r["start"] if i != mr.NO_CONTIG else 0 for r, i in zip(reads, ids)], dtype=np.int64)
    ends = np.array([r["end"] if i != mr.NO_CONTIG else 0 for r, i in zip(reads, ids)], dtype=np.int64)
    M, ladder = 40, [20, 5]
    out = tmp_path / "out.bam"
    template = tmp_path / "out.{M}x.bam"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, ladder=ladder, ladder_out=template)
    assert isinstance(written, list) and len(written) == 3
    levels = lm.ladder_levels(oracle, starts.astype(np.uint32), ends.astype(np.uint32), ids, ref_lengths, [M] + ladder)
    bam_ids = np.array([r["bam_id"] for r in reads], dtype=np.int64)
    files = [out] + [tmp_path / f"out.{m}x.bam" for m in ladder]
    above = None
    for j, f in enumerate(files):
        mask = oracle.find_pairs(lm.level_mask(levels, j), len(reads))
        kept_ids = np.sort(bam_ids[pkg.mask_to_indices(mask, len(reads)).astype(np.int64)])
        oh, orecs, _ = bam_py.parse(f)
        assert oh == header and written[j] == kept_ids.size == len(orecs), f
        assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()], f
        names = {r["raw"] for r in orecs}
        assert above is None or names <= above
        assert above is None or len(names) < len(above)
        above = names
    # what the ladder refuses
    for kwargs, word in [(dict(per_reference=False), "per_reference"),
                         (dict(ladder_out=tmp_path / "out.bam"), "{M}"),
                         (dict(ladder=[40, 5]), "below"), (dict(ladder=[5, 20]), "decreas"), (dict(ladder=[20, 20]), "decreas"),
                         (dict(targets=tmp_path / "t.bed"), "targets"), (dict(report=tmp_path / "r.tsv"), "report")]:
        args = dict(per_reference=True, ladder=ladder, ladder_out=template)
        args.update(kwargs)
        with pytest.raises(ValueError, match=word.replace("{", r"\{").replace("}", r"\}")):
            pkg.downsample_bam("quasi-mcp-hip", path, out, M, **args)
    with pytest.raises(ValueError, match="quality"):
        pkg.downsample_bam("quasi-mcp-hip-quality", path, out, M, per_reference=True, ladder=ladder, ladder_out=template)


def test_the_ladder_takes_no_longer_than_the_chain_of_plain_calls(pkg, solver):
    """2 M reads on 8 contigs, coverages [100, 50, 25, 10], median of 5 runs after a warm-up, both timed by the wall
    clock around blocking calls in this process.  The chain is the only route without the ladder: solve_by_contig_device
    at each coverage, on columns compacted with torch between the calls -- it regroups the reads at every level."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    n_contigs, pairs, L, cov = 8, 125_000, 20_000, [100, 50, 25, 10]
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, seed=500 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
    perm = np.random.default_rng(8).permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    n = s.size
    lengths = np.full(n_contigs, L, np.uint32)
    d_s, d_e, d_ids = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids))
    d_levels = torch.zeros(n, dtype=torch.uint8, device=dev)
    shifts = torch.arange(64, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def ladder():
        solver.solve_ladder_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, cov, d_levels.data_ptr(),
                                   stream=stream)

    def chain():
        cols, alive = (d_s, d_e, d_ids), torch.arange(n, device=dev)
        out = torch.zeros(n, dtype=torch.uint8, device=dev)
        for M in cov:
            m = cols[0].numel()
            mask = torch.zeros(pkg.mask_words(m), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            solver.solve_by_contig_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), m, lengths, M,
                                          mask.data_ptr(), stream=stream)
            bits = ((mask.unsqueeze(1) >> shifts) & 1).flatten()[:m].bool()
            cols = tuple(c[bits].contiguous() for c in cols)
            alive = alive[bits]
            out[alive] += 1
        torch.cuda.synchronize()
        return out

    def median_ms(f):
        f()
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return sorted(times)[2]

    want = chain()
    ladder()
    assert torch.equal(d_levels, want)               # the same nested levels either way
    t_chain, t_ladder = median_ms(chain), median_ms(ladder)
    ls = solver.last_ladder_stats.as_dict()
    print(f"ladder {t_ladder:.3f} ms, chain of plain calls {t_chain:.3f} ms; levels {ls}")
    assert t_ladder <= t_chain, (t_ladder, t_chain, ls)
