"""qmcp_hip_solve_replicates_*: one read set split into disjoint downsamples in one by-contig call, every further
replicate solved on the reads the earlier ones left free.  The label bytes are compared byte for byte with the model on
the oracle (tests/replicates_model.py)."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import multi_reference as mr
import profile_model as pm
import replicates_model as rm

pytestmark = pytest.mark.gpu

COVERAGE_LISTS = [[5, 5, 5, 5], [3] * 6, [30, 10, 30], [1, 1, 1], [8], [2, 40], [20] * 16, [4, 9, 4, 9]]
SEEDS = 48
MODES = (0, rm.WHOLE_PAIRS)
TILE = 1024          # qmcp::kRepTileReads: the candidates one workgroup of k_rep_split takes at a time


def case(seed):
    rng = np.random.default_rng(3000 + seed)
    s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(1, 7)), max_reads_per_contig=2500)
    if s.size % 2:
        s, e, ids = s[:-1], e[:-1], ids[:-1]            # whole pairs need an even number of reads
    return s, e, ids, lengths, COVERAGE_LISTS[seed % len(COVERAGE_LISTS)]


@pytest.fixture(scope="module")
def expected(oracle):
    """the model's labels and counts of every seed in both modes, computed once"""
    return [[rm.replicate_labels(oracle, *case(seed), flags) for flags in MODES] for seed in range(SEEDS)]


def counts_of(rs, k):
    return {name: list(getattr(rs, name)[:k]) for name in ("n_offered", "n_kept", "n_mates")}


def plain_fields(st):
    """what of a qmcp_hip_stats describes the solve itself, not the run: the counts, the spans and the route"""
    return {k: getattr(st, k) for k in ("n_reads", "n_kept", "total_length", "n_contigs", "path", "min_span", "max_span",
                                        "sort_passes", "sweep_stretches")}


def test_labels_and_counts_equal_the_model(solver, expected):
    for seed in range(SEEDS):
        s, e, ids, lengths, cov = case(seed)
        solver.solve_by_contig(s, e, ids, lengths, cov[0])
        plain = plain_fields(solver.last_stats)
        for m, flags in enumerate(MODES):
            want, info = expected[seed][m]
            got = solver.solve_replicates(s, e, ids, lengths, cov, flags)
            assert got.dtype == np.uint8 and np.array_equal(got, want), f"seed {seed}, flags {flags}: {cov}, {s.size} reads"
            rs = solver.last_replicates_stats
            assert rs.n_replicates == len(cov) and rs.flags == flags
            assert counts_of(rs, len(cov)) == info, f"seed {seed}, flags {flags}"
            assert not any(rs.n_kept[len(cov):]) and not any(rs.n_offered[len(cov):])
            assert not any(rs.short_positions) and not any(rs.short_bases) and rs.n_full == 0   # no SHORTFALL flag
            assert plain_fields(solver.last_stats) == plain                      # replicate 1 is the plain call
            reps = solver.last_replicate_solve_stats
            assert len(reps) == len(cov) and plain_fields(reps[0]) == plain
            for r in range(len(cov)):
                assert reps[r].n_reads == info["n_offered"][r] and reps[r].n_kept == info["n_kept"][r] - info["n_mates"][r]


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
            ptr = [t.data_ptr() + 4 * shift for t in cols]
            assert all(p % 16 == 4 * shift for p in ptr)
            for m, flags in enumerate(MODES):
                d_labels = torch.full((n + shift + 4,), 0xFF, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                rs = solver.solve_replicates_device(ptr[0], ptr[1], ptr[2], n, lengths, cov, d_labels.data_ptr() + shift,
                                                    flags=flags, stream=torch.cuda.current_stream().cuda_stream)
                got = d_labels.cpu().numpy()
                want, info = expected[seed][m]
                assert np.array_equal(got[shift:shift + n], want), f"seed {seed}, shift {shift}, flags {flags}"
                assert (got[:shift] == 0xFF).all() and (got[shift + n:] == 0xFF).all()   # nothing written outside
                assert counts_of(rs, len(cov)) == info


def both_modes(oracle, solver, s, e, ids, lengths, cov, what):
    for flags in MODES:
        if flags and s.size % 2:
            continue
        got = solver.solve_replicates(s, e, ids, lengths, cov, flags)
        want, info = rm.replicate_labels(oracle, s, e, ids, lengths, cov, flags)
        assert got.size == s.size and np.array_equal(got, want), (what, cov, flags)
        assert counts_of(solver.last_replicates_stats, len(cov)) == info, (what, cov, flags)


def test_edge_sizes(pkg, oracle, solver):
    rng = np.random.default_rng(78)
    for n in (0, 1, 3, 4, 5, 63, 64, 65, 129, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 3):
        span = rng.integers(1, 60, size=n)
        s = (rng.random(n) * (500 - span + 1)).astype(np.uint32)
        e = (s + span - 1).astype(np.uint32)
        ids = np.zeros(n, np.uint32)
        for cov in ([3, 3, 3], [4], [1, 9, 2], [50, 50, 50]):
            both_modes(oracle, solver, s, e, ids, [500], cov, n)
    # contig offsets on multiples of 64 (the reads are grouped stably: counts of 64, 128, 0, 192 and 64)
    counts = [64, 128, 0, 192, 64]
    lengths = np.array([300, 500, 40, 700, 200], np.uint32)
    ids = rng.permutation(np.repeat(np.arange(5, dtype=np.uint32), counts))
    span = rng.integers(1, 40, size=ids.size)
    s = (rng.random(ids.size) * (lengths[ids] - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    for cov in ([2, 2, 2, 2], [5, 1, 5]):
        both_modes(oracle, solver, s, e, ids, lengths, cov, "offsets on multiples of 64")
    # every read unplaced
    n = 200
    s, e = rng.integers(0, 1 << 31, size=n).astype(np.uint32), rng.integers(0, 1 << 31, size=n).astype(np.uint32)
    for flags in MODES:
        got = solver.solve_replicates(s, e, np.full(n, mr.NO_CONTIG, np.uint32), [1000, 10], [5, 2, 5], flags)
        rs = solver.last_replicates_stats
        assert got.size == n and not got.any() and not any(rs.n_kept) and not any(rs.n_offered)
    # a contig without reads between two with reads
    n = 700
    ids = np.where(rng.random(n) < 0.5, 0, 2).astype(np.uint32)
    lengths = np.array([1000, 400, 800], np.uint32)
    span = rng.integers(1, 90, size=n)
    s = (rng.random(n) * (lengths[ids] - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    for cov in ([12, 4, 1], [6, 6, 6, 6]):
        both_modes(oracle, solver, s, e, ids, lengths, cov, "empty contig")
    # a replicate that takes every remaining read of one contig (contig 0: depth <= 3) but not of the others
    ids2 = ids.copy()
    thin = np.flatnonzero(ids2 == 0)[12:]
    ids2[thin] = 2
    s2 = np.where(ids2 == 2, np.minimum(s, 800 - span), s).astype(np.uint32)
    e2 = (s2 + span - 1).astype(np.uint32)
    cov = [3, 3, 3]
    want, info = rm.replicate_labels(oracle, s2, e2, ids2, lengths, cov)
    assert 0 < int((want[ids2 == 0] != 0).sum()) == int((ids2 == 0).sum()) and (want[ids2 == 2] == 0).any()
    both_modes(oracle, solver, s2, e2, ids2, lengths, cov, "one contig emptied")
    # a first coverage above every depth: replicate 1 keeps every placed read, the rest are empty
    for flags in MODES:
        got = solver.solve_replicates(s, e, ids, lengths, [100_000, 4, 4], flags)
        rs = solver.last_replicates_stats
        assert (got == 1).all() and list(rs.n_kept[:3]) == [n, 0, 0] and list(rs.n_offered[:3]) == [n, 0, 0]


def test_one_replicate_is_the_plain_call_and_the_second_the_plain_call_on_the_rest(pkg, solver):
    for seed in (3, 8, 21):
        s, e, ids, lengths, _ = case(seed)
        for M in (1, 9, 60):
            plain = solver.solve_by_contig(s, e, ids, lengths, M)
            n_kept = solver.last_stats.n_kept
            labels = solver.solve_replicates(s, e, ids, lengths, [M])
            assert int(labels.max(initial=0)) <= 1 and np.array_equal(pkg.replicate_mask(labels, 1), plain)
            assert solver.last_stats.n_kept == n_kept == solver.last_replicates_stats.n_kept[0]
            assert solver.last_stats.n_reads == int((ids != mr.NO_CONTIG).sum())
        labels = solver.solve_replicates(s, e, ids, lengths, [9, 6])
        rest = np.flatnonzero((labels != 1) & (ids != mr.NO_CONTIG))
        second = solver.solve_by_contig(s[rest], e[rest], ids[rest], lengths, 6)
        assert np.array_equal(pkg.replicate_mask(labels[rest], 2), second)


def deep_one_length(clipped):
    L, n = 20_000, 300_000
    rng = np.random.default_rng(5)
    s = rng.integers(0, L - 150 + 1, size=n).astype(np.uint32)
    e = (s + 149).astype(np.uint32)
    if clipped:
        short = rng.random(n) < 0.01
        e = np.where(short, s + rng.integers(30, 149, size=n), e).astype(np.uint32)
    return s, e, np.zeros(n, np.uint32), [L]


def test_later_replicates_stay_on_the_ranked_route(pkg, oracle, solver):
    """300 000 reads of 150 bases on 20 000 positions at [100, 100, 100]: the model keeps 13 400 per replicate and
    leaves 286 600 and 273 200 reads, so every replicate is above rank_min_reads and takes the range-ranked route"""
    s, e, ids, lengths = deep_one_length(False)
    cov = [100, 100, 100]
    want, info = rm.replicate_labels(oracle, s, e, ids, lengths, cov)
    assert info["n_kept"] == [13_400] * 3 and info["n_offered"] == [300_000, 286_600, 273_200]
    got = solver.solve_replicates(s, e, ids, lengths, cov)
    assert np.array_equal(got, want)
    reps = solver.last_replicate_solve_stats
    assert [r.sort_passes for r in reps] == [1, 1, 1], [r.as_dict() for r in reps]
    assert counts_of(solver.last_replicates_stats, 3) == info
    got = solver.solve_replicates(s, e, ids, lengths, cov, rm.WHOLE_PAIRS)
    assert np.array_equal(got, rm.replicate_labels(oracle, s, e, ids, lengths, cov, rm.WHOLE_PAIRS)[0])


def test_one_percent_clipped_reads_still_equal_the_model(pkg, oracle, solver):
    s, e, ids, lengths = deep_one_length(True)
    cov = [100, 100, 100]
    got = solver.solve_replicates(s, e, ids, lengths, cov)
    assert np.array_equal(got, rm.replicate_labels(oracle, s, e, ids, lengths, cov)[0])


TWO_BATCH_LENGTHS = [1_200_000_000, 1_150_000_123, 5_000]


@functools.lru_cache(maxsize=None)
def two_batch_instance():
    inst = rm.island_pairs(83, TWO_BATCH_LENGTHS, 300, per_island=40)
    return inst, pm.compact(*inst)[:4]


def test_two_position_batches_with_mates_across_them(pkg, oracle, solver):
    """two contigs of about 1.2e9 positions (one call takes 2^31 - 2) and a short third: contig 0 is a batch of its own,
    and most pairs have their mates in different batches, so a replicate's completion needs every batch's labels.  Under
    cut_points = 1 (stretches): one chain per contig would walk 1.2e9 positions.  The model runs on
    profile_model.compact's copy"""
    inst, model_inst = two_batch_instance()
    s, e, ids, lengths = inst
    L = lengths.astype(np.int64)
    assert int(L[:2].sum()) > (1 << 31) - 2 >= int(L[1:].sum())
    batch_of = (ids != 0).astype(np.int64)
    assert int(np.count_nonzero(batch_of[0::2] != batch_of[1::2])) > 50
    cov = [3, 3, 3, 3]
    labels = []
    for flags in MODES:
        want, info = rm.replicate_labels(oracle, *model_inst, cov, flags)
        assert all(info["n_kept"])                                           # four non-empty replicates
        with solver.options(cut_points=1):
            got = solver.solve_replicates(s, e, ids, lengths, cov, flags)
        assert np.array_equal(got, want), flags
        assert counts_of(solver.last_replicates_stats, 4) == info
        assert solver.last_stats.total_length == int(L.sum()) and solver.last_stats.n_contigs == 3
        labels.append(got)
    assert int((labels[0] != labels[1]).sum()) > 100                         # the flag changes the split


def test_shortfall_equals_the_numpy_model_and_the_depth_report(pkg, oracle, solver):
    for seed in (1, 6, 14, 22, 31):
        s, e, ids, lengths, cov = case(seed)
        for m, flags in enumerate(MODES):
            labels = solver.solve_replicates(s, e, ids, lengths, cov, flags | rm.SHORTFALL)
            rs = solver.last_replicates_stats
            want, info = rm.replicate_labels(oracle, s, e, ids, lengths, cov, flags)
            assert np.array_equal(labels, want) and counts_of(rs, len(cov)) == info
            sp, sb, n_full = rm.shortfall(want, s, e, ids, lengths, cov)
            assert list(rs.short_positions[:len(cov)]) == sp and list(rs.short_bases[:len(cov)]) == sb, (seed, flags)
            assert rs.n_full == n_full and sp[0] == 0
            assert not any(rs.short_positions[len(cov):]) and not any(rs.short_bases[len(cov):])
            for r, M in enumerate(cov, start=1):
                rep = solver.depth_report(s, e, ids, lengths, M, keep_mask=pkg.replicate_mask(labels, r))
                assert int(rep.contig_rows["deficit_positions"].sum()) == sp[r - 1]
                assert int(rep.contig_rows["deficit_sum"].sum()) == sb[r - 1]
            # without the flag the fields are all 0
            solver.solve_replicates(s, e, ids, lengths, cov, flags)
            rs = solver.last_replicates_stats
            assert not any(rs.short_positions) and not any(rs.short_bases) and rs.n_full == 0


def raw_host(pkg, solver, s, e, ids, lengths, cov, k, flags, labels, null_cov=False, n=None):
    """the host entry itself, on a label buffer the caller owns -> status code"""
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    cov = np.ascontiguousarray(cov, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    return pkg._hip.qmcp_hip_solve_replicates_host(solver._ctx, p(s), p(e), p(ids), s.size if n is None else n, p(lengths),
                                                   lengths.size, None if null_cov else p(cov), k, flags,
                                                   C.c_void_p(labels.ctypes.data), None, None, None)


def test_errors_leave_the_output_untouched(pkg, solver):
    torch = pytest.importorskip("torch")
    s = np.array([0, 5, 9, 2], np.uint32)
    e = np.array([3, 8, 9, 6], np.uint32)
    ids = np.array([0, 1, 1, 0], np.uint32)
    lengths = [10, 10]
    fresh = lambda: np.full(s.size, 0xFF, np.uint8)
    E, R = pkg.QMCP_EINVAL, pkg.QMCP_ERANGE
    host_side = [([], 0, 0, None, E), ([3] * 17, 17, 0, None, E), ([3, 0], 2, 0, None, E), ([0], 1, 0, None, E),
                 ([1 << 31], 1, 0, None, R), ([5, 0xFFFFFFFF], 2, 0, None, R), ([5, 5], 2, 4, None, E),
                 ([5, 5], 2, 0x10, None, E), ([5, 5], 2, 1, 3, E), ([5, 5], 2, 3, 3, E)]
    for cov, k, flags, n, code in host_side:
        labels = fresh()
        assert raw_host(pkg, solver, s, e, ids, lengths, cov or [1], k, flags, labels, n=n) == code, (cov, flags, n)
        assert (labels == 0xFF).all(), cov
    labels = fresh()
    assert raw_host(pkg, solver, s, e, ids, lengths, [3, 1], 2, 0, labels, null_cov=True) == E
    assert (labels == 0xFF).all()
    for cov, flags in (([5, 0], 0), ([], 0), ([2, 3], 8)):
        with pytest.raises(pkg.QmcpError) as ex:
            solver.solve_replicates(s, e, ids, lengths, cov, flags)
        assert ex.value.code == E
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_replicates(s[:3], e[:3], ids[:3], lengths, [2, 2], rm.WHOLE_PAIRS)
    assert ex.value.code == E
    # bad id / bad read: found on the device; the host entry does not write labels_out, the device bytes are all zero
    dev = torch.device("cuda", 0)
    bad = [(np.array([0, 2, 1, 0], np.uint32), [10, 10], E),                    # id 2 of 2 contigs
           (ids, [10, 9], pkg.QMCP_EREAD)]                                     # end 9 on a 9-position contig
    for bad_ids, bad_lengths, code in bad:
        for flags in (0, 3):
            labels = fresh()
            assert raw_host(pkg, solver, s, e, bad_ids, bad_lengths, [3, 1], 2, flags, labels) == code
            assert (labels == 0xFF).all()
            t = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, bad_ids)]
            d_labels = torch.full((s.size + 3,), 0xFF, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            with pytest.raises(pkg.QmcpError) as ex:
                solver.solve_replicates_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), s.size, bad_lengths,
                                               [3, 1], d_labels.data_ptr(), flags=flags,
                                               stream=torch.cuda.current_stream().cuda_stream)
            assert ex.value.code == code
            got = d_labels.cpu().numpy()
            assert not got[:s.size].any() and (got[s.size:] == 0xFF).all()
    # the context still works
    assert solver.solve_replicates(s, e, ids, lengths, [2, 1], 3).size == 4


def test_two_runs_give_identical_bytes(solver):
    s, e, ids, lengths, _ = case(13)
    rng = np.random.default_rng(99)
    s2, e2, ids2, lengths2 = mr.random_by_contig(rng, 5, max_reads_per_contig=40_000)
    s2, e2, ids2 = s2[:s2.size & ~1], e2[:s2.size & ~1], ids2[:s2.size & ~1]
    for flags in (0, 3):
        for args in ((s, e, ids, lengths, [5, 5, 5, 5]), (s2, e2, ids2, lengths2, [30, 10, 30])):
            a = solver.solve_replicates(*args, flags).copy()
            b = solver.solve_replicates(*args, flags)
            assert np.array_equal(a, b)


def test_the_host_entry_leaves_replicate_1_in_the_context(pkg, solver):
    s, e, ids, lengths, _ = case(5)
    pkg._hip.qmcp_hip_kept_indices_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    for flags in MODES:
        labels = solver.solve_replicates(s, e, ids, lengths, [9, 2, 9], flags)
        out = np.zeros(s.size, np.uint64)
        n_out = C.c_uint64(0)
        rc = pkg._hip.qmcp_hip_kept_indices_host(solver._ctx, s.size, C.c_void_p(out.ctypes.data), out.size, C.byref(n_out))
        assert rc == pkg.QMCP_OK
        assert np.array_equal(out[:n_out.value], np.flatnonzero(labels == 1))


def test_the_split_takes_no_longer_than_the_chain_of_plain_calls(pkg, solver):
    """2 M reads on 8 contigs, coverages [100] * 4, median of 5 runs after a warm-up, both timed by the wall clock around
    blocking calls in this process.  The chain is the only route without the entry: solve_by_contig_device per replicate,
    on columns whose complement was compacted with torch in between -- it regroups the reads at every replicate."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    n_contigs, pairs, L, cov = 8, 125_000, 20_000, [100] * 4
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, seed=500 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
    perm = np.random.default_rng(8).permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    n = s.size
    lengths = np.full(n_contigs, L, np.uint32)
    d_s, d_e, d_ids = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids))
    d_labels = torch.zeros(n, dtype=torch.uint8, device=dev)
    shifts = torch.arange(64, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def split():
        solver.solve_replicates_device(d_s.data_ptr(), d_e.data_ptr(), d_ids.data_ptr(), n, lengths, cov,
                                       d_labels.data_ptr(), stream=stream)

    def chain():
        cols, free = (d_s, d_e, d_ids), torch.arange(n, device=dev)
        out = torch.zeros(n, dtype=torch.uint8, device=dev)
        for r, M in enumerate(cov, start=1):
            m = cols[0].numel()
            mask = torch.zeros(pkg.mask_words(m), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            solver.solve_by_contig_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), m, lengths, M,
                                          mask.data_ptr(), stream=stream)
            bits = ((mask.unsqueeze(1) >> shifts) & 1).flatten()[:m].bool()
            out[free[bits]] = r
            cols = tuple(c[~bits].contiguous() for c in cols)
            free = free[~bits]
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
    split()
    assert torch.equal(d_labels, want)               # the same replicates either way
    t_chain, t_split = median_ms(chain), median_ms(split)
    rs = solver.last_replicates_stats.as_dict()
    print(f"replicates {t_split:.3f} ms, chain of plain calls {t_chain:.3f} ms; {rs}")
    assert t_split <= t_chain, (t_split, t_chain, rs)


def test_file_to_file_replicates(pkg, oracle, tmp_path):
    """downsample_bam(per_reference=True, replicates=3) at M = 10: every file holds the records of the model's label set
    in file order -- no find_pairs follows --, the files are pairwise disjoint by record, and the counts, the report and
    every refused combination are as documented"""
    import bam_py
    refs = [("chr1", 30_000), ("chr2", 12_000), ("chr3", 5_000), ("chrM", 1_600)]
    path = tmp_path / "multi.bam"
    header, parsed, _ = mr.write_multi_reference_bam(path, np.random.default_rng(19), refs, 20_000)
    cols = pkg.read_bam(path, per_reference=True)
    s, e, ids, lengths = cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"]
    bam_ids = np.asarray(cols["bam_ids"], np.int64)
    assert s.size % 2 == 0
    M = 10
    out, template, report = tmp_path / "out.bam", tmp_path / "out.rep{R}.bam", tmp_path / "replicates.tsv"
    for replicates, cov in ((3, [M, M, M]), ([4, 25], [M, 4, 25]), (1, [M])):
        written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, replicates=replicates,
                                     replicates_out=template, replicates_report=report)
        assert isinstance(written, list) and len(written) == len(cov)
        labels, info = rm.replicate_labels(oracle, s, e, ids, lengths, cov, rm.WHOLE_PAIRS)
        sp, sb, n_full = rm.shortfall(labels, s, e, ids, lengths, cov)
        files = [out] + [tmp_path / f"out.rep{r}.bam" for r in range(2, len(cov) + 1)]
        seen = set()
        for r, f in enumerate(files, start=1):
            kept_ids = np.sort(bam_ids[labels == r])
            oh, orecs, _ = bam_py.parse(f)
            assert oh == header and written[r - 1] == kept_ids.size == len(orecs) > 0, f
            assert [x["raw"] for x in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()], f
            assert not seen & set(kept_ids.tolist())                               # pairwise disjoint by record
            seen |= set(kept_ids.tolist())
        lines = [line.split("\t") for line in report.read_text().splitlines() if not line.startswith("#")]
        assert lines[-1] == ["n_full", str(n_full)] and len(lines) == len(cov) + 1
        for r, row in enumerate(lines[:-1]):
            assert [int(x) for x in row] == [r + 1, cov[r], info["n_offered"][r], info["n_kept"][r], info["n_mates"][r],
                                             sp[r], sb[r], written[r]]
    # what the flow refuses
    bed = tmp_path / "t.bed"
    for kwargs, word in [(dict(per_reference=False), "per_reference"), (dict(replicates_out=tmp_path / "out.bam"), "{R}"),
                         (dict(replicates=0), "1 .."), (dict(replicates=17), "1 .."), (dict(replicates=[3] * 16), "at most"),
                         (dict(replicates=[3, 0]), "coverage"), (dict(targets=bed), "targets"),
                         (dict(report=tmp_path / "r.tsv"), "report"), (dict(track=tmp_path / "t.bg"), "track"),
                         (dict(ladder=[5], ladder_out=tmp_path / "l.{M}.bam"), "ladder"), (dict(stratify="strand"), "stratify"),
                         (dict(dedup=True), "dedup"), (dict(profile=tmp_path / "p.bg"), "profile"),
                         (dict(pair_aware=True), "pair_aware"), (dict(template_aware=True), "template_aware"),
                         (dict(ceiling=True), "ceiling"), (dict(budget_reads=100), "budget"),
                         (dict(budget_fraction=0.5), "budget"), (dict(bed=bed, amplicons_by_reference=True), "amplicon")]:
        args = dict(per_reference=True, replicates=3, replicates_out=template)
        args.update(kwargs)
        with pytest.raises(ValueError, match=word.replace("{", r"\{").replace("}", r"\}")):
            pkg.downsample_bam("quasi-mcp-hip", path, out, M, **args)
    with pytest.raises(ValueError, match="quality"):
        pkg.downsample_bam("quasi-mcp-hip-quality", path, out, M, per_reference=True, replicates=3, replicates_out=template)
    with pytest.raises(ValueError, match="need replicates"):
        pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, replicates_out=template)
