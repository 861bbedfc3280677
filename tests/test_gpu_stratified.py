"""qmcp_hip_solve_stratified_*: one coverage cap per stratum.  The mask is compared bit for bit with the model on the
oracle (tests/stratified_model.py: per stratum, the by-contig selection of that stratum's reads alone, ORed), the rows
with numpy sums."""
import ctypes as C

import numpy as np
import pytest

import multi_reference as mr
import stratified_model as sm

pytestmark = pytest.mark.gpu

SEEDS = 48
STRATA_COUNTS = [1, 2, 3, 7]
CAPS = [0, 1, 3, 12, 50, 200]


def case(seed):
    rng = np.random.default_rng(7000 + seed)
    s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(1, 7)), max_reads_per_contig=2500)
    n_strata = STRATA_COUNTS[seed % len(STRATA_COUNTS)]
    strata = sm.random_strata(rng, s.size, n_strata)            # about 3 % NO_STRATUM
    caps = rng.choice(CAPS, size=n_strata).astype(np.uint32)
    return s, e, ids, strata, lengths, caps


@pytest.fixture(scope="module")
def expected(oracle):
    """the model's kept bits of every seed, computed once"""
    return [sm.stratified_bits(oracle, *case(seed)) for seed in range(SEEDS)]


def check_rows(solver, s, e, ids, strata, n_strata, keep_bits):
    got = sm.rows_of(solver.last_stratum_rows)
    want = sm.rows(s, e, ids, strata, n_strata, keep_bits)
    assert got.shape == want.shape and np.array_equal(got, want), (got, want)
    assert solver.last_stats.n_kept == want[:, 1].sum() and solver.last_stats.n_reads == want[:, 0].sum()


def test_mask_and_rows_equal_the_model(solver, expected):
    for seed in range(SEEDS):
        s, e, ids, strata, lengths, caps = case(seed)
        got = solver.solve_stratified(s, e, ids, strata, lengths, caps)
        assert np.array_equal(got, sm.pack(expected[seed])), f"seed {seed}: caps {caps}, {s.size} reads"
        check_rows(solver, s, e, ids, strata, caps.size, expected[seed])
        assert solver.last_stats.n_kept == sum(r.n_kept for r in solver.last_stratum_rows)


def test_one_stratum_is_the_plain_by_contig_call(solver):
    for seed in (3, 8, 21):
        s, e, ids, _, lengths, _ = case(seed)
        for M in (1, 9, 60):
            plain = solver.solve_by_contig(s, e, ids, lengths, M)
            n_kept, n_reads = solver.last_stats.n_kept, solver.last_stats.n_reads
            got = solver.solve_stratified(s, e, ids, np.zeros(s.size, np.uint32), lengths, [M])
            assert np.array_equal(got, plain)
            assert solver.last_stats.n_kept == n_kept == solver.last_stratum_rows[0].n_kept
            assert solver.last_stats.n_reads == n_reads == solver.last_stratum_rows[0].n_reads


def test_every_stratum_is_valid_by_the_depth_report(solver):
    """independent of the model: the depth report of a stratum's reads alone (the others unplaced) against the stratified
    mask has no position short of min(the stratum's coverage, its cap)"""
    for seed in range(6):
        s, e, ids, strata, lengths, caps = case(seed)
        mask = solver.solve_stratified(s, e, ids, strata, lengths, caps)
        for k in range(caps.size):
            alone = np.where(strata == k, ids, mr.NO_CONTIG).astype(np.uint32)
            report = solver.depth_report(s, e, alone, lengths, int(caps[k]), keep_mask=mask)
            assert report.valid, f"seed {seed}, stratum {k} (cap {caps[k]}): {report.stats.as_dict()}"


def test_device_entry_aligned_and_one_element_off(pkg, solver, expected):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    guard = -0x0123456789ABCDEF
    for seed in range(0, SEEDS, 6):
        s, e, ids, strata, lengths, caps = case(seed)
        n, words = s.size, pkg.mask_words(s.size)
        for shift in (0, 1):
            cols = []
            for x in (s, e, ids, strata):
                t = torch.zeros(n + shift + 4, dtype=torch.int32, device=dev)   # (a base allocation is 256-byte aligned)
                t[shift:shift + n] = torch.from_numpy(x.view(np.int32)).to(dev)
                cols.append(t)
            d_mask = torch.full((words + 3,), guard, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            ptr = [t.data_ptr() + 4 * shift for t in cols]
            assert all(p % 16 == 4 * shift for p in ptr)
            st = solver.solve_stratified_device(ptr[0], ptr[1], ptr[2], ptr[3], n, lengths, caps, d_mask.data_ptr(),
                                                stream=torch.cuda.current_stream().cuda_stream)
            got = d_mask.cpu().numpy()
            assert np.array_equal(got[:words].view(np.uint64), sm.pack(expected[seed])), f"seed {seed}, shift {shift}"
            assert (got[words:] == guard).all()                                  # nothing beyond ceil(n / 64) words
            assert st.n_kept == expected[seed].sum()
            check_rows(solver, s, e, ids, strata, caps.size, expected[seed])


def test_edge_sizes(oracle, solver):
    rng = np.random.default_rng(77)

    def run(s, e, ids, strata, lengths, caps):
        got = solver.solve_stratified(s, e, ids, strata, lengths, caps)
        want = sm.stratified_bits(oracle, s, e, ids, strata, lengths, caps)
        assert got.size == (s.size + 63) // 64 and np.array_equal(got, sm.pack(want)), (s.size, caps)
        check_rows(solver, s, e, ids, strata, len(caps), want)
        return want

    for n in (0, 1, 63, 64, 65, 129):
        span = rng.integers(1, 60, size=n)
        s = (rng.random(n) * (500 - span + 1)).astype(np.uint32)
        e = (s + span - 1).astype(np.uint32)
        ids = np.zeros(n, np.uint32)
        for caps in ([3, 1], [4], [9, 0, 2]):
            run(s, e, ids, rng.integers(0, len(caps), size=n).astype(np.uint32), [500], caps)
    n = 700
    lengths = np.array([1000, 400, 800], np.uint32)
    ids = np.where(rng.random(n) < 0.5, 0, 2).astype(np.uint32)          # a contig without reads
    span = rng.integers(1, 90, size=n)
    s = (rng.random(n) * (lengths[ids] - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    # every read without a stratum
    kept = run(s, e, ids, np.full(n, sm.NO_STRATUM, np.uint32), lengths, [5, 2])
    assert not kept.any() and solver.last_stats.n_reads == 0
    # a stratum with no reads between two that have reads
    run(s, e, ids, np.where(rng.random(n) < 0.5, 0, 2).astype(np.uint32), lengths, [6, 6, 2])
    # a stratum with cap 0 between two with caps
    strata = rng.integers(0, 3, size=n).astype(np.uint32)
    kept = run(s, e, ids, strata, lengths, [6, 0, 2])
    assert not kept[strata == 1].any() and kept[strata == 0].any() and kept[strata == 2].any()
    assert solver.last_stratum_rows[1].n_reads == (strata == 1).sum() and solver.last_stratum_rows[1].n_kept == 0


def _tally_case(pkg, rng, n, run_lengths):
    """n reads on one contig, shuffled; in grouped order the strata form runs of the given lengths"""
    assert sum(run_lengths) == n
    strata = np.repeat(np.arange(len(run_lengths), dtype=np.uint32), run_lengths)
    span = rng.integers(1, 200, size=n)
    s = (rng.random(n) * (5000 - span + 1)).astype(np.uint32)
    e = (s + span - 1).astype(np.uint32)
    perm = rng.permutation(n)
    return s[perm], e[perm], np.zeros(n, np.uint32), strata[perm]


def test_tally_edges(pkg, solver):
    """the rows against numpy where k_st_tally's runs meet the edges of its waves and workgroups: 1 000 strata of 1 to 3
    reads each (runs shorter than a wave, beginning and ending at every lane, 0, 63 and 64 included), and one stratum
    that spans every workgroup; the sizes sit on both sides of the kernel's tile"""
    T = pkg.STRATUM_TALLY_TILE
    rng = np.random.default_rng(31)
    for n in (T - 1, T, T + 1, 2 * T + 65):
        runs = np.ones(1000, dtype=np.int64)                     # 1 000 <= n <= 3 000 for a tile of 1 024
        assert runs.size <= n <= 3 * runs.size
        while runs.sum() < n:
            k = int(rng.integers(0, runs.size))
            runs[k] += runs[k] < 3
        starts_of_runs = np.concatenate([[0], np.cumsum(runs)[:-1]]) % 64
        assert {0, 63}.issubset(set(starts_of_runs.tolist()))    # a run begins at lane 0 (the one before ends at 63), at 63
        for run_lengths, caps in ((runs, rng.choice([0, 1, 2], size=runs.size)), (np.array([n]), [4])):
            s, e, ids, strata = _tally_case(pkg, rng, n, run_lengths)
            mask = solver.solve_stratified(s, e, ids, strata, [5000], caps)
            keep = sm.unpack(mask, n)
            check_rows(solver, s, e, ids, strata, len(caps), keep)
            got = sm.rows_of(solver.last_stratum_rows)
            assert np.array_equal(got[:, 0], run_lengths)
            assert np.array_equal(got[:, 2], np.bincount(strata, weights=(e.astype(np.int64) - s + 1), minlength=len(caps)))


def test_ranked_route_inside_each_stratum(pkg, solver):
    """two strata, each above rank_min_reads, one read length on two contigs: every stratum's solve takes the
    range-ranked route, and the mask is the two plain by-contig calls on the split columns"""
    threshold = solver.get_options().rank_min_reads or (1 << 17)       # 0: the library's default, 2^17 (qmcp_hip.h)
    n = 2 * threshold + 40_000
    rng = np.random.default_rng(5)
    lengths = np.array([20_000, 15_000], np.uint32)
    ids = rng.integers(0, 2, size=n).astype(np.uint32)
    s = (rng.random(n) * (lengths[ids] - 150 + 1)).astype(np.uint32)
    e = (s + 149).astype(np.uint32)
    strata = (np.arange(n) % 2).astype(np.uint32)
    rng.shuffle(strata)
    caps = [100, 30]
    assert min((strata == 0).sum(), (strata == 1).sum()) >= threshold
    got = sm.unpack(solver.solve_stratified(s, e, ids, strata, lengths, caps), n)
    st = solver.last_stats
    assert st.path == pkg.PATH_UNIFORM and st.sort_passes == 1, st.as_dict()
    want = np.zeros(n, dtype=bool)
    for k, M in enumerate(caps):
        on = np.flatnonzero(strata == k)
        want[on[sm.unpack(solver.solve_by_contig(s[on], e[on], ids[on], lengths, M), on.size)]] = True
        assert solver.last_stats.sort_passes == 1
    assert np.array_equal(got, want)


def raw_host(pkg, solver, s, e, ids, strata, lengths, caps, n_strata, mask, null_caps=False, n_contigs=None):
    """the host entry itself, on a mask buffer the caller owns -> status code"""
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    caps = np.ascontiguousarray(caps, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    return pkg._hip.qmcp_hip_solve_stratified_host(solver._ctx, p(s), p(e), p(ids), p(strata), s.size, p(lengths),
                                                   lengths.size if n_contigs is None else n_contigs,
                                                   None if null_caps else p(caps), n_strata,
                                                   mask.ctypes.data_as(C.POINTER(C.c_uint64)), None, None)


def test_errors_leave_the_guard_intact_and_the_context_usable(pkg, solver):
    torch = pytest.importorskip("torch")
    s = np.array([0, 5, 9, 2], np.uint32)
    e = np.array([3, 8, 9, 6], np.uint32)
    ids = np.array([0, 1, 1, 0], np.uint32)
    strata = np.array([0, 1, 1, 0], np.uint32)
    lengths = [10, 10]
    guard = np.uint64(0xA5A5A5A5A5A5A5A5)
    fresh = lambda: np.full(4, guard, np.uint64)

    def good():
        # at cap 1 every read is needed: 0-3 and 2-6 each cover positions of contig 0 alone, 5-8 and 9-9 do not overlap
        assert sm.unpack(solver.solve_stratified(s, e, ids, strata, lengths, [1, 1]), 4).all()
        assert not sm.unpack(solver.solve_stratified(s, e, ids, strata, lengths, [1, 0]), 4)[1:3].any()

    big = np.zeros(65537, np.uint32)
    assert 257 * 65281 == (1 << 24) + 1                   # 2^24 + 1 = 97 * 257 * 673: 257 strata on 65 281 contigs
    long_lengths = np.full(65281, 10, np.uint32)
    cases = [
        (dict(strata=np.array([0, 2, 1, 0], np.uint32)), [1, 1], 2, pkg.QMCP_EINVAL, "2"),       # stratum id n_strata
        (dict(), [1], 0, pkg.QMCP_EINVAL, "n_strata"),
        (dict(), big, 65537, pkg.QMCP_ERANGE, "65537"),
        (dict(lengths=long_lengths), np.ones(257, np.uint32), 257, pkg.QMCP_ERANGE, str((1 << 24) + 1)),
        (dict(null_caps=True), [1, 1], 2, pkg.QMCP_EINVAL, "max_coverages"),
        (dict(ids=np.array([0, 2, 1, 0], np.uint32)), [1, 1], 2, pkg.QMCP_EINVAL, "contig id"),
        (dict(lengths=[10, 9]), [1, 1], 2, pkg.QMCP_EREAD, "read"),
    ]
    for kwargs, caps, n_strata, code, word in cases:
        args = dict(s=s, e=e, ids=ids, strata=strata, lengths=lengths)
        null_caps = kwargs.pop("null_caps", False)
        args.update(kwargs)
        mask = fresh()
        rc = raw_host(pkg, solver, args["s"], args["e"], args["ids"], args["strata"], args["lengths"], caps, n_strata, mask,
                      null_caps=null_caps)
        assert rc == code, (kwargs, rc)
        assert word in pkg._hip.qmcp_hip_last_error().decode(), pkg._hip.qmcp_hip_last_error()
        assert (mask == guard).all(), kwargs                # the host entry does not write keep_mask_out
        good()
    # the device entry: a bad stratum id is found on the device; the mask's own word is cleared, nothing beyond it
    dev = torch.device("cuda", 0)
    bad = np.array([0, 7, 1, 0], np.uint32)
    t = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids, bad)]
    d_mask = torch.full((4,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_stratified_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), 4, lengths,
                                       [1, 1], d_mask.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    assert ex.value.code == pkg.QMCP_EINVAL and "stratum" in str(ex.value)
    got = d_mask.cpu().numpy()
    assert got[0] == 0 and (got[1:] == -0x5A5A5A5A5A5A5A5B).all()
    good()


@pytest.mark.parametrize("stratify", ["read_group", "strand"])
def test_file_to_file(pkg, oracle, tmp_path, stratify):
    """downsample_bam(per_reference=True, stratify=...): the written records are find_pairs of the model's mask on
    read_bam's columns with the caps the flow documents, and the TSV's counts are the rows of that mask"""
    import bam_py
    path = tmp_path / "groups.bam"
    header, parsed, ref_lengths = sm.write_stratified_bam(path, np.random.default_rng(23))
    cols = pkg.read_bam(path, per_reference=True, stratify=stratify)
    n, names = cols["starts"].size, cols["stratum_names"]
    M = 7
    caps = [M - M // 2, M // 2] if stratify == "strand" else [M] * len(names)
    placed = cols["contig_ids"] != mr.NO_CONTIG
    s, e = np.where(placed, cols["starts"], 0).astype(np.uint32), np.where(placed, cols["ends"], 0).astype(np.uint32)
    keep = sm.stratified_bits(oracle, s, e, cols["contig_ids"], cols["strata"], cols["contig_lengths"], caps)
    assert 0 < keep.sum() < placed.sum()
    out, tsv = tmp_path / "out.bam", tmp_path / "strata.tsv"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, stratify=stratify, strata_report=tsv)
    mask = oracle.find_pairs(sm.pack(keep), n)
    kept_ids = np.sort(cols["bam_ids"][pkg.mask_to_indices(mask, n).astype(np.int64)].astype(np.int64))
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == kept_ids.size == len(orecs)
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]
    want = sm.rows(s, e, cols["contig_ids"], cols["strata"], len(names), keep)
    lines = [l.split("\t") for l in open(tsv).read().splitlines() if not l.startswith("#")]
    assert [l[0] for l in lines] == names and [int(l[1]) for l in lines] == caps
    assert [[int(l[2]), int(l[3])] for l in lines] == want[:, :2].tolist()
    total = float(sum(ref_lengths))
    for l, row in zip(lines, want):
        assert abs(float(l[4]) - row[2] / total) < 1e-5 and abs(float(l[5]) - row[3] / total) < 1e-5
