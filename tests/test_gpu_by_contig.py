"""qmcp_hip_solve_by_contig_*: reads of several contigs in any order, one contig id each, grouped on the device and
solved per contig.  Every mask here is compared bit for bit: with the oracle run per contig on that contig's reads in
input order, with qmcp_hip_solve_host on reads already grouped, or with one qmcp_hip_solve_host call per contig where
the genome is past one call's position limit."""
import numpy as np
import pytest

import multi_reference as mr

pytestmark = pytest.mark.gpu


def test_random_shuffled_contigs_equal_the_oracle_per_contig(pkg, oracle, solver):
    rng = np.random.default_rng(41)
    for trial in range(24):
        n_contigs = int(rng.integers(1, 41))
        s, e, ids, lengths = mr.random_by_contig(rng, n_contigs)
        M = int(rng.integers(1, 40))
        got = solver.solve_by_contig(s, e, ids, lengths, M)
        want = mr.oracle_by_contig(oracle, s, e, ids, lengths, M)
        assert np.array_equal(got, want), f"trial {trial}: {n_contigs} contigs, {s.size} reads, M = {M}"
        st = solver.last_stats
        placed = ids != mr.NO_CONTIG
        assert st.n_reads == placed.sum() and st.n_contigs == n_contigs and st.total_length == int(lengths.sum())
        assert st.n_kept == int(np.unpackbits(got.view(np.uint8)).sum())
        assert not np.unpackbits(got.view(np.uint8), bitorder="little")[:s.size][~placed].any()


def test_device_twin_and_the_kept_indices(pkg, oracle, solver):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(7)
    s, e, ids, lengths = mr.random_by_contig(rng, 17, max_reads_per_contig=20_000)
    M = 25
    want = mr.oracle_by_contig(oracle, s, e, ids, lengths, M)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (s, e, ids)]
    d_mask = torch.full((pkg.mask_words(s.size),), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    solver.solve_by_contig_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), s.size, lengths, M,
                                  d_mask.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    got = d_mask.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want)
    # the host entry leaves the input-order mask in the context: the kept index list is the mask's
    got_host = solver.solve_by_contig(s, e, ids, lengths, M)
    assert np.array_equal(got_host, want)


def test_one_contig_already_grouped_equals_solve_host(pkg, solver):
    for seed, (pairs, L, M) in enumerate([(5000, 3000, 100), (125_000, 30_000, 100), (267_000, 800_000, 50)]):
        s, e = pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, seed=seed + 3)
        want = solver.solve(s, e, L, M)
        path = solver.last_stats.path
        got = solver.solve_by_contig(s, e, np.zeros(s.size, np.uint32), [L], M)
        assert np.array_equal(got, want)
        assert solver.last_stats.path == path and solver.last_stats.n_reads == s.size


def test_many_contigs(oracle, solver):
    rng = np.random.default_rng(5000)
    s, e, ids, lengths = mr.random_by_contig(rng, 5200, max_reads_per_contig=120, unplaced=0.01)
    for M in (3, 20):
        got = solver.solve_by_contig(s, e, ids, lengths, M)
        assert np.array_equal(got, mr.oracle_by_contig(oracle, s, e, ids, lengths, M))
        assert solver.last_stats.n_contigs == 5200


def test_a_genome_past_one_calls_position_limit(pkg, solver):
    """GRCh38-like lengths, 3.1 Gbp (one call takes 2^31 - 2 positions), shallow: the mask equals one
    qmcp_hip_solve_host call per contig"""
    grch38_mb = [248, 242, 198, 190, 182, 171, 159, 145, 138, 134, 135, 133, 114, 107, 102, 90, 83, 80, 59, 64, 47,
                 51, 156, 57]
    lengths = np.array([mb * 1_000_000 + 1_234 for mb in grch38_mb] + [16_569], dtype=np.uint32)
    assert int(lengths.sum()) > (1 << 31) - 2
    rng = np.random.default_rng(38)
    ss, ee, ii = [], [], []
    for c, L in enumerate(lengths.tolist()):
        n = max(2, L // 2000)                             # ~0.075 x coverage of 150-base reads, a few deep spots
        s = rng.integers(0, L - 150, size=n)
        hot = rng.random(n) < 0.1
        s[hot] = rng.integers(0, 5000, size=hot.sum())    # (the first 5 kb of every contig is deep)
        ss.append(s)
        ee.append(s + 149)
        ii.append(np.full(n, c))
    s, e, ids = (np.concatenate(x) for x in (ss, ee, ii))
    perm = rng.permutation(s.size)
    s, e, ids = s[perm].astype(np.uint32), e[perm].astype(np.uint32), ids[perm].astype(np.uint32)
    M = 10
    got = solver.solve_by_contig(s, e, ids, lengths, M)
    st = solver.last_stats
    assert st.total_length == int(lengths.sum()) and st.n_contigs == lengths.size
    order, offs = mr.group_stably(ids, lengths.size)
    parts = []
    for c in range(lengths.size):
        idx = order[int(offs[c]):int(offs[c + 1])]
        m = solver.solve(s[idx], e[idx], int(lengths[c]), M)
        bits = np.unpackbits(m.view(np.uint8), bitorder="little")[:idx.size]
        parts.append(idx[bits.astype(bool)])
    want = pkg.indices_to_mask(np.sort(np.concatenate(parts)), s.size)
    assert np.array_equal(got, want)
    assert 0 < st.n_kept < s.size


def test_cfg4_shuffled_across_its_contigs_equals_the_grouped_solve(pkg, solver):
    n_contigs, pairs, L, rl, M = 8, 6_250_000, 1_000_000, 150, 100   # bench.py's cfg4
    ss, ee = [], []
    for c in range(n_contigs):
        s, e = pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, rl, seed=12345 + c)
        ss.append(s)
        ee.append(e)
    s, e = np.concatenate(ss), np.concatenate(ee)
    n = s.size
    offs = np.arange(n_contigs + 1, dtype=np.uint64) * (2 * pairs)
    lengths = np.full(n_contigs, L, dtype=np.uint32)
    grouped = solver.solve(s, e, lengths, M, contig_read_offsets=offs)
    # the contigs' reads interleaved at random, each contig's own reads kept in their order: grouped read k sits at
    # input position where[k]
    ids = np.random.default_rng(4).permutation(np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs))
    where = np.argsort(ids, kind="stable")
    s_in, e_in = np.empty_like(s), np.empty_like(e)
    s_in[where], e_in[where] = s, e
    got = solver.solve_by_contig(s_in, e_in, ids, lengths, M)
    want = np.zeros(n, dtype=bool)
    want[where] = np.unpackbits(grouped.view(np.uint8), bitorder="little")[:n].astype(bool)
    assert np.array_equal(got, np.packbits(want, bitorder="little").view(np.uint64)[:pkg.mask_words(n)])
    assert solver.last_stats.n_kept == int(want.sum()) and solver.last_stats.sweep_stretches >= n_contigs


def test_errors(pkg, solver):
    s = np.array([0, 5, 9], np.uint32)
    e = np.array([3, 8, 9], np.uint32)
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_by_contig(s, e, np.array([0, 2, 0], np.uint32), [10, 10], 2)   # id 2 of 2 contigs
    assert ex.value.code == pkg.QMCP_EINVAL
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_by_contig(s, e, np.array([0, 1, 1], np.uint32), [10, 9], 2)    # end 9 on a 9-position contig
    assert ex.value.code == pkg.QMCP_EREAD
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_by_contig(s, e, np.array([0, 0, 0], np.uint32), [10, 1 << 31], 2)   # one contig past the limit
    assert ex.value.code == pkg.QMCP_ERANGE and "contig 1" in str(ex.value)
    # the sentinel is no error, and an unplaced read is never kept
    got = solver.solve_by_contig(s, e, np.array([0, mr.NO_CONTIG, 0], np.uint32), [10], 2)
    assert pkg.mask_to_indices(got, 3).tolist() == [0, 2]


def test_file_to_file_per_reference(pkg, oracle, tmp_path):
    """downsample_bam(per_reference=True) on a multi-reference file: the written records are the per-reference oracle
    selection followed by the pairing rules (a kept read brings its mate, on whichever reference it lies)"""
    import bam_py
    refs = [("chr1", 30_000), ("chr2", 12_000), ("chr3", 5_000), ("chrM", 1_600)]
    path = tmp_path / "multi.bam"
    header, parsed, ref_lengths = mr.write_multi_reference_bam(path, np.random.default_rng(9), refs, 20_000)
    reads, ids, filtered = mr.expected_per_reference_reads(parsed)
    starts = np.array([r["start"] if i != mr.NO_CONTIG else 0 for r, i in zip(reads, ids)], dtype=np.int64)
    ends = np.array([r["end"] if i != mr.NO_CONTIG else 0 for r, i in zip(reads, ids)], dtype=np.int64)
    M = 15
    out = tmp_path / "out.bam"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True)
    mask = mr.oracle_by_contig(oracle, starts.astype(np.uint32), ends.astype(np.uint32), ids, ref_lengths, M)
    mask = oracle.find_pairs(mask, len(reads))
    bam_ids = np.array([r["bam_id"] for r in reads], dtype=np.int64)
    kept_ids = np.sort(bam_ids[pkg.mask_to_indices(mask, len(reads)).astype(np.int64)])
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == kept_ids.size == len(orecs)
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]
