"""qmcp_hip_solve_quality_*: every mask against quality_model.quality_choice of the oracle's plain mask -- same
coverage and count as the plain solve, the best reads of every (contig, start, end) cell."""
import numpy as np
import pytest
import torch

import amplicon_panels as ap
import bam_py
import multi_reference as mr
import quality_model as qm
import workloads
from forcing import forced

pytestmark = pytest.mark.gpu

CASES = [  # the reference's CoverageTester inputs (coverage_tester.cpp:120-175): kind, pairs, L, M
    (0, 1_000_000, 30_000, 1000), (1, 1_000_000, 30_000, 8000), (2, 1_000_000, 30_000, 8000),
    (3, 1_000_000, 30_000, 8000), (0, 10_000, 3_000, 100),
]


def _check(pkg, oracle, solver, s, e, lengths, M, q, offs=None, info=""):
    got = solver.solve_quality(s, e, q, lengths, M, contig_read_offsets=offs)
    qs = solver.last_quality_stats
    plain = oracle.solve(s, e, lengths, M, contig_read_offsets=offs)
    contig = None if offs is None else qm.contig_of(offs, s.size)
    want = qm.quality_choice(plain, s, e, contig, q)
    assert np.array_equal(got, want), info
    n = s.size
    assert qm.bits_of(got, n).sum() == qm.bits_of(plain, n).sum() == solver.last_stats.n_kept, info
    assert np.array_equal(solver.coverage(s, e, lengths, contig_read_offsets=offs, keep_mask=got),
                          solver.coverage(s, e, lengths, contig_read_offsets=offs, keep_mask=plain)), info
    return got, plain, qs


@pytest.mark.parametrize("kind,pairs,L,M", CASES)
def test_equal_qualities_give_the_plain_mask(pkg, solver, kind, pairs, L, M):
    s, e = pkg.reads_gen(kind, pairs, L)
    plain = solver.solve(s, e, L, M)
    got = solver.solve_quality(s, e, np.full(s.size, 37, np.uint32), L, M)
    assert np.array_equal(got, plain)
    qs = solver.last_quality_stats
    assert qs.sort_passes == 0 and qs.quality_min == qs.quality_max == 37 and qs.reads_swapped == 0


def test_equal_qualities_on_cfg2(pkg, solver):
    s, e = pkg.reads_gen(0, 500_000, 1_000_000)
    plain = solver.solve(s, e, 1_000_000, 100)
    assert np.array_equal(solver.solve_quality(s, e, np.zeros(s.size, np.uint32), 1_000_000, 100), plain)
    assert solver.last_quality_stats.sort_passes == 0


@pytest.mark.parametrize("kind,pairs,L,M", CASES)
def test_reads_gen_qualities_equal_the_model(pkg, oracle, solver, kind, pairs, L, M):
    s, e, q = pkg.reads_gen(kind, pairs, L, with_qualities=True)
    assert q.min() < q.max()
    _, plain, qs = _check(pkg, oracle, solver, s, e, L, M, q)
    assert qs.sort_passes >= 1 and qs.cells_contested > 0 and qs.reads_swapped > 0


def test_mixed_spans_and_cut_points(pkg, oracle, solver):
    rng = np.random.default_rng(5)
    s, e, q = pkg.reads_gen(0, 300_000, 60_000, with_qualities=True)
    offs = np.array([0, s.size], np.uint64)
    cs, ce = workloads.clipped_mix(s, e, 0.01)
    _check(pkg, oracle, solver, cs, ce, 60_000, 100, q, info="1 % clipped")
    le = workloads.lengthened_mix(cs, ce, offs, np.array([60_000], np.uint32), 0.005)
    _check(pkg, oracle, solver, cs, le, 60_000, 100, q, info="and 0.5 % lengthened")
    # shallow data: coverage around M, split at cut points
    s2, e2 = pkg.reads_gen(0, 40_000, 2_000_000, seed=3)
    _check(pkg, oracle, solver, s2, e2, 2_000_000, 8, rng.integers(0, 61, size=s2.size).astype(np.uint32),
           info="shallow")


def test_amplicon_shape_with_huge_cells(pkg, oracle, solver):
    # cfg3's shape: reads run from primer to primer, so a cell holds > 10^5 reads
    rng = np.random.default_rng(8)
    a0, a1 = workloads.amplicon_panel()
    k = a0.size
    n_pairs = 12_000_000
    amp = rng.integers(0, k, size=n_pairs)
    s = np.empty(2 * n_pairs, np.uint32)
    e = np.empty(2 * n_pairs, np.uint32)
    s[0::2], e[0::2] = a0[amp] + 25, a0[amp] + 174
    s[1::2], e[1::2] = a1[amp] - 174, a1[amp] - 25
    q = rng.integers(0, 61, size=s.size).astype(np.uint32)
    assert np.bincount(amp).max() > 10 ** 5
    got, plain, qs = _check(pkg, oracle, solver, s, e, 29_903, 200, q)
    assert qs.cells_contested > 0


def test_every_route_gives_the_same_mask(pkg, oracle, solver):
    s, e, q = pkg.reads_gen(0, 150_000, 40_000, with_qualities=True)
    cs, ce = workloads.clipped_mix(s, e, 0.01)
    want = None
    for cols in ((s, e), (cs, ce)):
        for env in ({}, dict(QMCP_HIP_PM="1"), dict(QMCP_HIP_PM="0"), dict(QMCP_HIP_NO_RANK="1"),
                    dict(QMCP_HIP_SWEEP="fast"), dict(QMCP_HIP_SWEEP="gen"), dict(QMCP_HIP_SWEEP="ev"),
                    dict(QMCP_HIP_SPEC="1"), dict(QMCP_HIP_SPEC="0"), dict(QMCP_HIP_NEAR="0")):
            with forced(solver, **env):
                got = solver.solve_quality(cols[0], cols[1], q, 40_000, 100)
            if not env:
                want = qm.quality_choice(oracle.solve(cols[0], cols[1], 40_000, 100), cols[0], cols[1], None, q)
            assert np.array_equal(got, want), env


def test_keys_wider_than_32_bits_and_errors(pkg, oracle, solver):
    rng = np.random.default_rng(11)
    L = 1 << 27
    lengths = np.array([L, L], np.uint32)
    n = 6000
    hot = rng.integers(0, L - 400, size=40)                    # a few positions deep enough to be contested
    s = hot[rng.integers(0, hot.size, size=n)] + rng.integers(0, 3, size=n)
    span = rng.choice([100, 150], size=n)
    e = s + span - 1
    offs = np.array([0, n // 2, n], np.uint64)
    q = rng.integers(0, 50_001, size=n).astype(np.uint32)
    got, plain, qs = _check(pkg, oracle, solver, s.astype(np.uint32), e.astype(np.uint32), lengths, 5, q, offs)
    assert qs.key_bits > 32 and qs.sort_passes == (qs.key_bits + 7) // 8 and qs.reads_swapped > 0
    q2 = q.copy()
    q2[0], q2[1] = 0, 65_536
    with pytest.raises(pkg.QmcpError) as err:
        solver.solve_quality(s, e, q2, lengths, 5, contig_read_offsets=offs)
    assert err.value.code == pkg.QMCP_ERANGE
    with pytest.raises(pkg.QmcpError) as err:
        solver.solve_quality(s, e, None, lengths, 5, contig_read_offsets=offs)
    assert err.value.code == pkg.QMCP_EINVAL
    # the range is checked before the solve: a caller's device mask is left as it was
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to("cuda:0")
    ds, de, dq2 = dev(s), dev(e), dev(q2)
    dm = torch.full((pkg.mask_words(n),), 0x5A5A, dtype=torch.int64, device="cuda:0")
    with pytest.raises(pkg.QmcpError) as err:
        solver.solve_quality_device(ds.data_ptr(), de.data_ptr(), dq2.data_ptr(), n, lengths, 5, dm.data_ptr(),
                                    contig_read_offsets=offs)
    assert err.value.code == pkg.QMCP_ERANGE
    assert bool((dm == 0x5A5A).all())
    # the context is usable afterwards
    assert np.array_equal(solver.solve_quality(s, e, q, lengths, 5, contig_read_offsets=offs), got)


def test_device_entry_on_a_caller_stream_and_pairs_completed_by_the_adapter(pkg, oracle, solver):
    s, e, q = pkg.reads_gen(2, 200_000, 50_000, with_qualities=True)
    want = solver.solve_quality(s, e, q, 50_000, 300)
    assert np.array_equal(want, qm.quality_choice(oracle.solve(s, e, 50_000, 300), s, e, None, q))
    n = s.size
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):       # the columns are produced on the caller's stream, the entry orders after it
        ds = torch.from_numpy(s.astype(np.int32)).to("cuda:0", non_blocking=False)
        de = torch.from_numpy(e.astype(np.int32)).to("cuda:0")
        dq = torch.from_numpy(q.astype(np.int32)).to("cuda:0")
        dm = torch.full((pkg.mask_words(n),), -1, dtype=torch.int64, device="cuda:0")
    qs = solver.solve_quality_device(ds.data_ptr(), de.data_ptr(), dq.data_ptr(), n, 50_000, 300, dm.data_ptr(),
                                     stream=side.cuda_stream)
    got = dm.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want) and qs.reads_swapped > 0
    # QuasiMcpHipQualitySolver with complete_pairs: the quality mask, then the mates on the device
    kept = pkg.host_solve("quasi-mcp-hip-quality", s, e, 50_000, 300, qualities=q, adapter_pairs=True)
    assert np.array_equal(kept, pkg.mask_to_indices(oracle.find_pairs(want, n), n))


def test_by_contig_with_shuffled_contigs_and_unplaced_reads(pkg, oracle, solver):
    rng = np.random.default_rng(77)
    for trial in range(6):
        s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(1, 30)))
        q = rng.integers(0, 61, size=s.size).astype(np.uint32)
        M = int(rng.integers(2, 30))
        got = solver.solve_quality_by_contig(s, e, ids, q, lengths, M)
        plain = mr.oracle_by_contig(oracle, s, e, ids, lengths, M)
        want = qm.quality_choice(plain, s, e, ids, q)
        assert np.array_equal(got, want), f"trial {trial}"
        assert not qm.bits_of(got, s.size)[ids == mr.NO_CONTIG].any()
        assert np.array_equal(solver.solve_by_contig(s, e, ids, lengths, M), plain)


def test_cfg4_full_size(pkg, oracle, solver):
    pairs, L, M = 6_250_000, 1_000_000, 100
    ss, ee = zip(*[pkg.reads_gen(0, pairs, L, seed=12345 + c) for c in range(8)])
    s, e = np.concatenate(ss), np.concatenate(ee)
    offs = np.arange(9, dtype=np.uint64) * np.uint64(2 * pairs)
    lengths = np.full(8, L, np.uint32)
    q = np.random.default_rng(60).integers(0, 61, size=s.size).astype(np.uint32)
    solver.solve_quality(s, e, q, lengths, M, contig_read_offsets=offs)            # (arena grown)
    got = solver.solve_quality(s, e, q, lengths, M, contig_read_offsets=offs)
    qs, st = solver.last_quality_stats, solver.last_stats
    print(f"\ncfg4 quality pass {qs.ms_quality:.3f} ms (plain solve {st.ms_total:.3f} ms), {qs.as_dict()}")
    assert qs.key_bits == 29 and qs.sort_passes == 4
    assert qs.ms_quality <= 8 * st.ms_total
    plain = oracle.solve(s, e, lengths, M, contig_read_offsets=offs)
    n_c = 2 * pairs
    gb, pb = qm.bits_of(got, s.size), qm.bits_of(plain, s.size)
    for c in range(8):
        sl = slice(c * n_c, (c + 1) * n_c)
        want = qm.quality_choice(qm.mask_of(pb[sl]), s[sl], e[sl], None, q[sl])
        assert np.array_equal(qm.mask_of(gb[sl]), want), f"contig {c}"


def test_plugin_and_file_flow_with_grade(pkg, oracle, solver, tmp_path):
    s, e, q = pkg.reads_gen(0, 20_000, 5_000, with_qualities=True)
    kept = pkg.host_solve("quasi-mcp-hip-quality", s, e, 5_000, 50, qualities=q)
    want = qm.quality_choice(oracle.solve(s, e, 5_000, 50), s, e, None, q)
    assert np.array_equal(kept, pkg.mask_to_indices(want, s.size))
    with pytest.raises(KeyError):
        pkg.host_solve("quasi-mcp-hip-qualityx", s, e, 5_000, 50, qualities=q)

    refs = ap.INFLUENZA
    names = [n for n, _ in refs]
    panel = ap.segment_panel(refs[:7], per_ref=12)
    path = tmp_path / "flu.bam"
    header, parsed, ref_lengths = ap.write_panel_bam(path, np.random.default_rng(41), refs, panel, 20_000)
    bed, tsv = tmp_path / "flu.bed", tmp_path / "flu.tsv"
    ap.write_panel_files(panel, bed, tsv)
    offs, a0, a1 = ap.panel_csr(panel, names)
    M = 40
    out = tmp_path / "out.bam"
    written = pkg.downsample_bam("quasi-mcp-hip-quality", path, out, M, per_reference=True, bed=bed, tsv=tsv,
                                 amplicons_by_reference=True)
    cols = pkg.read_bam(path, bed=bed, tsv=tsv, amplicon_mode=2, per_reference=True, amplicons_by_reference=True)
    # GRADE restated: quality - min + (max - min if the pair sits in one amplicon of its own reference)
    reads, _ = bam_py.pair_like_the_reference(parsed)
    inside = ap.inside_by_reference(parsed, offs, a0, a1)
    qs_ = [r["q"] for r in reads]
    lo, hi = min(qs_), max(qs_)
    grades = [x - lo + ((hi - lo) if inside(reads[i - i % 2], reads[i - i % 2 + 1]) else 0) for i, x in enumerate(qs_)]
    assert cols["qualities"].tolist() == grades
    assert cols["bam_ids"].tolist() == [r["bam_id"] for r in reads]
    # cross-amplicon pairs are in the input: GRADE, not FILTER, was chosen
    assert any(not inside(reads[2 * k], reads[2 * k + 1]) for k in range(len(reads) // 2))
    n = cols["starts"].size
    plain = mr.oracle_by_contig(oracle, cols["starts"], cols["ends"], cols["contig_ids"], ref_lengths, M)
    chosen = qm.quality_choice(plain, cols["starts"], cols["ends"], cols["contig_ids"], cols["qualities"])
    mask = oracle.find_pairs(chosen, n)
    kept_ids = np.sort(cols["bam_ids"][pkg.mask_to_indices(mask, n).astype(np.int64)].astype(np.int64))
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == kept_ids.size == len(orecs) > 0
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]
    # the plain solver on the same files still filters
    out2 = tmp_path / "out2.bam"
    w2 = pkg.downsample_bam("quasi-mcp-hip", path, out2, M, per_reference=True, bed=bed, tsv=tsv,
                            amplicons_by_reference=True)
    w1 = pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "out1.bam", M, per_reference=True, bed=bed, tsv=tsv,
                            amplicons_by_reference=True, amplicon_mode=1)
    assert w2 == w1
