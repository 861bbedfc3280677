"""qmcp_hip_filter_solve_by_contig_host: pairs of several references, FILTERed against the amplicons of each read's own
reference, solved per reference, mates completed, the mask in input order.  Every mask is compared bit for bit with
the composed oracle (oracle.amplicon_filter per contig on its same-contig pairs -> multi_reference.oracle_by_contig on
the survivors -> oracle.find_pairs -> input order), with qmcp_hip_filter_solve_host on one contig, and with the
per-reference file-to-file flow."""
import numpy as np
import pytest

import amplicon_panels as ap
import multi_reference as mr
import workloads

pytestmark = pytest.mark.gpu


def random_amplicons(rng, lengths):
    """per contig: none (some contigs), a tiled panel, or amplicons drawn at random (unsorted, nested, duplicated)"""
    offs, a0, a1 = [0], [], []
    for L in lengths.tolist():
        kind = rng.random()
        if kind < 0.2:
            pass
        elif kind < 0.6:
            size = int(rng.integers(200, min(600, L) + 1))
            step = int(rng.integers(size // 2, size + 1))
            for s in range(0, L - size + 1, step):
                a0.append(s)
                a1.append(s + size - 1)
        else:
            k = int(rng.integers(1, 60))
            s = rng.integers(0, L - 200, size=k)
            e = np.minimum(s + rng.integers(150, 800, size=k), L - 1)
            if k > 2:
                s[1], e[1] = s[0], e[0]                          # a duplicate
            a0 += s.tolist()
            a1 += e.tolist()
        offs.append(len(a0))
    return np.array(offs, np.uint32), np.array(a0, np.uint32), np.array(a1, np.uint32)


def test_random_multi_contig_inputs_equal_the_composed_oracle(pkg, oracle, solver):
    rng = np.random.default_rng(355)
    for trial in range(24):
        n_contigs = int(rng.integers(1, 41))
        lengths = rng.integers(400, 20_000, size=n_contigs).astype(np.uint32)
        offs, a0, a1 = random_amplicons(rng, lengths)
        n_pairs = int(rng.integers(1000, 30_000))
        s, e, ids = ap.panel_pairs(rng, lengths, offs, a0, a1, n_pairs, straddle=0.1, cross=0.05, unplaced=0.02)
        M = int(rng.integers(1, 40))
        pairs = bool(trial % 2)
        ignore = trial % 6 == 5
        filt = {}
        if trial % 3:
            filt = dict(seq_lengths=rng.integers(60, 151, size=s.size).astype(np.uint32),
                        qualities=rng.integers(0, 61, size=s.size).astype(np.uint32), min_length=90, min_mapq=20)
        amp = {} if ignore else dict(amp_offsets=offs, amp_starts=a0, amp_ends=a1)
        got, dropped = solver.filter_solve_by_contig(s, e, ids, lengths, M, complete_pairs=pairs, **amp, **filt)
        want, want_dropped = ap.oracle_filter_by_contig(oracle, pkg, s, e, ids, lengths, None if ignore else offs, a0,
                                                        a1, M, complete_pairs=pairs, **filt)
        info = f"trial {trial}: {n_contigs} contigs, {n_pairs} pairs, M = {M}, pairs {pairs}, ignore {ignore}"
        assert dropped == want_dropped, info
        assert np.array_equal(got, want), info
        assert 0 < dropped < n_pairs or ignore, info
        st = solver.last_stats
        assert st.n_contigs == n_contigs and st.total_length == int(lengths.sum())


def test_cfg3_full_size_one_contig_equals_filter_solve(pkg, solver):
    n_pairs = 15_000_000
    s, e, a0, a1, straddle = workloads.amplicon_reads(n_pairs)
    want, want_dropped = solver.filter_solve(s, e, 29_903, 200, amp_starts=a0, amp_ends=a1, complete_pairs=True)
    got, dropped = solver.filter_solve_by_contig(s, e, np.zeros(s.size, np.uint32), [29_903], 200,
                                                 amp_offsets=[0, a0.size], amp_starts=a0, amp_ends=a1,
                                                 complete_pairs=True)
    assert dropped == want_dropped and dropped >= int(straddle.sum())
    assert np.array_equal(got, want)


def test_multi_reference_panel_at_cfg3_size(pkg, oracle, solver):
    """eight influenza-like segments (13.6 kb), 25 amplicons each, 15 M pairs: a tenth straddles two amplicons, about
    1 % has its mates on two segments; M = 200"""
    refs = ap.INFLUENZA
    names = [n for n, _ in refs]
    lengths = np.array([L for _, L in refs], np.uint32)
    offs, a0, a1 = ap.panel_csr(ap.segment_panel(refs), names)
    rng = np.random.default_rng(2009)
    s, e, ids = ap.panel_pairs(rng, lengths, offs, a0, a1, 15_000_000, straddle=0.10, cross=0.01)
    got, dropped = solver.filter_solve_by_contig(s, e, ids, lengths, 200, amp_offsets=offs, amp_starts=a0,
                                                 amp_ends=a1, complete_pairs=True)
    want, want_dropped = ap.oracle_filter_by_contig(oracle, pkg, s, e, ids, lengths, offs, a0, a1, 200,
                                                    complete_pairs=True)
    assert dropped == want_dropped and np.array_equal(got, want)
    assert solver.last_stats.n_contigs == len(refs) and solver.last_stats.n_kept > 0
    # IGNORE: solve_by_contig + mate completion on the length / MAPQ survivors
    lens = rng.integers(60, 151, size=s.size).astype(np.uint32)
    mapq = rng.integers(0, 61, size=s.size).astype(np.uint32)
    got, dropped = solver.filter_solve_by_contig(s, e, ids, lengths, 200, seq_lengths=lens, qualities=mapq,
                                                 min_length=90, min_mapq=20, complete_pairs=True)
    keep = ((lens[0::2] >= 90) & (lens[1::2] >= 90) & (mapq[0::2] >= 20) & (mapq[1::2] >= 20))
    sel = np.repeat(keep, 2)
    orig = np.flatnonzero(sel)
    m = solver.solve_by_contig(s[sel], e[sel], ids[sel], lengths, 200)
    m = solver.complete_pairs(m, orig.size)
    want = pkg.indices_to_mask(orig[pkg.mask_to_indices(m, orig.size).astype(np.int64)], s.size)
    assert dropped == int((~keep).sum()) and np.array_equal(got, want)


def test_errors_and_recovery(pkg, oracle, solver):
    rng = np.random.default_rng(12)
    lengths = np.array([3000, 2000], np.uint32)
    offs, a0, a1 = ap.panel_csr(ap.tiled_panel([("a", 3000), ("b", 2000)], 20), ["a", "b"])
    s, e, ids = ap.panel_pairs(rng, lengths, offs, a0, a1, 5000, cross=0.05)
    amp = dict(amp_offsets=offs, amp_starts=a0, amp_ends=a1)
    want, _ = ap.oracle_filter_by_contig(oracle, pkg, s, e, ids, lengths, offs, a0, a1, 10, complete_pairs=True)

    def good_call():
        got, _ = solver.filter_solve_by_contig(s, e, ids, lengths, 10, complete_pairs=True, **amp)
        assert np.array_equal(got, want)

    good_call()
    with pytest.raises(pkg.QmcpError) as ex:                        # odd n_reads
        solver.filter_solve_by_contig(s[:-1], e[:-1], ids[:-1], lengths, 10, **amp)
    assert ex.value.code == pkg.QMCP_EINVAL
    good_call()
    # a pair the FILTER drops (mates on two contigs) still has its reads checked
    q = int(np.flatnonzero(ids[0::2] != ids[1::2])[0])
    bad_ids = ids.copy()
    bad_ids[2 * q + 1] = 7                                          # id 7 of 2 contigs
    with pytest.raises(pkg.QmcpError) as ex:
        solver.filter_solve_by_contig(s, e, bad_ids, lengths, 10, **amp)
    assert ex.value.code == pkg.QMCP_EINVAL
    good_call()
    bad_e = e.copy()
    bad_e[2 * q] = lengths[ids[2 * q]]                              # one past its contig's end
    with pytest.raises(pkg.QmcpError) as ex:
        solver.filter_solve_by_contig(s, bad_e, ids, lengths, 10, **amp)
    assert ex.value.code == pkg.QMCP_EREAD
    good_call()
    for bad_offs in ([1, offs[1], offs[2]], [0, offs[2], offs[1]]):  # not from 0; decreasing
        with pytest.raises(pkg.QmcpError) as ex:
            solver.filter_solve_by_contig(s, e, ids, lengths, 10, amp_offsets=np.array(bad_offs, np.uint32),
                                          amp_starts=a0, amp_ends=a1)
        assert ex.value.code == pkg.QMCP_EINVAL
        good_call()
    # the mask of the last call stays in the context
    n = s.size
    assert np.array_equal(pkg.mask_to_indices(want, n), pkg.mask_to_indices(solver.filter_solve_by_contig(
        s, e, ids, lengths, 10, complete_pairs=True, **amp)[0], n))


def test_file_to_file_with_amplicons_by_reference(pkg, oracle, solver, tmp_path):
    import bam_py
    refs = ap.INFLUENZA
    names = [n for n, _ in refs]
    panel = ap.segment_panel(refs[:7], per_ref=12)                 # NS has no amplicons
    path = tmp_path / "flu.bam"
    header, parsed, ref_lengths = ap.write_panel_bam(path, np.random.default_rng(31), refs, panel, 20_000)
    bed, tsv = tmp_path / "flu.bed", tmp_path / "flu.tsv"
    ap.write_panel_files(panel, bed, tsv)
    offs, a0, a1 = ap.panel_csr(panel, names)
    M = 40
    out = tmp_path / "out.bam"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, bed=bed, tsv=tsv,
                                 amplicons_by_reference=True)
    # the per-reference oracle selection after pairing
    reads, _ = bam_py.pair_like_the_reference(parsed, inside=ap.inside_by_reference(parsed, offs, a0, a1))
    ids = np.array([parsed[r["bam_id"]]["ref_id"] for r in reads], np.uint32)
    starts = np.array([r["start"] for r in reads], np.uint32)
    ends = np.array([r["end"] for r in reads], np.uint32)
    mask = oracle.find_pairs(mr.oracle_by_contig(oracle, starts, ends, ids, ref_lengths, M), len(reads))
    bam_ids = np.array([r["bam_id"] for r in reads], dtype=np.int64)
    kept_ids = np.sort(bam_ids[pkg.mask_to_indices(mask, len(reads)).astype(np.int64)])
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == kept_ids.size == len(orecs) > 0
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]
    # the column path: unfiltered per-reference columns, the amplicons from the files, the device FILTER
    cols = pkg.read_bam(path, per_reference=True)
    ref_names = pkg.reference_names(path)
    assert ref_names == names
    c_offs, c0, c1 = pkg.amplicons_by_reference(bed, tsv, ref_names)
    got, _ = solver.filter_solve_by_contig(
        cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"], M, amp_offsets=c_offs,
        amp_starts=c0, amp_ends=c1, complete_pairs=True)
    col_ids = np.sort(cols["bam_ids"][pkg.mask_to_indices(got, cols["starts"].size).astype(np.int64)])
    assert np.array_equal(col_ids.astype(np.int64), kept_ids)
