"""qmcp_hip_solve_targets_*: every mask bit for bit against "project with tests/target_model.py, solve each contig's
projected on-target reads in input order with the oracle, map back"; identity cases, validity on the original axis, the
quality pass on the projected problem, errors, the file flow, determinism, and the time of the pre- / post-pass against
the grouping stages of the plain by-contig solve."""
import json
import os
import statistics

import numpy as np
import pytest
import torch

import multi_reference as mr
import quality_model as qm
import target_model as tm

pytestmark = pytest.mark.gpu

NO_CONTIG = 0xFFFFFFFF
GROUPING = ("k_bc_keys", "k_radix_hist_rec(by contig)", "scan_radix_hist(by contig, 3 kernels)",
            "k_radix_scatter_rec(by contig)", "k_bc_bounds", "k_bc_gather")
TARGET_STAGES = ("k_target_project", "count targets(2 x popcounts, scan)", "k_compact_reads", "k_expand_mask_reads",
                 "k_or_words(off-target reads)")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")


def _solve_device(pkg, solver, s, e, ids, lengths, M, offs, t0, t1, q=None, offset=0, **kw):
    """through the _device entry; offset > 0 shifts the columns off 16-byte alignment (the 32-bit load path)"""
    n = s.size
    pad = np.zeros(offset, np.uint32)
    ds, de, di = (_dev(np.concatenate([pad, x])) for x in (s, e, ids))
    dq = None if q is None else _dev(np.concatenate([pad, q]))
    d_mask = torch.full((max(pkg.mask_words(n), 1),), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr() + 4 * offset
    ts = solver.solve_targets_device(ptr(ds), ptr(de), ptr(di), n, lengths, M, offs, t0, t1, d_mask.data_ptr(),
                                     d_qualities=0 if dq is None else ptr(dq), **kw)
    torch.cuda.synchronize()
    return d_mask.cpu().numpy().view(np.uint64)[:pkg.mask_words(n)].copy(), ts


def _check_validity(pkg, oracle, got, on, s, e, ids, lengths, offs, t0, t1, M, padding):
    """at every target position of the original axis, cover(kept) >= min(cover(all), M); off-target reads not kept"""
    n = s.size
    bits = qm.bits_of(got, n)
    assert not np.any(bits & ~on)
    sets = tm.target_sets(lengths, offs, t0, t1, padding)
    for c, tset in enumerate(sets):
        sel = np.flatnonzero(ids == c)
        if sel.size == 0 or not tset.any():
            continue
        L = int(lengths[c])
        cov_all = oracle.cover(s[sel], e[sel], L)
        cov_kept = oracle.cover(s[sel], e[sel], L, keep_mask=qm.mask_of(bits[sel]))
        assert np.all(cov_kept[tset] >= np.minimum(cov_all[tset], M)), c


def test_random_calls_equal_the_model_and_the_oracle(pkg, oracle, solver):
    seen_empty_target_contig = seen_unplaced = seen_clipped = 0
    for seed in range(64):
        rng = np.random.default_rng(1000 + seed)
        s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(1, 7)), max_reads_per_contig=2500)
        offs, t0, t1 = tm.random_regions(rng, lengths, max_regions=6, max_len=700)
        padding = int(rng.choice([0, 0, 30]))
        M = int(rng.choice([1, 3, 50]))
        want, on = tm.expected_mask(oracle, s, e, ids, lengths, offs, t0, t1, M, padding=padding)
        got = solver.solve_targets(s, e, ids, lengths, M, offs, t0, t1, padding=padding)
        info = f"seed {seed}"
        assert np.array_equal(got, want), info
        ts = solver.last_target_stats
        placed = ids != NO_CONTIG
        assert ts.reads_on_target == int(on.sum()) and ts.reads_off_target == int((placed & ~on).sum()), info
        sets = tm.target_sets(lengths, offs, t0, t1, padding)
        assert ts.target_positions == sum(int(t.sum()) for t in sets), info
        assert ts.regions_in == t0.size and ts.regions_merged == sum(len(tm.merged_regions(t)) for t in sets), info
        assert solver.last_stats.n_kept == int(qm.bits_of(got, s.size).sum()), info     # the oracle's on-target count
        _check_validity(pkg, oracle, got, on, s, e, ids, lengths, offs, t0, t1, M, padding)
        if seed % 4 == 0:    # the same call through the device entry, aligned and not
            for offset in (0, 1):
                got_d, _ = _solve_device(pkg, solver, s, e, ids, lengths, M, offs, t0, t1, padding=padding, offset=offset)
                assert np.array_equal(got_d, want), (info, offset)
        seen_empty_target_contig += int(any(not t.any() for t in sets))
        seen_unplaced += int((~placed).any())
        _, ps, pe, _ = tm.project(s, e, ids, lengths, offs, t0, t1, padding)
        seen_clipped += int(np.any(on & (pe - ps < e.astype(np.int64) - s)))
    assert seen_empty_target_contig > 5 and seen_unplaced > 30 and seen_clipped > 30


def _tiled_regions(rng, L, region_len_lo, region_len_hi, share):
    """regions of region_len_lo..hi at about `share` of the positions, ascending, disjoint"""
    t0, t1, p = [], [], 0
    mean = (region_len_lo + region_len_hi) / 2
    gap = mean * (1 - share) / share
    while True:
        p += int(rng.integers(int(gap * 0.5), int(gap * 1.5) + 1))
        ln = int(rng.integers(region_len_lo, region_len_hi + 1))
        if p + ln >= L:
            break
        t0.append(p)
        t1.append(p + ln - 1)
        p += ln
    return np.array(t0, np.uint32), np.array(t1, np.uint32)


def _one_length_case(pkg, rng, n_contigs, pairs, L, region_lo, region_hi, share):
    ss, ee, ii, t0s, t1s, offs = [], [], [], [], [], [0]
    for c in range(n_contigs):
        s, e = pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, 150, seed=77 + c)
        ss.append(s)
        ee.append(e)
        ii.append(np.full(s.size, c, np.uint32))
        a, b = _tiled_regions(rng, L, region_lo, region_hi, share)
        t0s.append(a)
        t1s.append(b)
        offs.append(offs[-1] + a.size)
    s, e, ids = np.concatenate(ss), np.concatenate(ee), np.concatenate(ii)
    perm = rng.permutation(s.size)
    return (s[perm], e[perm], ids[perm], np.full(n_contigs, L, np.uint32), np.array(offs, np.uint32),
            np.concatenate(t0s), np.concatenate(t1s))


LARGE = {
    # one read length, exome-like regions (1-3 read lengths at a tenth of the positions), > 10^6 reads; the table fits LDS
    "exome_lds": dict(n_contigs=2, pairs=300_000, L=1_500_000, region_lo=150, region_hi=450, share=0.1, M=20),
    # the same shape with > 4 096 merged regions: the table is read through global memory
    "exome_global": dict(n_contigs=3, pairs=250_000, L=6_000_000, region_lo=150, region_hi=450, share=0.1, M=3),
    # regions far longer than a read: a few per cent of the on-target reads are clipped (the near-uniform shape)
    "long_regions": dict(n_contigs=2, pairs=300_000, L=1_000_000, region_lo=15_000, region_hi=25_000, share=0.5, M=30),
}


@pytest.mark.parametrize("name", list(LARGE))
def test_large_one_length_cases(pkg, oracle, solver, name):
    cfg = dict(LARGE[name])
    M = cfg.pop("M")
    s, e, ids, lengths, offs, t0, t1 = _one_length_case(pkg, np.random.default_rng(5), **cfg)
    assert s.size >= 1_000_000
    want, on = tm.expected_mask(oracle, s, e, ids, lengths, offs, t0, t1, M)
    got = solver.solve_targets(s, e, ids, lengths, M, offs, t0, t1)
    assert np.array_equal(got, want)
    ts = solver.last_target_stats
    assert ts.reads_on_target == int(on.sum()) and (ts.regions_merged > 4096) == (name == "exome_global")
    if name == "long_regions":
        _, ps, pe, _ = tm.project(s, e, ids, lengths, offs, t0, t1)
        clipped = np.count_nonzero(on & (pe - ps < 149)) / max(int(on.sum()), 1)
        assert 0.005 < clipped < 0.08
    for offset in (0, 3):
        got_d, ts_d = _solve_device(pkg, solver, s, e, ids, lengths, M, offs, t0, t1, offset=offset)
        assert np.array_equal(got_d, want), offset
        assert ts_d.reads_on_target == ts.reads_on_target
    # determinism: the same call again gives the same mask
    assert np.array_equal(solver.solve_targets(s, e, ids, lengths, M, offs, t0, t1), got)
    _check_validity(pkg, oracle, got, on, s, e, ids, lengths, offs, t0, t1, M, 0)


def test_identity_cases(pkg, oracle, solver):
    rng = np.random.default_rng(9)
    s, e, ids, lengths = mr.random_by_contig(rng, 5, max_reads_per_contig=4000)
    n = s.size
    M = 7
    plain = solver.solve_by_contig(s, e, ids, lengths, M)
    # one region covering each whole contig (once exactly, once by padding and clipping)
    whole_offs = np.arange(lengths.size + 1, dtype=np.uint32)
    zeros = np.zeros(lengths.size, np.uint32)
    assert np.array_equal(solver.solve_targets(s, e, ids, lengths, M, whole_offs, zeros, lengths - 1), plain)
    assert solver.last_target_stats.reads_off_target == 0
    assert np.array_equal(solver.solve_targets(s, e, ids, lengths, M, whole_offs, zeros, zeros, padding=1 << 20), plain)
    # no region: nothing kept; with the flag, every placed read
    none = np.zeros(lengths.size + 1, np.uint32)
    empty = np.zeros(0, np.uint32)
    assert not solver.solve_targets(s, e, ids, lengths, M, none, empty, empty).any()
    assert not solver.solve_targets(s, e, ids, lengths, M, none, None, None).any()
    everything = solver.solve_targets(s, e, ids, lengths, M, none, empty, empty, keep_off_target=True)
    assert np.array_equal(qm.bits_of(everything, n), ids != NO_CONTIG)
    # KEEP_OFF_TARGET == the plain result OR every placed off-target read
    offs, t0, t1 = tm.random_regions(rng, lengths, max_regions=4, max_len=900, empty=0.3)
    base = solver.solve_targets(s, e, ids, lengths, M, offs, t0, t1, padding=10)
    want, on = tm.expected_mask(oracle, s, e, ids, lengths, offs, t0, t1, M, padding=10)
    assert np.array_equal(base, want)
    both = solver.solve_targets(s, e, ids, lengths, M, offs, t0, t1, padding=10, keep_off_target=True)
    assert np.array_equal(qm.bits_of(both, n), qm.bits_of(base, n) | ((ids != NO_CONTIG) & ~on))
    assert np.array_equal(both, tm.expected_mask(oracle, s, e, ids, lengths, offs, t0, t1, M, padding=10,
                                                 keep_off_target=True)[0])
    # the host entry leaves the mask in the context: completing pairs there equals completing them on the oracle
    if n % 2 == 0:
        assert np.array_equal(solver.complete_pairs(both, n), oracle.find_pairs(both, n))
    # no read at all
    assert solver.solve_targets(empty, empty, empty, lengths, M, offs, t0, t1).size == 0


def test_quality_pass_on_the_projected_problem(pkg, oracle, solver):
    contested = 0
    for seed in range(12):
        rng = np.random.default_rng(400 + seed)
        s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(1, 5)), max_reads_per_contig=3000)
        # short regions: many reads share a projected interval although their own intervals differ
        offs, t0, t1 = tm.random_regions(rng, lengths, max_regions=8, max_len=60, empty=0.1)
        q = rng.integers(0, 61, size=s.size).astype(np.uint32)
        M = int(rng.choice([2, 10]))
        want, _ = tm.expected_mask(oracle, s, e, ids, lengths, offs, t0, t1, M, qualities=q,
                                   quality_choice=qm.quality_choice)
        got = solver.solve_targets(s, e, ids, lengths, M, offs, t0, t1, qualities=q)
        assert np.array_equal(got, want), seed
        no_quality = solver.solve_targets(s, e, ids, lengths, M, offs, t0, t1)
        contested += int(not np.array_equal(got, no_quality))
        assert qm.bits_of(got, s.size).sum() == qm.bits_of(no_quality, s.size).sum()
        equal = solver.solve_targets(s, e, ids, lengths, M, offs, t0, t1, qualities=np.full(s.size, 31, np.uint32))
        assert np.array_equal(equal, no_quality), seed
        if seed % 4 == 0:
            got_d, _ = _solve_device(pkg, solver, s, e, ids, lengths, M, offs, t0, t1, q=q)
            assert np.array_equal(got_d, want), seed
    assert contested >= 8


def test_errors_and_recovery(pkg, oracle, solver):
    rng = np.random.default_rng(12)
    s, e, ids, lengths = mr.random_by_contig(rng, 3, max_reads_per_contig=3000, unplaced=0.02)
    lengths = lengths.copy()
    offs = np.array([0, 1, 2, 2], np.uint32)
    t0 = np.array([50, 20], np.uint32)
    t1 = np.array([120, 90], np.uint32)
    M = 5
    want, on = tm.expected_mask(oracle, s, e, ids, lengths, offs, t0, t1, M)
    placed = ids != NO_CONTIG
    assert on.any() and (placed & ~on).any()

    def good_call():
        assert np.array_equal(solver.solve_targets(s, e, ids, lengths, M, offs, t0, t1), want)

    def fails(code, **kw):
        args = dict(starts=s, ends=e, contig_ids=ids, contig_lengths=lengths, max_coverage=M, target_offsets=offs,
                    target_starts=t0, target_ends=t1)
        args.update(kw)
        with pytest.raises(pkg.QmcpError) as ex:
            solver.solve_targets(**args)
        assert ex.value.code == code, kw.keys()
        good_call()

    good_call()
    # a bad id / a bad read among the on-target reads and among the off-target reads: all are validated
    for victim in (int(np.flatnonzero(on)[0]), int(np.flatnonzero(placed & ~on)[0])):
        bad_ids = ids.copy()
        bad_ids[victim] = 3                                             # id 3 of 3 contigs
        fails(pkg.QMCP_EINVAL, contig_ids=bad_ids)
        bad_e = e.copy()
        bad_e[victim] = lengths[ids[victim]]                            # one past its contig's end
        fails(pkg.QMCP_EREAD, ends=bad_e)
        bad_s = s.copy()
        bad_s[victim] = e[victim] + 1                                   # start > end
        fails(pkg.QMCP_EREAD, starts=bad_s)
    # a bad table
    fails(pkg.QMCP_EINVAL, target_offsets=np.array([1, 1, 2, 2], np.uint32))
    fails(pkg.QMCP_EINVAL, target_offsets=np.array([0, 2, 1, 2], np.uint32))
    fails(pkg.QMCP_EINVAL, target_starts=np.array([130, 20], np.uint32))    # start > end
    fails(pkg.QMCP_EINVAL, target_offsets=None)
    fails(pkg.QMCP_EINVAL, target_starts=None)
    # the state of a device mask: untouched after a bad table (found on the host), all zero after a bad read
    n = s.size
    ds, de, di = _dev(s), _dev(e), _dev(ids)
    bad_e = e.copy()
    bad_e[int(np.flatnonzero(placed & ~on)[0])] = 0xFFFFFFF0
    d_bad_e = _dev(bad_e)
    d_mask = torch.full((pkg.mask_words(n),), -1, dtype=torch.int64, device="cuda:0")
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_targets_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M,
                                    np.array([0, 2, 1, 2], np.uint32), t0, t1, d_mask.data_ptr())
    assert ex.value.code == pkg.QMCP_EINVAL and bool((d_mask == -1).all())
    with pytest.raises(pkg.QmcpError) as ex:
        solver.solve_targets_device(ds.data_ptr(), d_bad_e.data_ptr(), di.data_ptr(), n, lengths, M, offs, t0, t1,
                                    d_mask.data_ptr())
    assert ex.value.code == pkg.QMCP_EREAD and bool((d_mask == 0).all())
    good_call()


@pytest.mark.parametrize("solver_name", ["quasi-mcp-hip", "quasi-mcp-hip-quality"])
def test_file_to_file_with_targets(pkg, oracle, solver, tmp_path, solver_name):
    import bam_py
    refs = [("chr1", 30_000), ("chr2", 12_000), ("chr3", 9_000), ("chrM", 4_000)]
    path = tmp_path / "multi.bam"
    header, parsed, ref_lengths = mr.write_multi_reference_bam(path, np.random.default_rng(21), refs, 15_000)
    bed = tmp_path / "targets.bed"
    bed.write_text("track name=targets\n# chr3 has none\nchr1\t1000\t1400\tex1\nchr1\t1350\t2000\nchr1\t20000\t20200\n"
                   "chr2\t0\t300\nchr2\t11900\t12000\nchrM\t100\t101\n")
    M, padding = 6, 25
    reads, ids, _ = mr.expected_per_reference_reads(parsed)
    starts = np.array([r["start"] if i != NO_CONTIG else 0 for r, i in zip(reads, ids)], np.int64).astype(np.uint32)
    ends = np.array([r["end"] if i != NO_CONTIG else 0 for r, i in zip(reads, ids)], np.int64).astype(np.uint32)
    offs, t0, t1 = pkg.targets_from_bed(bed, [n for n, _ in refs])
    assert offs.tolist() == [0, 3, 5, 5, 6]
    quality = solver_name.endswith("quality")
    q = np.array([r["q"] for r in reads], np.uint32) if quality else None
    bam_ids = np.array([r["bam_id"] for r in reads], dtype=np.int64)
    for keep_off in (False, True):
        want, on = tm.expected_mask(oracle, starts, ends, ids, ref_lengths, offs, t0, t1, M, padding=padding,
                                    keep_off_target=keep_off, qualities=q, quality_choice=qm.quality_choice)
        assert on.any() and not on.all()
        mask = oracle.find_pairs(want, len(reads))
        kept_ids = np.sort(bam_ids[pkg.mask_to_indices(mask, len(reads)).astype(np.int64)])
        out = tmp_path / f"out_{int(keep_off)}.bam"
        written = pkg.downsample_bam(solver_name, path, out, M, per_reference=True, targets=bed, target_padding=padding,
                                     keep_off_target=keep_off)
        oh, orecs, _ = bam_py.parse(out)
        assert oh == header and written == kept_ids.size == len(orecs) > 0
        assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]
    # the column path gives the same mask
    cols = pkg.read_bam(path, per_reference=True)
    got = solver.solve_targets(cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"], M, offs, t0, t1,
                               padding=padding, keep_off_target=True, qualities=cols["qualities"] if quality else None)
    assert np.array_equal(got, want)


def _grouping_ms(times):
    return sum(ms for name, (_, ms) in times.items() if name in GROUPING)


def test_pre_and_post_pass_cost_no_more_than_the_grouping_they_feed(pkg, solver):
    """cfg4's reads (10^8 on 8 contigs, shuffled) with regions that leave about half of them on target.  Asserted:
    ms_targets (projection + compaction + expansion; median of 5 after a warm-up) does not exceed the grouping stages
    (k_bc_keys, the radix pass, k_bc_bounds, k_bc_gather; per-kernel events, median of 5) of the plain by-contig solve of
    the same unprojected reads, measured here in the same process.  QMCP_TARGETS_TIME_OUT=<file> keeps the figures."""
    n_contigs, pairs, L, M = 8, 6_250_000, 1_000_000, 100
    rng = np.random.default_rng(4)
    ss, ee = zip(*(pkg.reads_gen(pkg.KIND_UNIFORM, pairs, L, 150, seed=12345 + c) for c in range(n_contigs)))
    s, e = np.concatenate(ss), np.concatenate(ee)
    ids = np.repeat(np.arange(n_contigs, dtype=np.uint32), 2 * pairs)
    perm = rng.permutation(s.size)
    s, e, ids = s[perm], e[perm], ids[perm]
    n = s.size
    lengths = np.full(n_contigs, L, np.uint32)
    # regions of 5 000 every 10 300 positions: a read of 150 touches one with probability (5 000 + 149) / 10 300 = 0.5
    starts_1 = np.arange(2_000, L - 5_000, 10_300, dtype=np.uint32)
    offs = (np.arange(n_contigs + 1) * starts_1.size).astype(np.uint32)
    t0 = np.tile(starts_1, n_contigs)
    t1 = t0 + 4_999
    ds, de, di = _dev(s), _dev(e), _dev(ids)
    d_mask = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    def targets():
        return solver.solve_targets_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M, offs, t0, t1,
                                           d_mask.data_ptr())

    def plain():
        return solver.solve_by_contig_device(ds.data_ptr(), de.data_ptr(), di.data_ptr(), n, lengths, M,
                                             d_mask.data_ptr())

    targets(); plain(); targets(); plain()                       # warm-up: arena growth, route memory
    ms_targets, ms_projected_solve = [], []
    for _ in range(5):
        ts = targets()
        ms_targets.append(float(ts.ms_targets))
        ms_projected_solve.append(float(solver.last_stats.ms_total))
    share = ts.reads_on_target / n
    assert 0.45 < share < 0.55, share
    grouping, plain_total, stage_runs, target_stage_runs = [], [], [], []
    for _ in range(5):
        solver.set_profiling(True)
        st = plain()
        kt = solver.kernel_times()
        grouping.append(_grouping_ms(kt))
        plain_total.append(float(st.ms_total))
        stage_runs.append({k: kt[k][1] for k in GROUPING if k in kt})
        solver.set_profiling(True)
        targets()
        kt = solver.kernel_times()
        target_stage_runs.append({k: kt[k][1] for k in TARGET_STAGES if k in kt})
    solver.set_profiling(False)
    med = statistics.median
    a, c_grouping = med(ms_targets), med(grouping)
    # bytes the three stages move at least: 12 B in + 8 B out per read (+ 2 bits), the compaction 1 bit + 12 B per read
    # looked at (the ids, and the lines of the projections) and 16 B out per survivor, the expansion ~0
    n_on = int(ts.reads_on_target)
    need_bytes = 20 * n + n // 4 + 12 * n + 16 * n_on
    figures = {
        "reads": n, "contigs": n_contigs, "M": M, "regions": int(t0.size), "on_target_share": round(share, 4),
        "a_ms_targets_median": round(a, 4), "a_ms_targets_runs": [round(x, 4) for x in ms_targets],
        "a_stages_ms_median": {k: round(med([r.get(k, 0.0) for r in target_stage_runs]), 4) for k in TARGET_STAGES},
        "b_projected_solve_device_ms_median": round(med(ms_projected_solve), 4),
        "c_grouping_ms_median": round(c_grouping, 4), "c_grouping_runs": [round(x, 4) for x in grouping],
        "c_grouping_stages_ms_median": {k: round(med([r.get(k, 0.0) for r in stage_runs]), 4) for k in GROUPING},
        "c_plain_by_contig_device_ms_median": round(med(plain_total), 4),
        "a_min_bytes": need_bytes, "a_ms_at_copy_rate_6.29TBps": round(need_bytes / 6.29e12 * 1e3, 4),
    }
    print("targets_time " + json.dumps(figures))
    out = os.environ.get("QMCP_TARGETS_TIME_OUT")
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(figures, indent=1) + "\n")
    assert a <= c_grouping, figures
