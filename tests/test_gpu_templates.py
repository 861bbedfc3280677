"""qmcp_hip_solve_templates_*: the staged solve whose unit is every segment that carries one template id.  Every mask is
compared bit for bit with tests/template_model.py through both the host and the device entry; ids i // 2 with
qmcp_hip_solve_pairs_*, distinct ids with qmcp_hip_solve_by_contig_*; the file flow with the records of the model's kept
templates."""
import ctypes as C

import numpy as np
import pytest
import torch

import bam_py
import pair_model as pairs
import profile_model as pm
import template_bams as tb
import template_model as tm

pytestmark = pytest.mark.gpu

NO_CONTIG = 0xFFFFFFFF
QMCP_EINVAL = -1
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
STAGE_FIELDS = ("target", "n_selected", "n_kept", "capped_positions", "demand", "sweeps")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")


def solve_device(pkg, solver, s, e, ids, tids, n_templates, lengths, M, stages):
    """the device entry on a mask buffer filled with ones, one guard word behind it"""
    n = s.size
    words = pkg.mask_words(n)
    cols = [_dev(x) for x in (s, e, ids, tids)]
    d_mask = torch.full((words + 1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st, ts = solver.solve_templates_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(),
                                           n, n_templates, lengths, M, d_mask.data_ptr(), stages,
                                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_mask.cpu().numpy().view(np.uint64)
    assert out[words] == ALL_ONES                                        # nothing written past the mask
    if n % 64:
        assert int(out[words - 1]) >> (n % 64) == 0                      # no bit at or beyond n_reads
    return out[:words].copy(), st, ts


def solve_host_prefilled(pkg, solver, s, e, ids, tids, n_templates, lengths, M, stages):
    """the host entry through the C ABI, keep_mask_out filled with 0xFF"""
    n = s.size
    words = pkg.mask_words(n)
    cols = [np.ascontiguousarray(x, np.uint32) for x in (s, e, ids, tids, lengths)]
    tg = None if stages is None else np.asarray(stages, np.uint32)
    out = np.full(words + 1, ALL_ONES, np.uint64)
    st, ts = pkg.Stats(), pkg.TemplateStats()
    u32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    rc = pkg._hip.qmcp_hip_solve_templates_host(solver._ctx, u32(cols[0]), u32(cols[1]), u32(cols[2]), u32(cols[3]), n,
                                                n_templates, u32(cols[4]), cols[4].size, M, u32(tg),
                                                0 if tg is None else tg.size, out.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                C.byref(st), C.byref(ts))
    assert rc == 0, pkg._hip.qmcp_hip_last_error()
    assert out[words] == ALL_ONES
    if n % 64:
        assert int(out[words - 1]) >> (n % 64) == 0
    return out[:words].copy(), st, ts


def check_both_entries(pkg, solver, inst, M, stages):
    """host and device entry against the model: mask, per-stage counts, template counts -> the host call's stats"""
    s, e, ids, tids, n_templates, lengths = inst
    n = s.size
    want, selected, kept, sets = tm.staged(s, e, ids, tids, n_templates, lengths, M, stages)
    hist, used, largest = tm.template_counts(tids, n_templates)
    out = None
    for entry in ("host", "device"):
        solve = solve_host_prefilled if entry == "host" else solve_device
        got, st, ts = solve(pkg, solver, s, e, ids, tids, n_templates, lengths, M, stages)
        diff = int(np.count_nonzero(pm.unpack(got ^ want, n))) if n else 0
        assert np.array_equal(got, want), (entry, M, stages, diff)
        k = len(selected)
        assert ts.n_stages == k and list(ts.target)[:k] == (tm.default_stages(M) if stages is None else list(stages))
        assert list(ts.n_selected)[:k] == selected and list(ts.n_kept)[:k] == kept, (entry, M, stages)
        assert st.n_kept == selected[0] and ts.sweeps[0] == 0
        assert list(ts.size_hist) == hist and ts.n_templates_used == used and ts.max_template_size == largest
        assert ts.n_templates_kept == tm.kept_templates(sets[-1], tids)
        assert tm.whole_templates(sets[-1], tids, n_templates) and tm.covers(s, e, ids, lengths, sets[-1], M)
        for j in range(1, k):
            assert (ts.sweeps[j] >= 1) == (ts.demand[j] > 0) == (selected[j] > 0)
        out = out or (st, ts)
    got, _, _ = solver.solve_templates(s, e, ids, tids, n_templates, lengths, M, stages)
    assert np.array_equal(got, want)
    return out, selected


# ------------------------------------------------------------------------------------------ instances
def segments(seed, n, M, n_contigs=3, unplaced=0.05):
    """n segments of spans 20 .. 200 on 2 - 3 contigs of 500 .. 5 000 positions, depth about 2 .. 8 x M where n allows
    it (the contigs shrink towards 500 positions, then the spans towards 20), some unplaced, shuffled"""
    rng = np.random.default_rng(seed)
    depth = float(rng.uniform(2, 8)) * M
    hi = 200
    per = n * (20 + hi) / 2 / depth / n_contigs
    while per > 5000 and hi > 40:
        hi -= 20
        per = n * (20 + hi) / 2 / depth / n_contigs
    lengths = np.clip(rng.uniform(0.7, 1.3, size=n_contigs) * per, 500, 5000).astype(np.uint32)
    ids = rng.integers(0, n_contigs, size=n).astype(np.uint32)
    span = rng.integers(20, hi + 1, size=n)
    s = (rng.random(n) * (lengths[ids].astype(np.int64) - span + 1)).astype(np.int64)
    e = s + span - 1
    ids[rng.random(n) < unplaced] = NO_CONTIG
    return s.astype(np.uint32), e.astype(np.uint32), ids, lengths


SIZES = [0, 1, 63, 64, 65, 4097, 20_000]


@pytest.mark.parametrize("M", [1, 3, 10])
@pytest.mark.parametrize("n", SIZES)
def test_random_templates_equal_the_model(pkg, solver, n, M):
    """template sizes 1 .. 6 and one template of 1 000 segments (where n allows), ids dealt through a permutation: a
    template's segments lie in different words, workgroups and contigs, some are unplaced; n_templates % 32 is 0, 1 or
    31, ids are left unused and the highest id is in use"""
    s, e, ids, lengths = segments(100 + 7 * n + M, n, M, n_contigs=2 + (n + M) % 2)
    large = 1000 if n >= 4097 else 0
    _, used = tm.random_templates(np.random.default_rng(7 * n + M), n, large=large)
    rest = {1: 0, 3: 1, 10: 31}[M]
    n_templates = used + 5 + (rest - used - 5) % 32                      # some ids stay unused
    tids, n_templates = tm.random_templates(np.random.default_rng(7 * n + M), n, n_templates, large=large)
    assert n_templates % 32 == rest and (n == 0 or int(tids.max()) == n_templates - 1)
    if large:
        big = np.flatnonzero(tids == np.bincount(tids).argmax())
        assert big.size == 1000 and np.unique(big // 256).size > 12 and np.unique(ids[big]).size >= 3   # incl. unplaced
    (st, ts), selected = check_both_entries(pkg, solver, (s, e, ids, tids, n_templates, lengths), M, None)
    assert ts.n_stages == (1 if M == 1 else 2)
    (st, ts), _ = check_both_entries(pkg, solver, (s, e, ids, tids, n_templates, lengths), M, [M])
    assert ts.n_stages == 1


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_one_template_holds_every_segment(pkg, solver, n):
    """n_templates = 1: the first kept segment brings every other one along, unplaced ones included"""
    s, e, ids, lengths = segments(900 + n, n, 3)
    s[0], e[0], ids[0] = 0, 19, 0                                        # at least one placed segment
    tids = np.zeros(n, np.uint32)
    (st, ts), _ = check_both_entries(pkg, solver, (s, e, ids, tids, 1, lengths), 3, None)
    assert ts.n_kept[0] == n and ts.n_templates_kept == 1 and ts.max_template_size == n
    assert ts.n_selected[1] == 0 and ts.sweeps[1] == 0                   # no candidate is left for stage 2


@pytest.mark.parametrize("M", [3, 10])
def test_three_stages_on_scattered_templates(pkg, solver, M):
    s, e, ids, lengths = segments(40 + M, 4097, M)
    tids, n_templates = tm.random_templates(np.random.default_rng(M), 4097, large=1000)
    (st, ts), selected = check_both_entries(pkg, solver, (s, e, ids, tids, n_templates, lengths), M, [1, 2, M])
    assert ts.n_stages == 3 and sum(selected[1:]) > 0 and sum(ts.sweeps[1:3]) >= 1


# ------------------------------------------------------------------------------------------ the identities
def pair_instances(M):
    """pair_model.overshoot's pairs on one contig, and the same pairs dealt over three contigs with unplaced mates"""
    s, e, ids, lengths = pairs.overshoot(M, 5000, M, 4)
    yield s, e, ids, lengths
    rng = np.random.default_rng(M)
    lengths3 = np.array([5000, 5000, 5000], np.uint32)
    ids3 = rng.integers(0, 3, size=s.size).astype(np.uint32)
    ids3[rng.random(s.size) < 0.04] = NO_CONTIG
    yield s, e, ids3, lengths3


@pytest.mark.parametrize("M", [1, 3, 10])
def test_ids_i_div_2_equal_solve_pairs_bit_for_bit(pkg, solver, M):
    three = {1: [1], 3: [1, 2, 3], 10: [2, 5, 10]}[M]
    for s, e, ids, lengths in pair_instances(M):
        n = s.size
        assert n % 2 == 0 and n > 128
        tids = (np.arange(n) // 2).astype(np.uint32)
        for stages in (None, [M], three):
            want, st_p, ps = solver.solve_pairs(s, e, ids, lengths, M, stages)
            want = want.copy()
            got, st_t, ts = solver.solve_templates(s, e, ids, tids, n // 2, lengths, M, stages)
            assert np.array_equal(got, want), (M, stages)
            got_d, _, ts_d = solve_device(pkg, solver, s, e, ids, tids, n // 2, lengths, M, stages)
            assert np.array_equal(got_d, want)
            assert ts.n_stages == ps.n_stages == ts_d.n_stages
            for f in STAGE_FIELDS:
                assert list(getattr(ts, f)) == list(getattr(ps, f)) == list(getattr(ts_d, f)), (f, M, stages)
            assert st_t.n_kept == st_p.n_kept and st_t.n_reads == st_p.n_reads and st_t.path == st_p.path
            assert list(ts.size_hist) == [0, n // 2, 0, 0, 0, 0, 0, 0] and ts.max_template_size == 2
            assert 2 * ts.n_templates_kept == ts.n_kept[ts.n_stages - 1]


@pytest.mark.parametrize("M, n", [(1, 65), (3, 4097), (10, 20_000)])
def test_distinct_ids_and_one_stage_equal_solve_by_contig_bit_for_bit(pkg, solver, M, n):
    s, e, ids, lengths = segments(300 + n, n, M)
    tids = np.random.default_rng(n).permutation(n).astype(np.uint32)
    want = solver.solve_by_contig(s, e, ids, lengths, M).copy()
    plain_kept = solver.last_stats.n_kept
    got, st, ts = solver.solve_templates(s, e, ids, tids, n, lengths, M, [M])
    got_d, _, _ = solve_device(pkg, solver, s, e, ids, tids, n, lengths, M, [M])
    assert np.array_equal(got, want) and np.array_equal(got_d, want)
    assert ts.n_selected[0] == ts.n_kept[0] == ts.n_templates_kept == plain_kept == st.n_kept
    assert list(ts.size_hist) == [n, 0, 0, 0, 0, 0, 0, 0] and ts.n_templates_used == n


def test_one_stage_is_solve_by_contig_and_the_template_completion(pkg, solver):
    M, n = 3, 4097
    s, e, ids, lengths = segments(77, n, M)
    tids, n_templates = tm.random_templates(np.random.default_rng(77), n, large=1000)
    plain = pm.unpack(solver.solve_by_contig(s, e, ids, lengths, M), n)
    got, st, ts = solver.solve_templates(s, e, ids, tids, n_templates, lengths, M, [M])
    assert np.array_equal(pm.unpack(got, n), tm.complete(plain, tids, n_templates))
    assert ts.n_selected[0] == int(plain.sum())


# ------------------------------------------------------------------------------------------ errors
def test_an_id_beyond_n_templates_is_refused_with_the_mask_cleared(pkg, solver):
    n = 4097
    s, e, ids, lengths = segments(5, n, 3)
    tids, n_templates = tm.random_templates(np.random.default_rng(5), n)
    for where in (0, 2048, n - 1):
        bad = tids.copy()
        bad[where] = n_templates
        with pytest.raises(pkg.QmcpError) as err:
            solver.solve_templates(s, e, ids, bad, n_templates, lengths, 3)
        assert err.value.code == QMCP_EINVAL and "template id" in str(err.value)
        cols = [_dev(x) for x in (s, e, ids, bad)]
        d_mask = torch.full((pkg.mask_words(n) + 1,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(pkg.QmcpError) as err:
            solver.solve_templates_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), n,
                                          n_templates, lengths, 3, d_mask.data_ptr())
        assert err.value.code == QMCP_EINVAL
        torch.cuda.synchronize()
        out = d_mask.cpu().numpy()
        assert (out[:-1] == 0).all() and out[-1] == -1                   # cleared, and nothing behind it touched
    # the context is still good
    check_both_entries(pkg, solver, (s, e, ids, tids, n_templates, lengths), 3, None)


# ------------------------------------------------------------------------------------------ the file flow
def check_file_flow(pkg, solver, tmp_path, name, refs, records, M, stages=None, **ingest):
    """downsample_bam(template_aware=True) writes exactly the records of the model's kept templates, in file order, and
    the kept segments reach min(cov, M) on every reference"""
    path = tmp_path / f"{name}.bam"
    bam_py.write_bam(path, refs, records)
    header, parsed, _ = bam_py.parse(path)
    segs = tb.expected_segments(records, **ingest)
    cols = pkg.read_bam(path, per_reference=True, templates=True, **ingest)
    for key in ("starts", "ends", "contig_ids", "template_ids", "segment_records"):
        assert np.array_equal(np.asarray(cols[key], np.int64), np.asarray(segs[key], np.int64)), key
    want, _, kept, sets = tm.staged(segs["starts"], segs["ends"], segs["contig_ids"], segs["template_ids"],
                                    segs["n_templates"], cols["contig_lengths"], M, stages)
    assert tm.covers(segs["starts"], segs["ends"], segs["contig_ids"], cols["contig_lengths"], sets[-1], M)
    kept_records = np.unique(np.asarray(segs["segment_records"], np.int64)[sets[-1]])
    out, report = tmp_path / f"{name}.out.bam", tmp_path / f"{name}.tsv"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, template_aware=True,
                                 template_stages=stages, template_report=report, **ingest)
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == kept_records.size == len(orecs) > 0
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_records.tolist()]
    assert pkg.check_bam(out)[0]
    rows = dict(line.split("\t", 1) for line in report.read_text().splitlines() if "\t" in line)
    hist, used, largest = tm.template_counts(segs["template_ids"], segs["n_templates"])
    assert int(rows["templates_used"]) == used and int(rows["max_template_size"]) == largest
    assert int(rows["templates_kept"]) == tm.kept_templates(sets[-1], segs["template_ids"])
    assert int(rows["segments_kept"]) == kept[-1]
    assert [int(rows[k]) for k in ("1", "2", "3", "4", "5", "6", "7", "8+")] == hist
    return segs, sets[-1], written


def test_downsample_bam_template_aware_on_a_single_end_file(pkg, solver, tmp_path):
    refs = [("chrA", 4000), ("chrB", 2500)]
    records = tb.single_end_records(np.random.default_rng(3), refs, 1500)
    segs, kept, written = check_file_flow(pkg, solver, tmp_path, "single", refs, records, 5)
    assert segs["n_templates"] == len(records) and 0 < written < len(records)
    # without the feature every record of this file is lost
    assert pkg.downsample_bam("quasi-mcp-hip", tmp_path / "single.bam", tmp_path / "plain.bam", 5, per_reference=True) == 0


def test_downsample_bam_template_aware_on_a_mixed_file(pkg, solver, tmp_path):
    """pairs, spliced reads, a split read with a supplementary, secondaries, unmapped mates"""
    refs = [("chrA", 5000), ("chrB", 3000), ("chrC", 800)]
    records = tb.mixed_records(np.random.default_rng(11), refs, 700)
    for stages in (None, [1, 2, 6]):
        segs, kept, written = check_file_flow(pkg, solver, tmp_path, "mixed", refs, records, 6, stages)
        sizes = np.bincount(segs["template_ids"])
        assert sizes.max() >= 4 and (sizes == 1).any() and (segs["contig_ids"] == NO_CONTIG).any()
        assert 0 < written < len(records)
    segs_all, _, _ = check_file_flow(pkg, solver, tmp_path, "mixed_sec", refs, records, 6, include_secondary=True)
    segs_whole, _, _ = check_file_flow(pkg, solver, tmp_path, "mixed_whole", refs, records, 6, split_spliced=False)
    assert len(segs_all["starts"]) > len(segs["starts"]) > len(segs_whole["starts"])


def test_template_aware_refuses_what_it_does_not_go_together_with(pkg, tmp_path):
    refs = [("chrA", 4000)]
    path = tmp_path / "in.bam"
    bam_py.write_bam(path, refs, tb.single_end_records(np.random.default_rng(1), refs, 50))
    bed = tmp_path / "t.bed"
    bed.write_text("chrA\t10\t500\n")
    graph = tmp_path / "caps.bedgraph"
    graph.write_text("chrA\t10\t500\t3\n")
    go = lambda **kw: pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", 4,
                                         **{"per_reference": True, "template_aware": True, **kw})
    refused = [dict(per_reference=False), dict(pair_aware=True), dict(targets=bed), dict(profile=graph),
               dict(ladder=[3], ladder_out=tmp_path / "l{M}.bam"), dict(stratify="strand"), dict(dedup=True),
               dict(bed=bed, amplicons_by_reference=True), dict(tsv=bed), dict(report=tmp_path / "r.tsv"),
               dict(track=tmp_path / "t.bedgraph"), dict(template_stages=[3, 5]), dict(template_stages=[])]
    for kw in refused:
        with pytest.raises(ValueError):
            go(**kw)
    with pytest.raises(ValueError):
        pkg.downsample_bam("quasi-mcp-hip-quality", path, tmp_path / "no.bam", 4, per_reference=True, template_aware=True)
    for kw in (dict(template_stages=[2, 4]), dict(template_report=tmp_path / "r.tsv"), dict(include_secondary=True),
               dict(split_spliced=False)):
        with pytest.raises(ValueError):
            pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", 4, per_reference=True, **kw)
    assert not (tmp_path / "no.bam").exists()
