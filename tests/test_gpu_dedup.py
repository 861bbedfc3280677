"""qmcp_hip_solve_dedup_*: duplicate families collapsed before the by-contig solve.  Keep mask, duplicate mask,
statistics and family-size histogram are compared bit for bit with the literal model on the oracle
(tests/dedup_model.py)."""
import ctypes as C

import numpy as np
import pytest

import dedup_model as dm
import multi_reference as mr

pytestmark = pytest.mark.gpu

STAT_KEYS = ("units", "families", "duplicate_units", "largest_family", "reads_survived")
BINS = 8


def check(solver, oracle, s, e, ids, lengths, M, tags=None, q=None, pairs=False, complete=False, bins=BINS,
          by_contig=None, what=""):
    """the host entry against the model; -> (keep bits, dup bits, stats dict of the entry)"""
    mask, dup, st, hist = solver.solve_dedup(s, e, ids, lengths, M, tags=tags, qualities=q, pairs=pairs,
                                             complete_pairs=complete, hist_bins=bins)
    keep_w, dup_w, st_w, hist_w = dm.dedup(oracle, s, e, ids, lengths, M, tags=tags, qualities=q, pairs=pairs,
                                           complete_pairs=complete, hist_bins=bins, by_contig=by_contig)
    n = len(s)
    assert mask.size == dup.size == (n + 63) // 64
    assert np.array_equal(dup, dm.pack(dup_w)), f"{what}: duplicate mask"
    assert {k: st[k] for k in STAT_KEYS} == st_w, f"{what}: stats"
    assert np.array_equal(hist, hist_w), f"{what}: histogram {hist} != {hist_w}"
    assert np.array_equal(mask, dm.pack(keep_w)), f"{what}: keep mask"
    assert not (mask & dup).any()
    if not complete:
        assert solver.last_stats.n_kept == keep_w.sum()
    return keep_w, dup_w, st


def duplicated_reads(rng, n, lengths, n_sites=50, unplaced=0.05):
    """n reads drawn from at most n_sites intervals over the contigs, a few unplaced"""
    lengths = np.asarray(lengths, np.uint32)
    site_ids = rng.integers(0, lengths.size, size=n_sites)
    span = rng.integers(1, 40, size=n_sites)
    site_s = (rng.random(n_sites) * (lengths[site_ids] - span + 1)).astype(np.int64)
    pick = rng.integers(0, n_sites, size=n)
    ids = np.where(rng.random(n) < unplaced, mr.NO_CONTIG, site_ids[pick])
    return site_s[pick].astype(np.uint32), (site_s[pick] + span[pick] - 1).astype(np.uint32), ids.astype(np.uint32)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 8191, 8193])
def test_read_mode_sizes_across_word_wave_and_tile_edges(solver, oracle, n):
    rng = np.random.default_rng(100 + n)
    lengths = [700, 400]
    s, e, ids = duplicated_reads(rng, n, lengths)
    tags = rng.integers(0, 2, size=n).astype(np.uint32)
    q = rng.integers(0, 4, size=n).astype(np.uint32)          # (ties in quality inside every family)
    _, dup, st = check(solver, oracle, s, e, ids, lengths, 3, tags=tags, q=q, what=f"n={n}")
    if n > 200:
        assert st["duplicate_units"] > n // 2 and st["key_bits"] <= 32 and st["sort_passes"] == (st["key_bits"] + 7) // 8


def test_one_family_holds_every_read(solver, oracle):
    n = 20_000
    s, e, ids = np.full(n, 17, np.uint32), np.full(n, 60, np.uint32), np.zeros(n, np.uint32)
    q = np.zeros(n, np.uint32)
    q[12_345] = q[15_000] = 9                                 # the representative: the first of the two best
    keep, dup, st = check(solver, oracle, s, e, ids, [100], 5, q=q)
    assert st["families"] == 1 and st["largest_family"] == n and st["reads_survived"] == 1
    assert np.flatnonzero(keep).tolist() == [12_345] and dup.sum() == n - 1
    keep, dup, st = check(solver, oracle, s, e, ids, [100], 5)   # no qualities: the key is gstart alone (7 bits)
    assert np.flatnonzero(keep).tolist() == [0] and st["key_bits"] == 7 and st["sort_passes"] == 1


def test_families_straddle_the_sort_tile_edges(solver, oracle):
    """one read per start, except that the cells at sorted positions 4 093 and 8 189 hold six reads each: both families
    lie across a sort tile's (4 096) and a scan tile's edge"""
    rng = np.random.default_rng(9)
    sizes = np.ones(9000, dtype=np.int64)
    sizes[4093] = 6
    sizes[8189 - 5] = 6                                       # (sorted position = reads of the cells before it)
    starts = np.repeat(np.arange(sizes.size), sizes)
    assert starts[4093] == starts[4098] == 4093 and starts[8189] == starts[8194] != starts[8188] and starts[8195] != starts[8194]
    perm = rng.permutation(starts.size)
    s = starts[perm].astype(np.uint32)
    e = (s + 30).astype(np.uint32)
    q = rng.integers(0, 3, size=s.size).astype(np.uint32)
    _, _, st = check(solver, oracle, s, e, np.zeros(s.size, np.uint32), [9100], 4, q=q)
    assert st["families"] == 9000 and st["largest_family"] == 6 and st["duplicate_units"] == 10


def test_all_units_unique_is_solve_by_contig_bit_for_bit(solver, oracle):
    rng = np.random.default_rng(12)
    s, e, ids, lengths = mr.random_by_contig(rng, 3, max_reads_per_contig=2000)
    tags = rng.permutation(s.size).astype(np.uint32)          # every cell its own
    q = rng.integers(0, 61, size=s.size).astype(np.uint32)
    for M in (1, 7, 40):
        plain = solver.solve_by_contig(s, e, ids, lengths, M)
        mask, dup, st, _ = solver.solve_dedup(s, e, ids, lengths, M, tags=tags, qualities=q)
        assert np.array_equal(mask, plain) and not dup.any() and st["duplicate_units"] == 0
        n = s.size - s.size % 2
        plain = solver.solve_by_contig(s[:n], e[:n], ids[:n], lengths, M)
        mask, dup, st, _ = solver.solve_dedup(s[:n], e[:n], ids[:n], lengths, M, tags=tags[:n], qualities=q[:n], pairs=True)
        assert np.array_equal(mask, plain) and not dup.any() and st["duplicate_units"] == 0
    check(solver, oracle, s, e, ids, lengths, 7, tags=tags, q=q)


def test_null_tags_equal_one_tag_and_null_qualities_pick_the_lowest_index(solver, oracle):
    rng = np.random.default_rng(13)
    lengths = [500, 300]
    s, e, ids = duplicated_reads(rng, 3000, lengths, n_sites=40)
    q = rng.integers(0, 61, size=s.size).astype(np.uint32)
    a = solver.solve_dedup(s, e, ids, lengths, 3, qualities=q, hist_bins=BINS)
    b = solver.solve_dedup(s, e, ids, lengths, 3, tags=np.full(s.size, 0xDEADBEEF, np.uint32), qualities=q, hist_bins=BINS)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert {k: a[2][k] for k in STAT_KEYS + ("key_bits",)} == {k: b[2][k] for k in STAT_KEYS + ("key_bits",)}
    check(solver, oracle, s, e, ids, lengths, 3, q=q)
    # no qualities: the survivors are the first read of every cell
    _, dup, _ = check(solver, oracle, s, e, ids, lengths, 3)
    placed = ids != mr.NO_CONTIG
    cells = np.stack([ids, s, e], axis=1)[placed]
    _, first = np.unique(cells, axis=0, return_index=True)
    assert np.array_equal(np.flatnonzero(placed & ~dup), np.sort(np.flatnonzero(placed)[first]))
    # ties: two reads of a cell with the best quality -> the lower index survives
    qt = np.minimum(q, 1).astype(np.uint32)
    check(solver, oracle, s, e, ids, lengths, 3, q=qt)


def raw_host(pkg, solver, s, e, ids, tags, q, lengths, M, flags, mask, dup, hist):
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    p64 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint64))
    return pkg._hip.qmcp_hip_solve_dedup_host(solver._ctx, p(s), p(e), p(ids), p(tags), p(q), s.size, p(lengths),
                                              lengths.size, M, flags, p64(mask), p64(dup), p64(hist),
                                              0 if hist is None else hist.size, None, None)


def test_quality_range_and_errors_leave_the_outputs_untouched(pkg, solver, oracle):
    rng = np.random.default_rng(14)
    lengths = [500, 300]
    s, e, ids = duplicated_reads(rng, 1000, lengths, n_sites=30)
    placed = np.flatnonzero(ids != mr.NO_CONTIG)
    q = rng.integers(100, 2000, size=s.size).astype(np.uint32)
    q[placed[3]], q[placed[7]] = 100, 100 + 65535
    unplaced = np.flatnonzero(ids == mr.NO_CONTIG)
    q[unplaced] = 0xFFFFFFF0                                    # (unplaced reads do not count towards the range)
    check(solver, oracle, s, e, ids, lengths, 3, q=q, what="range 65535")
    guard = np.uint64(0xA5A5A5A5A5A5A5A5)
    words = (s.size + 63) // 64

    def refused(code, word, s=s, e=e, ids=ids, q=q, flags=0, lengths=lengths):
        mask, dup, hist = (np.full(words + 2, guard, np.uint64) for _ in range(3))
        rc = raw_host(pkg, solver, s, e, ids, None, q, lengths, 3, flags, mask, dup, hist[:BINS])
        assert rc == code, (rc, pkg._hip.qmcp_hip_last_error())
        assert word in pkg._hip.qmcp_hip_last_error().decode(), pkg._hip.qmcp_hip_last_error()
        assert (mask == guard).all() and (dup == guard).all() and (hist == guard).all()

    q2 = q.copy()
    q2[placed[7]] += 1
    refused(pkg.QMCP_ERANGE, "65535", q=q2)
    refused(pkg.QMCP_ERANGE, "65535", q=q2, flags=pkg.DEDUP_PAIRS)
    refused(pkg.QMCP_EINVAL, "even", s=s[:999], e=e[:999], ids=ids[:999], q=q[:999], flags=pkg.DEDUP_PAIRS)
    refused(pkg.QMCP_EINVAL, "even", s=s[:999], e=e[:999], ids=ids[:999], q=q[:999],
            flags=pkg.DEDUP_PAIRS | pkg.DEDUP_COMPLETE_PAIRS)
    refused(pkg.QMCP_EINVAL, "QMCP_DEDUP_PAIRS", flags=pkg.DEDUP_COMPLETE_PAIRS)
    refused(pkg.QMCP_EINVAL, "flag", flags=4)
    # a bad read inside a duplicate: the second copy of a cell ends past its contig
    p0 = placed[0]
    copies = np.flatnonzero((s == s[p0]) & (e == e[p0]) & (ids == ids[p0]))
    assert copies.size >= 2
    e2 = e.copy()
    i = copies[1]
    e2[i] = lengths[int(ids[i])]
    refused(pkg.QMCP_EREAD, "read", e=e2)
    ids2 = ids.copy()
    ids2[i] = 2
    refused(pkg.QMCP_EINVAL, "contig id", ids=ids2)
    check(solver, oracle, s, e, ids, lengths, 3, q=q, what="after the refusals")


def wide_case(rng, tag_hi, span_lo=30, span_hi=31):
    lengths = [1 << 27, 1 << 27]
    n, n_sites = 4096, 600
    site_ids = rng.integers(0, 2, size=n_sites)
    site_s = rng.integers(0, (1 << 27) - 100, size=n_sites)
    site_s[:4] = (1 << 27) - 40                                 # gstart's top bits in use on both contigs
    site_span = rng.integers(span_lo, span_hi + 1, size=n_sites)
    pick = rng.integers(0, n_sites, size=n)
    s = site_s[pick].astype(np.uint32)
    e = (s + site_span[pick] - 1).astype(np.uint32)
    tags = rng.choice(np.array([0, 1, tag_hi // 3, tag_hi], dtype=np.uint64), size=n).astype(np.uint32)
    ids = np.where(rng.random(n) < 0.03, mr.NO_CONTIG, site_ids[pick]).astype(np.uint32)
    q = rng.integers(0, 61, size=n).astype(np.uint32)
    return s, e, ids, tags, q, lengths


def test_wide_keys_and_the_sort_field_by_field(solver, oracle):
    """two contigs of 2^27 positions: gstart takes 29 bits.  Tags over 20 bits force the split 64-bit key; tags over the
    full uint32 range with 6 bits of quality and 1 of span go beyond 64 bits: one sort per field.  The oracle does not
    take 2^28 positions, so the model's inner solve is the by-contig entry here."""
    inner = solver.solve_by_contig
    for pairs in (False, True):
        rng = np.random.default_rng(15)
        s, e, ids, tags, q, lengths = wide_case(rng, (1 << 20) - 1)
        _, _, st = check(solver, oracle, s, e, ids, lengths, 2, tags=tags, q=q, pairs=pairs, by_contig=inner, what="64-bit")
        if not pairs:
            assert st["key_bits"] == 29 + 1 + 20 + 6 and st["sort_passes"] == 7
        s, e, ids, tags, q, lengths = wide_case(rng, (1 << 32) - 1)
        _, _, st = check(solver, oracle, s, e, ids, lengths, 2, tags=tags, q=q, pairs=pairs, by_contig=inner, what="fields")
        if not pairs:
            assert st["key_bits"] == 29 + 1 + 32 + 6 == 68 and st["sort_passes"] == 1 + 4 + 1 + 4
    # pair mode's first sort carries no quality: 29 + 32 + 1 = 62 bits fit 64; four bits of span push it beyond
    s, e, ids, tags, q, lengths = wide_case(np.random.default_rng(16), (1 << 32) - 1, span_lo=20, span_hi=35)
    check(solver, oracle, s, e, ids, lengths, 2, tags=tags, q=q, pairs=True, by_contig=inner, what="pairs, fields")
    check(solver, oracle, s, e, ids, lengths, 2, tags=tags, q=q, by_contig=inner, what="reads, fields, 4 span bits")


def pair_case(rng, n, lengths):
    """n reads = n / 2 units over a few cells: mates on different contigs, one or both mates unplaced, mates sharing one
    cell, and every signature in both mate orders"""
    lengths = np.asarray(lengths, np.uint32)
    n_cells = 6
    cell_ids = np.arange(n_cells) % lengths.size
    cell_s = rng.integers(0, 50, size=n_cells)
    cell_e = cell_s + rng.integers(5, 40, size=n_cells)
    a = rng.integers(-1, n_cells, size=n // 2)                  # -1: unplaced
    b = rng.integers(-1, n_cells, size=n // 2)
    same = rng.random(n // 2) < 0.15
    b = np.where(same, a, b)
    if n >= 8:
        a[:4], b[:4] = [0, 1, -1, 2], [1, 0, -1, 2]             # (A, B), (B, A), both unplaced, one cell twice
    cells = np.stack([a, b], axis=1).reshape(-1)
    ids = np.where(cells < 0, mr.NO_CONTIG, cell_ids[cells]).astype(np.uint32)
    s = np.where(cells < 0, rng.integers(0, 1 << 30, size=n), cell_s[cells]).astype(np.uint32)
    e = np.where(cells < 0, rng.integers(0, 1 << 30, size=n), cell_e[cells]).astype(np.uint32)
    return s, e, ids


@pytest.mark.parametrize("n", [2, 126, 128, 130, 16_386])
def test_pair_mode(solver, oracle, n):
    rng = np.random.default_rng(200 + n)
    lengths = [100, 120]
    s, e, ids = pair_case(rng, n, lengths)
    tags = rng.integers(0, 2, size=n).astype(np.uint32)
    q = rng.integers(0, 4, size=n).astype(np.uint32)
    for complete in (False, True):
        keep, dup, st = check(solver, oracle, s, e, ids, lengths, 2, tags=tags, q=q, pairs=True, complete=complete,
                              what=f"n={n} complete={complete}")
        assert np.array_equal(dup[0::2], dup[1::2])
        if complete:
            assert np.array_equal(keep[0::2], keep[1::2])
    check(solver, oracle, s, e, ids, lengths, 2, pairs=True, what=f"n={n}, no tags, no qualities")
    if n >= 8:
        # (A, B) and (B, A) are one family whatever their tags say about order: give both the same tags per cell
        t2 = tags.copy()
        t2[0:4] = [5, 6, 6, 5]
        _, dup, _ = check(solver, oracle, s, e, ids, lengths, 2, tags=t2, q=q, pairs=True)
        assert dup[0] or dup[2]                                 # one family: at most one of the two is its representative
        assert not dup[4:6].any()                               # both mates unplaced: in no family


def test_device_entry_equals_the_host_entry_at_any_alignment(pkg, solver, oracle):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(17)
    lengths = [700, 400]
    n = 5000
    s, e, ids = duplicated_reads(rng, n, lengths)
    tags = rng.integers(0, 3, size=n).astype(np.uint32)
    q = rng.integers(0, 61, size=n).astype(np.uint32)
    words = pkg.mask_words(n)
    guard = -0x0123456789ABCDEF
    for pairs in (False, True):
        want = solver.solve_dedup(s, e, ids, lengths, 3, tags=tags, qualities=q, pairs=pairs, complete_pairs=pairs,
                                  hist_bins=BINS)
        for shift in (0, 1):
            cols = []
            for x in (s, e, ids, tags, q):
                t = torch.zeros(n + shift + 4, dtype=torch.int32, device=dev)   # (a base allocation is 256-byte aligned)
                t[shift:shift + n] = torch.from_numpy(x.view(np.int32)).to(dev)
                cols.append(t)
            d_mask = torch.full((words + 3,), guard, dtype=torch.int64, device=dev)
            d_dup = torch.full((words + 3,), guard, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            ptr = [t.data_ptr() + 4 * shift for t in cols]
            assert all(p % 16 == 4 * shift for p in ptr)
            st, hist = solver.solve_dedup_device(ptr[0], ptr[1], ptr[2], n, lengths, 3, d_mask.data_ptr(), d_tags=ptr[3],
                                                 d_qualities=ptr[4], pairs=pairs, complete_pairs=pairs,
                                                 d_dup_mask=d_dup.data_ptr(), hist_bins=BINS,
                                                 stream=torch.cuda.current_stream().cuda_stream)
            got, got_dup = d_mask.cpu().numpy(), d_dup.cpu().numpy()
            assert np.array_equal(got[:words].view(np.uint64), want[0]), (pairs, shift)
            assert np.array_equal(got_dup[:words].view(np.uint64), want[1]), (pairs, shift)
            assert (got[words:] == guard).all() and (got_dup[words:] == guard).all()
            assert {k: st[k] for k in STAT_KEYS} == {k: want[2][k] for k in STAT_KEYS} and np.array_equal(hist, want[3])


def test_random_stress(solver, oracle):
    for seed in range(200):
        rng = np.random.default_rng(9000 + seed)
        n_contigs = int(rng.integers(1, 4))
        lengths = rng.integers(60, 3000, size=n_contigs).astype(np.uint32)
        n = int(rng.integers(0, 3001))
        pairs = bool(seed % 2)
        n -= n % 2 if pairs else 0
        s, e, ids = duplicated_reads(rng, n, lengths, n_sites=int(rng.integers(1, 400)), unplaced=float(rng.random() * 0.2))
        tags = None if rng.random() < 0.3 else rng.integers(0, int(rng.choice([2, 5, 1 << 20])), size=n).astype(np.uint32)
        q = None if rng.random() < 0.3 else rng.integers(0, int(rng.choice([2, 61, 60000])), size=n).astype(np.uint32)
        check(solver, oracle, s, e, ids, lengths, int(rng.choice([1, 2, 5, 30])), tags=tags, q=q, pairs=pairs,
              complete=pairs and bool(rng.random() < 0.5), bins=int(rng.choice([0, 1, 4, 64])), what=f"seed {seed}")


def test_file_to_file(pkg, oracle, tmp_path):
    """downsample_bam(per_reference=True, dedup=True): no duplicate pair is written, the written records are the model's
    kept set (pair mode, tag = strand, quality = MAPQ, mates completed) and the TSV holds the model's statistics; with
    dedup=False the output is today's"""
    import bam_py
    rng = np.random.default_rng(31)
    n_pairs, n_sites = 200, 60
    site_pos = rng.integers(0, 2500, size=n_sites)
    site_mate = site_pos + rng.integers(50, 300, size=n_sites)
    site_rev = rng.random(n_sites) < 0.5                        # duplicated pairs on both strands
    pick = rng.integers(0, n_sites, size=n_pairs)
    names = np.repeat(np.arange(n_pairs), 2)
    first = np.tile([True, False], n_pairs)
    rev = np.where(first, site_rev[pick].repeat(2), ~site_rev[pick].repeat(2))
    flags = np.where(first, 0x41, 0x81) | np.where(rev, 0x10, 0)
    pos = np.where(first, site_pos[pick].repeat(2), site_mate[pick].repeat(2))
    mapq = rng.integers(0, 61, size=2 * n_pairs)
    order = rng.permutation(2 * n_pairs)
    z = np.zeros(2 * n_pairs, np.uint32)
    path = tmp_path / "dups.bam"
    pkg.write_synthetic_bam(path, 3000, names[order], flags[order], pos[order], mapq[order], z, z + 100, z, z)
    header, parsed, _ = bam_py.parse(path)
    cols = pkg.read_bam(path, per_reference=True, stratify="strand")
    n = cols["starts"].size
    assert n == 2 * n_pairs
    M = 3
    keep, dup, st, hist = dm.dedup(oracle, cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"], M,
                                   tags=cols["strata"], qualities=cols["qualities"], pairs=True, complete_pairs=True,
                                   hist_bins=pkg.DEDUP_REPORT_BINS)
    assert st["duplicate_units"] > 50 and 0 < keep.sum() <= n - dup.sum()
    out, tsv, plain_out = tmp_path / "out.bam", tmp_path / "dedup.tsv", tmp_path / "plain.bam"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, dedup=True, dedup_report=tsv)
    kept_ids = np.sort(cols["bam_ids"][np.flatnonzero(keep)].astype(np.int64))
    dup_ids = set(cols["bam_ids"][np.flatnonzero(dup)].astype(np.int64).tolist())
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == kept_ids.size == len(orecs)
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]
    assert not dup_ids & set(kept_ids.tolist())
    lines = [l.split("\t") for l in open(tsv).read().splitlines()]
    stats_rows = {l[0]: int(l[1]) for l in lines[1:1 + len(STAT_KEYS)]}
    assert lines[0] == ["#stat", "value"] and stats_rows == st
    assert lines[1 + len(STAT_KEYS)] == ["#size", "families"]
    bins = [(int(a), int(b)) for a, b in lines[2 + len(STAT_KEYS):]]
    assert bins == [(k + 1, int(hist[k])) for k in range(pkg.DEDUP_REPORT_BINS)]
    # dedup=False: the flow as it was
    w0 = pkg.downsample_bam("quasi-mcp-hip", path, plain_out, M, per_reference=True, dedup=False)
    plain = mr.oracle_by_contig(oracle, cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"], M)
    ids0 = np.sort(cols["bam_ids"][pkg.mask_to_indices(oracle.find_pairs(plain, n), n).astype(np.int64)].astype(np.int64))
    _, precs, _ = bam_py.parse(plain_out)
    assert w0 == ids0.size and [r["raw"] for r in precs] == [parsed[i]["raw"] for i in ids0.tolist()]


def test_cost_against_the_quality_pass(pkg, solver):
    """2^22 reads of one length over 8 contigs, MAPQ 0..60, strand tags, about 20 % duplicate units: the duplicate pass of
    read mode costs at most twice the quality pass of solve_quality_by_contig on the same reads (it builds a key with
    one more field, runs the same record radix and one segmented stage, and adds a compaction of four columns, the mask
    expansion and the histogram); pair mode at most twice read mode (a second sort on half as many records and an id
    scatter).  Medians of 5 after a warm-up."""
    rng = np.random.default_rng(41)
    n = 1 << 22
    lengths = np.full(8, 4_000_000, np.uint32)
    n_orig = int(n * 0.8)
    ids_o = rng.integers(0, 8, size=n_orig)
    s_o = rng.integers(0, 4_000_000 - 150, size=n_orig)
    t_o = rng.integers(0, 2, size=n_orig)
    src = np.concatenate([np.arange(n_orig), rng.integers(0, n_orig, size=n - n_orig)])
    rng.shuffle(src)
    s = s_o[src].astype(np.uint32)
    e = (s + 149).astype(np.uint32)
    ids = ids_o[src].astype(np.uint32)
    tags = t_o[src].astype(np.uint32)
    q = rng.integers(0, 61, size=n).astype(np.uint32)
    M = 10

    def median_ms(call, read):
        call()
        times = []
        for _ in range(5):
            call()
            times.append(read())
        return float(np.median(times))

    ms_quality = median_ms(lambda: solver.solve_quality_by_contig(s, e, ids, q, lengths, M),
                           lambda: solver.last_quality_stats.ms_quality)
    ms_read = median_ms(lambda: solver.solve_dedup(s, e, ids, lengths, M, tags=tags, qualities=q, hist_bins=64),
                        lambda: solver.last_dedup_stats.ms_dedup)
    st = solver.last_dedup_stats
    dup_share = st.duplicate_units / st.units
    ms_pair = median_ms(lambda: solver.solve_dedup(s, e, ids, lengths, M, tags=tags, qualities=q, pairs=True, hist_bins=64),
                        lambda: solver.last_dedup_stats.ms_dedup)
    print(f"ms_quality {ms_quality:.3f}  ms_dedup(read) {ms_read:.3f}  ms_dedup(pair) {ms_pair:.3f}  duplicates {dup_share:.3f}")
    assert 0.1 < dup_share < 0.3
    assert ms_read <= 2 * ms_quality, (ms_read, ms_quality)
    assert ms_pair <= 2 * ms_read, (ms_pair, ms_read)
