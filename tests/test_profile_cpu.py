"""The coverage profile without a device: the model of tests/profile_model.py tied to the oracle, to brute force and to
the target model; its second restatement from sorted events (fast_select) and the translation helper tied to the first;
the host cap table (genome-downsampler_amd/csrc/cap_table.h through tests/cpp/cap_table_driver.cpp);
the bedGraph parser; the C ABI (header, exports, struct layout, version)."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import profile_model as pm
import target_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QMCP_EINVAL, QMCP_ERANGE = -1, -3
NAMES = ("qmcp_hip_solve_profile_host", "qmcp_hip_solve_profile_device")


def tiny_instance(rng, max_reads=11, max_positions=12):
    L = int(rng.integers(1, max_positions + 1))
    n = int(rng.integers(1, max_reads + 1))
    s = rng.integers(0, L, size=n)
    e = np.minimum(s + rng.integers(0, L, size=n), L - 1)
    return s.astype(np.uint32), e.astype(np.uint32), L


def run_caps(rng, L, max_cap):
    """caps 0..max_cap in runs"""
    cap = np.zeros(L, np.int64)
    p = 0
    while p < L:
        run = int(rng.integers(1, 5))
        cap[p:p + run] = int(rng.integers(0, max_cap + 1))
        p += run
    return cap


def test_model_equals_oracle_when_every_cap_is_M(oracle):
    rng = np.random.default_rng(20261)
    for _ in range(300):
        L = int(rng.integers(1, 120))
        n = int(rng.integers(1, 150))
        s = rng.integers(0, L, size=n)
        e = np.minimum(s + rng.integers(0, 40, size=n), L - 1)
        M = int(rng.integers(1, 9))
        s, e = s.astype(np.uint32), e.astype(np.uint32)
        want = oracle.solve(s, e, L, M)
        got = pm.pack(pm.select(s, e, np.full(L, M, np.int64)))
        assert np.array_equal(got, want)


def test_model_is_valid_and_minimum_under_random_caps():
    rng = np.random.default_rng(20262)
    for _ in range(1200):
        s, e, L = tiny_instance(rng)
        cap = run_caps(rng, L, 5)
        kept = pm.select(s, e, cap)
        assert pm.is_valid(s, e, cap, kept)
        assert int(kept.sum()) == pm.brute_minimum(s, e, cap)
        # a read that lies wholly in cap-0 positions is never kept
        for i in np.flatnonzero(kept).tolist():
            assert cap[s[i]:e[i] + 1].max() > 0


def test_model_count_equals_target_model(oracle):
    rng = np.random.default_rng(20263)
    for _ in range(60):
        lengths = rng.integers(1, 200, size=int(rng.integers(1, 4))).astype(np.uint32)
        n = int(rng.integers(1, 200))
        ids = rng.integers(0, lengths.size, size=n).astype(np.uint32)
        s = (rng.random(n) * lengths[ids]).astype(np.int64)
        e = np.minimum(s + rng.integers(0, 50, size=n), lengths[ids].astype(np.int64) - 1)
        s, e = s.astype(np.uint32), e.astype(np.uint32)
        M = int(rng.integers(1, 6))
        offs, r0, r1, caps = pm.random_regions(rng, lengths, 1)
        caps[:] = M
        mask = pm.expected_mask(s, e, ids, lengths, 0, offs, r0, r1, caps)
        want, _ = tm.expected_mask(oracle, s, e, ids, lengths, offs, r0, r1, M)
        count = lambda m: int(pm.unpack(m, n).sum())
        assert count(mask) == count(want)



# ---------------------------------------------------------------------------------------------- the model from sorted events
def test_fast_model_equals_the_model_bit_for_bit():
    """2 000 instances drawn as test_gpu_profile.random_instance draws them (1..4 contigs on <= 700 positions, <= 400
    reads of spans up to 3 | 40 | 130 | 500, 5 % unplaced, regions at multiples of 64 and +-1 with caps 0..12, some
    clipped).  What the draw has to contain is counted: cap-0 runs longer than the longest read, caps far above the
    coverage, and reads that tie in end and start (decided by the index)"""
    from test_gpu_profile import random_instance
    rng = np.random.default_rng(20265)
    zero_runs = high_caps = ties = kept_some = 0
    for _ in range(2000):
        s, e, ids, lengths, default, offs, r0, r1, caps = inst = random_instance(rng)
        want = pm.expected_mask(*inst)
        assert np.array_equal(pm.fast_expected_mask(*inst), want), (lengths.tolist(), s.size)
        placed = ids != pm.NO_CONTIG
        span_max = int((e.astype(np.int64) - s + 1).max())
        zero_runs += bool(np.any((caps == 0) & (r1.astype(np.int64) - r0 + 1 > span_max)))
        high_caps += bool(np.any(caps == 100_000))
        cells = (ids[placed].astype(np.int64) << 40) | (s[placed].astype(np.int64) << 20) | e[placed]
        ties += np.unique(cells).size < cells.size
        kept_some += bool(want.any())
    assert zero_runs > 600 and high_caps > 400 and ties > 1000 and kept_some > 1500, (zero_runs, high_caps, ties, kept_some)


def test_fast_model_is_minimum_under_random_caps():
    rng = np.random.default_rng(20262)                       # the instances of test_model_is_valid_and_minimum_under_random_caps
    for _ in range(1200):
        s, e, L = tiny_instance(rng)
        cap = run_caps(rng, L, 5)
        offs, r0, r1, caps = pm.regions_of(cap)
        kept = pm.fast_select(s, e, L, 77, pm.clipped_regions(L, r0, r1, caps))   # (the regions tile the contig)
        assert pm.is_valid(s, e, cap, kept)
        assert int(kept.sum()) == pm.brute_minimum(s, e, cap)


def test_translation_helper_changes_nothing():
    """random instances, and instances whose reads sit in a few islands of long contigs (still short enough for the
    model with an array per position): the mask, demand and capped positions of the compact instance are the original's,
    under both models; the compact contigs are no longer than the reads' islands and the gaps between them"""
    from test_gpu_profile import random_instance
    rng = np.random.default_rng(20266)
    shrunk = 0
    for k in range(400):
        if k % 2:
            s, e, ids, lengths, default, offs, r0, r1, caps = random_instance(rng)
        else:
            n_contigs = int(rng.integers(1, 4))
            lengths = rng.integers(5_000, 30_000, size=n_contigs).astype(np.uint32)
            n = int(rng.integers(1, 200))
            ids = rng.integers(0, n_contigs, size=n).astype(np.uint32)
            Ls = lengths[ids].astype(np.int64)
            anchors = rng.integers(0, 30_000, size=(n_contigs, 3))                # three islands per contig, the
            anchors[:, 0], anchors[:, 2] = 0, 30_000                              # first and last at the contig's ends
            span = rng.integers(1, 120, size=n)
            s = np.clip(anchors[ids, rng.integers(0, 3, size=n)] + rng.integers(-100, 100, size=n), 0, Ls - span)
            e = s + span - 1
            ids[rng.random(n) < 0.05] = pm.NO_CONTIG
            offs, r0, r1, caps = pm.random_regions(rng, lengths, 6, max_regions=20)
            default = int(rng.integers(0, 7))
            s, e = s.astype(np.uint32), e.astype(np.uint32)
        c = pm.compact(s, e, ids, lengths, offs, r0, r1, caps)
        cs, ce, cids, clen = c[:4]
        assert np.array_equal(cids, ids) and np.all(clen <= np.maximum(lengths, 1))
        assert np.array_equal(ce.astype(np.int64) - cs, e.astype(np.int64) - s)
        shrunk += int(clen.sum()) * 4 < int(lengths.sum())
        want = pm.expected_mask(s, e, ids, lengths, default, offs, r0, r1, caps)
        assert np.array_equal(pm.expected_mask(cs, ce, cids, clen, default, *c[4:]), want), k
        assert np.array_equal(pm.fast_expected_mask(cs, ce, cids, clen, default, *c[4:]), want), k
        assert np.array_equal(pm.fast_expected_mask(s, e, ids, lengths, default, offs, r0, r1, caps), want), k
        assert pm.demand_and_capped(cs, ce, cids, clen, default, *c[4:]) == \
            pm.demand_and_capped(s, e, ids, lengths, default, offs, r0, r1, caps), k
    assert shrunk > 100


def test_form_of_at_every_threshold():
    """the forms as kernels/profile.inc.hip's launchers and api/profile.inc.hip choose them: B from (max_span + 127) / 64
    (5 takes the form of 6, 7 that of 8, beyond 8 the plain walk), K = 4 up to 64 workgroups, rings in global memory
    beyond spans of 16 383, 64-bit keys from 5 sort passes, windows of at least 64 longest spans and none from 256 contigs"""
    st = lambda span, passes=4, ltot=1000: types.SimpleNamespace(max_span=span, sort_passes=passes, total_length=ltot)
    want = {1: 2, 64: 2, 65: 3, 128: 3, 129: 4, 192: 4, 193: 6, 320: 6, 321: 8, 448: 8}
    for span, b in want.items():
        assert pm.form_of(st(span), 3, -1) == ("rec", "reg", b, 4)
        assert pm.form_of(st(span, 5), 65, -1) == ("k64", "reg", b, 1)
    assert pm.form_of(st(449), 3, -1) == ("rec", "plain", "lds")
    assert pm.form_of(st(16383, 6), 3, 1) == ("k64", "plain", "lds")
    assert pm.form_of(st(16384), 3, 1) == ("rec", "plain", "global")
    assert pm.form_of(st(100), 64, -1)[3] == 4 and pm.form_of(st(100), 65, -1)[3] == 1
    assert pm.stretch_windows(2 * 6400 - 1, 100, 3) == 0 and pm.stretch_windows(2 * 6400, 100, 3) == 2
    assert pm.stretch_windows(1 << 30, 100, 255) == 3840 and pm.stretch_windows(1 << 30, 100, 256) == 0
    assert pm.form_of(st(100, 4, 61 * 6400), 3, 1)[3] == 4 and pm.form_of(st(100, 4, 62 * 6400), 3, 1)[3] == 1
    assert pm.form_of(st(100, 4, 62 * 6400), 3, -1)[3] == 4
    assert (pm.need_form(4096), pm.need_form(4097)) == ("need_lds", "need_global")
    with pytest.raises(ValueError):
        pm.form_of(st(100), 3, 0)


# ---------------------------------------------------------------------------------------------- the host table
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cap_table") / "cap_table_driver"
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "cap_table_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def table(driver, lengths, offs, r0, r1, caps, first=0, count=None, mode="ok"):
    count = len(lengths) - first if count is None else count
    tok = ["table", mode, len(lengths), len(r0), first, count] + list(lengths) + list(offs) + list(r0) + list(r1) + list(caps)
    out = subprocess.run([driver], input=" ".join(str(t) for t in tok) + "\n", capture_output=True, text=True, check=True)
    rows = out.stdout.splitlines()
    rc = int(rows[0].split()[1])
    if rc != 0:
        return rc, None, None, None
    f = rows[1].split()
    summary = {f[0]: int(f[1]), f[2]: int(f[3]), f[4]: int(f[5]), f[6]: int(f[7])}
    triples = lambda row: [tuple(int(x) for x in row[i:i + 3]) for i in range(0, len(row), 3)]
    contigs = [triples(r.split()[3:]) for r in rows[2:2 + len(lengths)]]
    return rc, summary, contigs, triples(rows[2 + len(lengths)].split()[2:])


def test_cap_table_clips_drops_and_sorts(driver):
    lengths = [100, 50, 0]
    # contig 0: out of order, one clipped (90..140 -> 90..99), one dropped (begins at 100); contig 1: one ending exactly at
    # the last position; contig 2 (length 0): its region is dropped
    rc, summary, contigs, batch = table(driver, lengths, [0, 4, 5, 6], [90, 10, 100, 40, 20, 0], [140, 19, 120, 40, 49, 5],
                                        [7, 3, 9, 0, 2, 4])
    assert rc == 0
    assert contigs == [[(10, 19, 3), (40, 40, 0), (90, 99, 7)], [(20, 49, 2)], []]
    assert summary == {"regions_in": 6, "regions_used": 4, "positions": 10 + 1 + 10 + 30, "max_cap": 7}
    assert batch == [(10, 19, 3), (40, 40, 0), (90, 99, 7), (120, 149, 2)]


def test_cap_table_batch_offsets_across_a_batch_boundary(driver):
    lengths = [100, 50, 70, 30]
    offs, r0, r1, caps = [0, 1, 2, 4, 5], [5, 0, 60, 0, 29], [9, 49, 69, 9, 29], [1, 2, 3, 4, 5]
    _, _, _, first_two = table(driver, lengths, offs, r0, r1, caps, first=0, count=2)
    _, _, _, last_two = table(driver, lengths, offs, r0, r1, caps, first=2, count=2)
    assert first_two == [(5, 9, 1), (100, 149, 2)]
    assert last_two == [(0, 9, 4), (60, 69, 3), (99, 99, 5)]      # positions restart at the batch's first contig


def test_cap_table_empty_and_adjacent(driver):
    rc, summary, contigs, batch = table(driver, [10, 10], [0, 0, 0], [], [], [])
    assert rc == 0 and summary["regions_used"] == 0 and contigs == [[], []] and batch == []
    rc, summary, _, _ = table(driver, [10], [0, 0], [], [], [], mode="null_offsets")          # NULL offsets: no regions
    assert rc == 0 and summary["regions_in"] == 0
    rc, _, contigs, _ = table(driver, [10], [0, 2], [0, 5], [4, 9], [1, 2])                   # adjacent stays two regions
    assert rc == 0 and contigs == [[(0, 4, 1), (5, 9, 2)]]


@pytest.mark.parametrize("lengths,offs,r0,r1,caps,mode,want", [
    ([100], [0, 2], [10, 20], [20, 30], [1, 1], "ok", QMCP_EINVAL),              # share position 20
    ([100], [0, 2], [95, 99], [200, 300], [1, 1], "ok", QMCP_EINVAL),            # overlap only after clipping
    ([100], [0, 1], [9], [3], [1], "ok", QMCP_EINVAL),                           # start > end
    ([100], [1, 1], [], [], [], "ok", QMCP_EINVAL),                              # offsets do not start at 0
    ([100, 100], [0, 2, 1], [1, 5], [2, 6], [1, 1], "ok", QMCP_EINVAL),          # offsets decrease
    ([100], [0, 1], [1], [2], [1], "null_regions", QMCP_EINVAL),
    ([100], [0, 1], [1], [2], [1], "null_lengths", QMCP_EINVAL),
    ([100], [0, 1], [1], [2], [1 << 31], "ok", QMCP_ERANGE),
])
def test_cap_table_errors(driver, lengths, offs, r0, r1, caps, mode, want):
    assert table(driver, lengths, offs, r0, r1, caps, mode=mode)[0] == want


def test_cap_table_overlap_in_another_contig_is_fine(driver):
    rc, _, contigs, _ = table(driver, [100, 100], [0, 1, 2], [10, 10], [20, 20], [1, 2])
    assert rc == 0 and contigs == [[(10, 20, 1)], [(10, 20, 2)]]


# ---------------------------------------------------------------------------------------------- bedGraph
REFS = ["chr1", "chr2", "chrM"]


def _file(tmp_path, text, name="caps.bedgraph"):
    path = tmp_path / name
    path.write_text(text)
    return path


def test_profile_from_bedgraph(pkg, tmp_path):
    path = _file(tmp_path, "track type=bedGraph\n# comment\n\n"
                           "chr2\t100\t200\t7\n"
                           "chr1\t0\t10\t3\n"
                           "chr1 5 8 9\n"                      # a later line wins inside an earlier one
                           "chr1\t20\t30\t4\n"
                           "chr1\t30\t40\t4\n")                # neighbours with one cap are joined
    offs, r0, r1, caps = pkg.profile_from_bedgraph(path, REFS)
    assert offs.dtype == r0.dtype == r1.dtype == caps.dtype == np.uint32
    assert offs.tolist() == [0, 4, 5, 5]
    assert list(zip(r0.tolist(), r1.tolist(), caps.tolist())) == \
        [(0, 4, 3), (5, 7, 9), (8, 9, 3), (20, 39, 4), (100, 199, 7)]     # half-open -> inclusive
    # the earlier line loses where they overlap, whatever their order by position
    offs, r0, r1, caps = pkg.profile_from_bedgraph(_file(tmp_path, "chr1\t5\t15\t1\nchr1\t0\t10\t2\n", "b.bedgraph"), REFS)
    assert list(zip(r0.tolist(), r1.tolist(), caps.tolist())) == [(0, 9, 2), (10, 14, 1)]
    empty = pkg.profile_from_bedgraph(_file(tmp_path, "# nothing\n", "e.bedgraph"), REFS)
    assert empty[0].tolist() == [0, 0, 0, 0] and all(a.size == 0 for a in empty[1:])


@pytest.mark.parametrize("text,needle", [
    ("chr3\t1\t2\t5\n", "chr3"),
    ("chr1\t1\t2\n", "chrom, start, end and cap"),
    ("chr1\t1\t2\t1.5\n", "not an integer"),
    ("chr1\t1\t2\t-1\n", "not in"),
    ("chr1\t1\t2\t2147483648\n", "not in"),
    ("chr1\t9\t9\t1\n", "empty"),
])
def test_profile_from_bedgraph_errors(pkg, tmp_path, text, needle):
    with pytest.raises(ValueError) as ex:
        pkg.profile_from_bedgraph(_file(tmp_path, "chr1\t1\t5\t2\n" + text), REFS)
    assert needle in str(ex.value) and ":2:" in str(ex.value)


def test_flattened_bedgraph_passes_the_cap_table(pkg, tmp_path, driver):
    rng = np.random.default_rng(20264)
    rows = []
    for _ in range(200):
        a = int(rng.integers(0, 900))
        rows.append(f"chr1\t{a}\t{a + int(rng.integers(1, 120))}\t{int(rng.integers(0, 9))}")
    offs, r0, r1, caps = pkg.profile_from_bedgraph(_file(tmp_path, "\n".join(rows) + "\n"), ["chr1"])
    want = np.full(1100, -1, np.int64)
    for row in rows:
        _, a, b, c = row.split("\t")
        want[int(a):int(b)] = int(c)
    got = np.full(1100, -1, np.int64)
    for a, b, c in zip(r0.tolist(), r1.tolist(), caps.tolist()):
        assert np.all(got[a:b + 1] == -1)
        got[a:b + 1] = c
    assert np.array_equal(got, want)
    assert table(driver, [1100], offs.tolist(), r0.tolist(), r1.tolist(), caps.tolist())[0] == 0


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_the_profile_entries(pkg):
    header = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in header
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
    assert "typedef struct qmcp_hip_profile_stats" in header
    assert "#define QMCP_HIP_ABI_VERSION 5" in header
    assert pkg.abi_version() == 5
    for field in ("positions_in_regions", "capped_positions", "demand", "regions_in", "regions_used", "ms_profile"):
        assert field in header.split("typedef struct qmcp_hip_profile_stats")[1].split("}")[0]
    assert C.sizeof(pkg.ProfileStats) == 40


def test_profile_needs_per_reference_and_refuses_other_modes(pkg, tmp_path):
    caps = _file(tmp_path, "chr1\t0\t10\t3\n")
    args = ("quasi-mcp-hip", "in.bam", str(tmp_path / "out.bam"), 10)
    with pytest.raises(ValueError, match="per_reference"):
        pkg.downsample_bam(*args, profile=caps)
    for extra in ({"targets": "t.bed"}, {"report": "r.tsv"}, {"ladder": [5], "ladder_out": "x{M}.bam"},
                  {"stratify": "strand"}, {"dedup": True}):
        with pytest.raises(ValueError):
            pkg.downsample_bam(*args, per_reference=True, profile=caps, **extra)
    with pytest.raises(ValueError, match="amplicon"):
        pkg.downsample_bam(*args, per_reference=True, profile=caps, bed="a.bed", amplicons_by_reference=True)
    with pytest.raises(ValueError, match="quality"):
        pkg.downsample_bam("quasi-mcp-hip-quality", *args[1:], per_reference=True, profile=caps)
