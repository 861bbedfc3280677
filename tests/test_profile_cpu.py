"""The coverage profile without a device: the model of tests/profile_model.py tied to the oracle, to brute force and to
the target model; the host cap table (genome-downsampler_amd/csrc/cap_table.h through tests/cpp/cap_table_driver.cpp);
the bedGraph parser; the C ABI (header, exports, struct layout, version)."""
import ctypes as C
import os
import subprocess

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
