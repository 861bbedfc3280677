"""Reads of several references, the parts that need no GPU: the batch planner (genome-downsampler_amd/csrc/
by_contig_plan.h) compiled with g++ alone into tests/cpp/by_contig_plan_driver.cpp, and per-reference BAM ingest
(BamApiConfig::per_reference) on multi-reference files written by the independent writer in tests/bam_py.py."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import multi_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_READS, MAX_POSITIONS = 1 << 30, (1 << 31) - 2
QMCP_OK, QMCP_EINVAL, QMCP_ERANGE = 0, -1, -3


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("by_contig_plan") / "by_contig_plan_driver"
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "by_contig_plan_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def plan(driver, tables, max_reads=0, max_positions=0):
    """tables: [(reads per contig, lengths)] -> [(rc, bad contig or -1, [(first, count, first_read, reads, positions)])]"""
    lines = []
    for reads, lengths in tables:
        pairs = " ".join(f"{int(r)} {int(l)}" for r, l in zip(reads, lengths))
        lines.append(f"{max_reads} {max_positions} {len(reads)} {pairs}")
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    plans = []
    for row in out.stdout.splitlines():
        d = dict(kv.split("=", 1) for kv in row.split())
        batches = [tuple(int(x) for x in b.split(",")) for b in d["batches"].split(";") if b]
        plans.append((int(d["rc"]), int(d["bad"]), batches))
    assert len(plans) == len(tables)
    return plans


def check_partition(reads, lengths, batches, max_reads=MAX_READS, max_positions=MAX_POSITIONS):
    """every contig in exactly one batch, in id order, within the limits, and no batch could have taken the next
    contig (greedy)"""
    expect_first, expect_read = 0, 0
    for k, (first, count, first_read, n, positions) in enumerate(batches):
        assert first == expect_first and first_read == expect_read and count >= 1
        assert n == sum(int(r) for r in reads[first:first + count]) <= max_reads
        assert positions == sum(int(l) for l in lengths[first:first + count]) <= max_positions
        if k + 1 < len(batches):
            nxt = first + count
            assert n + int(reads[nxt]) > max_reads or positions + int(lengths[nxt]) > max_positions
        expect_first, expect_read = first + count, first_read + n
    assert expect_first == len(reads) and expect_read == sum(int(r) for r in reads)


def test_plan_limits_exactly_at_and_one_over(driver):
    tables = [
        ([MAX_READS], [1000]),                          # one contig at the read limit
        ([MAX_READS + 1], [1000]),                      # ... one over: QMCP_ERANGE naming it
        ([5], [MAX_POSITIONS]),                         # one contig at the position limit
        ([5], [MAX_POSITIONS + 1]),                     # ... one over
        ([MAX_READS - 10, 10], [100, 100]),             # two contigs that fill the read limit exactly: one batch
        ([MAX_READS - 10, 11], [100, 100]),             # ... one read over: two batches
        ([1, 1], [MAX_POSITIONS - 100, 100]),           # the position limit exactly: one batch
        ([1, 1], [MAX_POSITIONS - 100, 101]),           # ... one position over: two batches
        ([0, 7, MAX_READS + 1, 3], [10, 10, 10, 10]),   # the oversize contig is named, whatever surrounds it
    ]
    got = plan(driver, tables)
    assert got[0] == (QMCP_OK, -1, [(0, 1, 0, MAX_READS, 1000)])
    assert got[1][:2] == (QMCP_ERANGE, 0) and got[1][2] == []
    assert got[2] == (QMCP_OK, -1, [(0, 1, 0, 5, MAX_POSITIONS)])
    assert got[3][:2] == (QMCP_ERANGE, 0)
    assert got[4] == (QMCP_OK, -1, [(0, 2, 0, MAX_READS, 200)])
    assert got[5] == (QMCP_OK, -1, [(0, 1, 0, MAX_READS - 10, 100), (1, 1, MAX_READS - 10, 11, 100)])
    assert got[6] == (QMCP_OK, -1, [(0, 2, 0, 2, MAX_POSITIONS)])
    assert got[7] == (QMCP_OK, -1, [(0, 1, 0, 1, MAX_POSITIONS - 100), (1, 1, 1, 1, 101)])
    assert got[8][:2] == (QMCP_ERANGE, 2)


def test_plan_empty_contigs_and_a_whole_genome(driver):
    grch38_mb = [248, 242, 198, 190, 182, 171, 159, 145, 138, 134, 135, 133, 114, 107, 102, 90, 83, 80, 59, 64, 47,
                 51, 156, 57]
    lengths = [mb * 1_000_000 + 12_345 for mb in grch38_mb] + [16_569]   # + chrM
    reads = [0] * len(lengths)
    tables = [
        ([0, 0, 0], [100, 0, 5]),                       # no reads at all: still one batch holding every contig
        ([0], [0]),
        (reads, lengths),                               # 3.1 Gbp: more than one call's positions
        ([3, 0, 0, 4, 0], [10, 10, 0, 10, 10]),
    ]
    got = plan(driver, tables)
    assert got[0] == (QMCP_OK, -1, [(0, 3, 0, 0, 105)])
    assert got[1] == (QMCP_OK, -1, [(0, 1, 0, 0, 0)])
    assert got[2][0] == QMCP_OK and len(got[2][2]) == 2
    check_partition(reads, lengths, got[2][2])
    assert got[3] == (QMCP_OK, -1, [(0, 5, 0, 7, 40)])
    # no contigs: EINVAL
    out = subprocess.run([driver], input="0 0 0\n", capture_output=True, text=True, check=True)
    assert out.stdout.split()[0] == f"rc={QMCP_EINVAL}"


def test_plan_seeded_grid_every_contig_in_one_batch_in_id_order(driver):
    rng = np.random.default_rng(2024)
    tables, limits = [], []
    for _ in range(300):
        n = int(rng.integers(1, 60))
        max_reads = int(rng.integers(1, 5000))
        max_positions = int(rng.integers(1, 100_000))
        reads = rng.integers(0, max_reads + 1, size=n)
        lengths = rng.integers(0, max_positions + 1, size=n)
        reads[rng.random(n) < 0.2] = 0
        tables.append((reads, lengths))
        limits.append((max_reads, max_positions))
    # one driver run per limit pair would be slow: the limits ride along per line
    lines = []
    for (reads, lengths), (mr_, mp) in zip(tables, limits):
        lines.append(f"{mr_} {mp} {len(reads)} " + " ".join(f"{int(r)} {int(l)}" for r, l in zip(reads, lengths)))
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = out.stdout.splitlines()
    assert len(rows) == len(tables)
    for row, (reads, lengths), (mr_, mp) in zip(rows, tables, limits):
        d = dict(kv.split("=", 1) for kv in row.split())
        assert int(d["rc"]) == QMCP_OK and int(d["bad"]) == -1
        batches = [tuple(int(x) for x in b.split(",")) for b in d["batches"].split(";") if b]
        check_partition(reads, lengths, batches, mr_, mp)
    # and with one contig over a limit somewhere: QMCP_ERANGE naming the first such contig
    for _ in range(50):
        n = int(rng.integers(1, 40))
        reads = rng.integers(0, 100, size=n)
        lengths = rng.integers(0, 1000, size=n)
        bad = int(rng.integers(0, n))
        if rng.random() < 0.5:
            reads[bad] = 101
        else:
            lengths[bad] = 1001
        (rc, got_bad, batches), = plan(driver, [(reads, lengths)], 100, 1000)
        assert rc == QMCP_ERANGE and got_bad == bad and batches == []


# ---------------------------------------------------------------- per-reference ingest
REFS = [("chr1", 40_000), ("chr2", 25_000), ("chrX", 9_000), ("seg4", 3_000)]


@pytest.fixture(scope="module")
def multi_ref_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("multi_ref") / "multi.bam"
    header, parsed, ref_lengths = mr.write_multi_reference_bam(path, np.random.default_rng(5), REFS, 3000)
    return path, header, parsed, ref_lengths


def test_per_reference_ingest_keeps_each_reads_reference(multi_ref_file):
    pkg = importlib.import_module("genome-downsampler_amd")
    path, _, parsed, ref_lengths = multi_ref_file
    assert ref_lengths == [L for _, L in REFS]
    got = pkg.read_bam(path, per_reference=True)
    reads, ids, filtered = mr.expected_per_reference_reads(parsed)
    assert got["contig_lengths"].tolist() == ref_lengths
    assert got["contig_ids"].tolist() == ids.tolist()
    assert got["bam_ids"].tolist() == [r["bam_id"] for r in reads]
    assert got["filtered_out"].tolist() == filtered
    placed = ids != mr.NO_CONTIG
    assert placed.sum() < ids.size and (ids[placed] < len(REFS)).all() and len(set(ids[placed].tolist())) == len(REFS)
    # a placed read's coordinates are on its own reference
    starts = np.array([r["start"] for r in reads], dtype=np.int64)
    ends = np.array([r["end"] for r in reads], dtype=np.int64)
    assert got["starts"][placed].tolist() == starts[placed].tolist()
    assert got["ends"][placed].tolist() == ends[placed].tolist()
    lengths = np.array(ref_lengths)
    assert (ends[placed] < lengths[ids[placed]]).all()


def test_default_config_reads_a_multi_reference_file_as_today(multi_ref_file):
    """without per_reference the file is read as one contig (the first reference's length), exactly as before: the
    same pairing, the same columns, no contig ids"""
    pkg = importlib.import_module("genome-downsampler_amd")
    path, _, parsed, ref_lengths = multi_ref_file
    got = pkg.read_bam(path)
    reads, filtered = __import__("bam_py").pair_like_the_reference(parsed)
    assert "contig_ids" not in got and got["ref_genome_length"] == ref_lengths[0]
    assert got["bam_ids"].tolist() == [r["bam_id"] for r in reads]
    wrap = lambda v: np.array(v, dtype=np.int64).astype(np.uint32).tolist()
    assert got["starts"].tolist() == wrap([r["start"] for r in reads])
    assert got["ends"].tolist() == wrap([r["end"] for r in reads])
    assert got["qualities"].tolist() == [r["q"] for r in reads]
    assert got["filtered_out"].tolist() == filtered
    per_ref = pkg.read_bam(path, per_reference=True)
    for k in ("bam_ids", "starts", "ends", "qualities", "seq_lengths", "is_first", "filtered_out"):
        assert np.array_equal(per_ref[k], got[k]), k


def test_per_reference_refuses_amplicon_files(multi_ref_file, tmp_path):
    pkg = importlib.import_module("genome-downsampler_amd")
    bed = tmp_path / "panel.bed"
    bed.write_text("chr1\t0\t100\tamp_1_LEFT\t1\t+\nchr1\t300\t400\tamp_1_RIGHT\t1\t-\n")
    with pytest.raises(ValueError, match="amplicons"):
        pkg.read_bam(multi_ref_file[0], bed=bed, per_reference=True)
