"""The two pure steps of the solver adapter (genome-downsampler_amd/host/include/qmcp-solver/adapter_columns.hpp),
compiled with g++ alone into tests/cpp/adapter_columns_driver.cpp: the 64-bit coordinate columns narrowed to uint32 -- an
unplaced read goes over as 0 / 0 whatever its coordinates are, the first placed read with a coordinate above 2^32 - 1 is
reported and nothing ends the process -- and a kept list turned into a keep mask."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_CONTIG = 0xFFFFFFFF
UNTOUCHED = 0xDEADBEEF
BIG, HUGE = 1 << 32, 1 << 40


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("adapter_columns") / "adapter_columns_driver"
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "host", "include"),
                          os.path.join(ROOT, "tests", "cpp", "adapter_columns_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def ask(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = [dict(kv.split("=", 1) for kv in row.split()) for row in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def column(text):
    return np.array([int(x) for x in text.split(",") if x], dtype=np.uint64)


# (name, starts, ends, contig ids or None) -- the smallest shapes at which the narrowing can go wrong
NARROW_CASES = [
    ("no reads", [], [], []),
    ("no reads, no ids", [], [], None),
    ("all placed", [0, 5, 17], [9, 5, 4000], [0, 1, 0]),
    ("an unplaced read with huge coordinates", [3, BIG, 8], [4, HUGE, 9], [0, NO_CONTIG, 1]),
    ("a placed start of 2^32 - 1", [BIG - 1, 1], [BIG - 1, 2], [0, 0]),
    ("a placed start of 2^32", [1, BIG, 2], [1, BIG, 2], [0, 0, 0]),
    ("a placed end of 2^32 with a small start", [1, 7, 2], [1, BIG, 2], [0, 1, 0]),
    ("two bad reads", [1, HUGE, 2, BIG], [1, HUGE, 2, BIG], [0, 0, 0, 0]),
    ("a bad read behind an unplaced one with the same coordinates", [BIG, BIG], [BIG, BIG], [NO_CONTIG, 0]),
    ("null ids, one coordinate too large", [1, 2, 3], [1, BIG, 3], None),
    ("null ids, all placed", [1, 2, 3], [1, 2, BIG - 1], None),
    ("unplaced first", [9, 1, 2], [9, 1, 2], [NO_CONTIG, 0, 0]),
    ("unplaced last", [1, 2, 9], [1, 2, 9], [0, 0, NO_CONTIG]),
    ("unplaced in the middle", [1, 9, 9, 2, 3], [1, 9, 9, 2, 3], [0, NO_CONTIG, NO_CONTIG, 1, 0]),
    ("all unplaced", [BIG, 9], [HUGE, 9], [NO_CONTIG, NO_CONTIG]),
]


def test_narrowing_is_the_rule_and_reports_the_first_bad_placed_read(driver):
    lines = []
    for _, s, e, ids in NARROW_CASES:
        reads = zip(s, e) if ids is None else zip(s, e, ids)
        lines.append(" ".join(["N", "0" if ids is None else "1", str(len(s))] + [str(x) for r in reads for x in r]))
    for (name, s, e, ids), row in zip(NARROW_CASES, ask(driver, lines)):
        s, e = np.array(s, dtype=np.uint64), np.array(e, dtype=np.uint64)
        n = s.size
        placed = np.ones(n, bool) if ids is None else np.array(ids, dtype=np.uint64) != NO_CONTIG
        wrong = np.flatnonzero(placed & ((s > BIG - 1) | (e > BIG - 1)))
        bad = int(wrong[0]) if wrong.size else n
        assert int(row["bad"]) == bad, name
        assert int(row["placed"]) == int(placed[:bad].sum()), name
        got_s, got_e = column(row.get("starts", "")), column(row.get("ends", ""))
        assert got_s.size == n and got_e.size == n, name
        assert np.array_equal(got_s[:bad], np.where(placed, s, 0)[:bad]), name
        assert np.array_equal(got_e[:bad], np.where(placed, e, 0)[:bad]), name
        assert np.all(got_s[bad:] == UNTOUCHED) and np.all(got_e[bad:] == UNTOUCHED), name  # (it stops at the bad read)


# (n, kept): every size around a word boundary; an index >= n, a repeated index, an unsorted list
MASK_CASES = [(n, kept) for n in (0, 1, 63, 64, 65, 130) for kept in (
    [], list(range(n)), list(range(0, n, 3)), [n - 1, 0, n // 2, 0, n - 1] if n else [0, 5], [n, n + 64, 1 << 40] + [0] * min(n, 1),
    [129, 64, 63, 0, 65, 64, 128, 1])]


def test_keep_mask_of_sets_the_bits_of_the_indices_below_n(driver):
    lines = [" ".join(["M", str(n), str(len(kept))] + [str(i) for i in kept]) for n, kept in MASK_CASES]
    for (n, kept), row in zip(MASK_CASES, ask(driver, lines)):
        bits = np.zeros(((n + 63) // 64) * 64, bool)
        bits[np.array([i for i in kept if i < n], dtype=np.intp)] = True
        want = np.packbits(bits, bitorder="little").view("<u8") if n else np.zeros(0, np.uint64)
        got = np.array([int(x, 16) for x in row.get("words", "").split(",") if x], dtype=np.uint64)
        assert np.array_equal(got, want), (n, kept)
