"""The coverage ladder, the parts that need no GPU: the model on the oracle (tests/ladder_model.py) gives nested levels
that are each valid for the ORIGINAL reads; the host-side plan (genome-downsampler_amd/csrc/ladder_plan.h) compiled with
g++ alone into tests/cpp/ladder_plan_driver.cpp; the two entries are declared, listed and exported."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ladder_model as lm
import multi_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QMCP_OK, QMCP_EINVAL = 0, -1


@pytest.mark.parametrize("seed, coverages", [(0, [40, 12, 3, 1]), (1, [7, 1]), (2, [3]), (3, [200, 199]), (4, [50, 12, 3, 1])])
def test_model_levels_are_nested_and_valid_for_the_original_reads(oracle, seed, coverages):
    rng = np.random.default_rng(seed)
    s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(1, 5)), max_reads_per_contig=2500)
    levels = lm.ladder_levels(oracle, s, e, ids, lengths, coverages)
    assert levels.dtype == np.uint8 and levels.size == s.size and int(levels.max(initial=0)) <= len(coverages)
    assert not levels[ids == mr.NO_CONTIG].any()
    # level 0 is the plain by-contig selection; K_j = {levels > j} is nested by construction of the byte
    assert np.array_equal(lm.level_mask(levels, 0), mr.oracle_by_contig(oracle, s, e, ids, lengths, coverages[0]))
    kept = lm.n_kept(levels, len(coverages))
    assert all(a >= b for a, b in zip(kept, kept[1:]))
    for c in range(lengths.size):
        on = np.flatnonzero(ids == c)
        L = int(lengths[c])
        cov = oracle.cover(s[on], e[on], L)
        for j, M in enumerate(coverages):
            sub = on[levels[on] > j]
            out = oracle.cover(s[sub], e[sub], L)
            assert oracle.is_out_cover_valid(cov, out, M), f"contig {c}, level {j} (M = {M})"
            if cov.size and int(cov.max()) > 0:
                assert sub.size > 0          # a contig with reads keeps one at every level (M >= 1)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ladder_plan") / "ladder_plan_driver"
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "ladder_plan_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def ask(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = [dict(kv.split("=", 1) for kv in row.split()) for row in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def test_plan_accepts_falling_lists_and_names_the_level_that_breaks_the_rule(driver):
    sixteen = list(range(16, 0, -1))
    cases = [
        ([100], QMCP_OK, 0), ([1], QMCP_OK, 0), ([50, 12, 3, 1], QMCP_OK, 0), ([200, 199], QMCP_OK, 0),
        (sixteen, QMCP_OK, 0), ([0xFFFFFFFF, 5], QMCP_OK, 0),
        ([], QMCP_EINVAL, 0),                          # no level
        (list(range(17, 0, -1)), QMCP_EINVAL, 0),      # 17 levels
        ([5, 5], QMCP_EINVAL, 1), ([5, 6], QMCP_EINVAL, 1), ([9, 4, 4, 1], QMCP_EINVAL, 2), ([9, 4, 2, 3], QMCP_EINVAL, 3),
        ([0], QMCP_EINVAL, 0), ([3, 0], QMCP_EINVAL, 1),
    ]
    rows = ask(driver, [f"c {len(c)} " + " ".join(map(str, c)) for c, _, _ in cases] + ["c -1"])
    for (cov, rc, bad), row in zip(cases, rows):
        assert (int(row["rc"]), int(row["bad"])) == (rc, bad), cov
    assert (int(rows[-1]["rc"]), int(rows[-1]["bad"])) == (QMCP_EINVAL, 0)   # a NULL list


def test_plan_next_offsets_keep_empty_contigs_and_refuse_ranks_that_fit_no_mask(driver):
    rows = ask(driver, [
        "n 3 0 10 10 25 | 0 4 4 9",        # the middle contig is empty and stays, with a zero-length run
        "n 1 0 7 | 0 7",                   # every read kept
        "n 2 0 0 0 | 0 0 0",               # no read at all
        "n 4 0 3 3 3 64 | 0 1 1 1 40",
        "n 2 0 5 9 | 1 3 5",               # ranks must start at 0
        "n 2 0 5 9 | 0 3 2",               # ... never fall
        "n 2 0 5 9 | 0 3 8",               # ... and give no contig more reads than it had (5 of 4)
        "n 2 1 5 9 | 0 3 5",               # offsets must start at 0
    ])
    assert [r["next"] for r in rows[:4]] == ["0,4,4,9", "0,7", "0,0,0", "0,1,1,1,40"]
    assert all(int(r["rc"]) == QMCP_OK for r in rows[:4])
    assert all(int(r["rc"]) == QMCP_EINVAL and r["next"] == "" for r in rows[4:])


def test_plan_matches_the_model_step_on_random_masks(driver):
    rng = np.random.default_rng(11)
    lines, want = [], []
    for _ in range(60):
        n_contigs = int(rng.integers(1, 9))
        counts = rng.integers(0, 200, size=n_contigs)
        counts[rng.random(n_contigs) < 0.3] = 0
        offs = np.concatenate([[0], np.cumsum(counts)])
        keep = rng.random(int(offs[-1])) < rng.random()
        ranks = np.concatenate([[0], np.cumsum(keep)])[offs]
        lines.append(f"n {n_contigs} " + " ".join(map(str, offs)) + " | " + " ".join(map(str, ranks)))
        want.append(",".join(str(int(keep[:o].sum())) for o in offs))
    rows = ask(driver, lines)
    assert [r["next"] for r in rows] == want and all(int(r["rc"]) == QMCP_OK for r in rows)


def test_entries_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_ladder_host", "qmcp_hip_solve_ladder_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
    assert "#define QMCP_LADDER_MAX_LEVELS 16" in text and pkg.LADDER_MAX_LEVELS == 16
    assert pkg.abi_version() == 5


def test_ladder_stats_layout_matches_the_header(pkg, tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ '
           'printf("%zu %zu %zu %zu\\n", sizeof(qmcp_hip_ladder_stats), offsetof(qmcp_hip_ladder_stats, n_kept), '
           'offsetof(qmcp_hip_ladder_stats, ms_level), offsetof(qmcp_hip_ladder_stats, ms_ladder)); return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", str(exe)],
                         input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    L = pkg.LadderStats
    assert got == [C.sizeof(L), L.n_kept.offset, L.ms_level.offset, L.ms_ladder.offset]


def test_ladder_mask_is_the_levels_bytes_thresholded(pkg):
    levels = np.array([0, 3, 1, 2, 0, 3] * 23, dtype=np.uint8)     # 138 reads: more than two words
    for j in range(3):
        m = pkg.ladder_mask(levels, j)
        assert m.dtype == np.uint64 and m.size == pkg.mask_words(levels.size)
        assert np.array_equal(pkg.mask_to_indices(m, levels.size), np.flatnonzero(levels > j))
        assert np.array_equal(m, lm.level_mask(levels, j))
    assert pkg.ladder_mask(np.zeros(0, np.uint8), 0).size == 0
