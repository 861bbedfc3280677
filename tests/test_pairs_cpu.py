"""Pair-aware downsampling, the parts that need no GPU: the model (tests/pair_model.py) gives whole pairs that are valid
at every stage, one stage is the plain by-contig selection + find_pairs, its two restatements agree, the overshoot
fixture keeps fewer reads than plain + completion; the host-side plan (genome-downsampler_amd/csrc/pair_plan.h) compiled
with g++ alone into tests/cpp/pair_plan_driver.cpp; the two entries are declared, listed and exported."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import multi_reference as mr
import pair_model as pairs
import profile_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QMCP_OK, QMCP_EINVAL, QMCP_ERANGE = 0, -1, -3


def random_pair_call(rng, n_contigs, max_reads_per_contig):
    """multi_reference.random_by_contig with an even number of reads, taken pairwise in its shuffled order: mates on
    other contigs and unplaced mates of placed reads come with the shuffle"""
    s, e, ids, lengths = mr.random_by_contig(rng, n_contigs, max_reads_per_contig=max_reads_per_contig)
    n = s.size - (s.size & 1)
    return s[:n], e[:n], ids[:n], lengths


def random_stages(rng, M):
    kind = int(rng.integers(0, 4))
    if kind == 0 or M == 1:
        return None
    if kind == 1:
        return [M]
    if kind == 2:
        return [1, M]
    k = int(rng.integers(1, min(M, 5) + 1))
    return sorted(rng.choice(np.arange(1, M), size=k - 1, replace=False).tolist()) + [M]


def test_every_stage_is_valid_and_holds_whole_pairs_on_200_random_calls(oracle):
    rng = np.random.default_rng(2024)
    staged_calls = 0
    for _ in range(200):
        s, e, ids, lengths = random_pair_call(rng, int(rng.integers(1, 4)), int(rng.integers(1, 120)))
        M = int(rng.choice([1, 2, 3, 7, 20]))
        stages = random_stages(rng, M)
        mask, selected, kept, sets = pairs.staged(oracle, s, e, ids, lengths, M, stages, fast=True)
        targets = pairs.default_stages(M) if stages is None else stages
        assert len(sets) == len(targets) == len(selected) == len(kept)
        before = np.zeros(s.size, bool)
        for T, S, n_sel, n_kept in zip(targets, sets, selected, kept):
            assert pairs.covers(s, e, ids, lengths, S, T), (M, stages, T)
            assert pairs.whole_pairs(S)
            assert not (before & ~S).any() and int(S.sum()) == n_kept >= int(before.sum()) + n_sel
            before = S
        assert np.array_equal(pm.unpack(mask, s.size), sets[-1])
        # an unplaced read is kept only as the mate of a kept placed read
        un = np.flatnonzero(ids == mr.NO_CONTIG)
        mate = un ^ 1
        assert not (sets[-1][un] & (ids[mate] == mr.NO_CONTIG)).any()
        staged_calls += len(targets) > 1
    assert staged_calls > 100


@pytest.mark.parametrize("seed, M", [(0, 1), (1, 2), (2, 7), (3, 20), (4, 200)])
def test_one_stage_is_the_plain_selection_and_find_pairs(oracle, seed, M):
    rng = np.random.default_rng(seed)
    s, e, ids, lengths = random_pair_call(rng, int(rng.integers(1, 5)), 600)
    want = pairs.plain(oracle, s, e, ids, lengths, M)
    for fast in (False, True):
        mask, selected, kept, _ = pairs.staged(oracle, s, e, ids, lengths, M, [M], fast=fast)
        assert np.array_equal(mask, want)
        assert selected == [int(pm.unpack(mr.oracle_by_contig(oracle, s, e, ids, lengths, M), s.size).sum())]
        assert kept == [int(pm.unpack(want, s.size).sum())]


@pytest.mark.parametrize("seed", range(6))
def test_the_two_restatements_agree_on_the_staged_result(oracle, seed):
    rng = np.random.default_rng(100 + seed)
    s, e, ids, lengths = random_pair_call(rng, int(rng.integers(1, 4)), 400)
    M = int(rng.choice([2, 3, 7, 20]))
    for stages in (None, [1, M], list(range(1, M + 1))[-16:]):
        slow = pairs.staged(oracle, s, e, ids, lengths, M, stages, fast=False)
        fast = pairs.staged(oracle, s, e, ids, lengths, M, stages, fast=True)
        assert np.array_equal(slow[0], fast[0]) and slow[1:3] == fast[1:3]


# (seed, L, M, depth) -> reads, plain + completion, |K_j| and |S_j| under the default stages: the model's counts
OVERSHOOT = [
    ((0, 20000, 20, 5), 13332, 4740, [1339, 375], [2530, 3270]),
    ((1, 20000, 20, 2), 5332, 4086, [1359, 471], [2380, 3246]),
    ((2, 10000, 50, 10), 33332, 6166, [1667, 328], [3230, 3880]),
    ((4, 20000, 20, 1.3), 3466, 3334, [1392, 657], [2198, 3186]),
]


@pytest.mark.parametrize("shape, n_reads, n_plain, selected, kept", OVERSHOOT)
def test_overshoot_fixture_default_stages_keep_fewer_reads_than_plain_and_completion(oracle, shape, n_reads, n_plain,
                                                                                      selected, kept):
    seed, L, M, depth = shape
    s, e, ids, lengths = pairs.overshoot(seed, L, M, depth)
    assert s.size == n_reads
    plain_bits = pm.unpack(pairs.plain(oracle, s, e, ids, lengths, M), s.size)
    mask, got_selected, got_kept, sets = pairs.staged(oracle, s, e, ids, lengths, M, fast=True)
    assert int(plain_bits.sum()) == n_plain and got_selected == selected and got_kept == kept
    assert got_kept[-1] < n_plain
    assert pairs.covers(s, e, ids, lengths, sets[-1], M) and pairs.whole_pairs(sets[-1])
    assert pairs.mean_kept_depth(s, e, sets[-1], L) < pairs.mean_kept_depth(s, e, plain_bits, L)
    # re-solving the plain completed set gives it back: the plain route cannot shed its surplus
    idx = np.flatnonzero(plain_bits)
    again = pm.unpack(pairs.plain(oracle, s[idx], e[idx], ids[idx], lengths, M), idx.size)
    assert again.all()


# ------------------------------------------------------------------------------------------ the plan header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pair_plan") / "pair_plan_driver"
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "pair_plan_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def ask(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = [dict(kv.split("=", 1) for kv in row.split()) for row in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def test_plan_default_schedule(driver):
    rows = ask(driver, [f"s {M} -1" for M in (1, 2, 3, 100, 101, 2**31 - 1)] + ["s 0 -1", f"s {2**31} -1"])
    assert [r["stages"] for r in rows[:6]] == ["1", "1,2", "2,3", "50,100", "51,101", f"{2**30},{2**31 - 1}"]
    assert all(int(r["rc"]) == QMCP_OK for r in rows[:6])
    assert [r["stages"] for r in rows[:4]] == [",".join(map(str, pairs.default_stages(M))) for M in (1, 2, 3, 100)]
    assert (int(rows[6]["rc"]), rows[6]["stages"]) == (QMCP_EINVAL, "")
    assert (int(rows[7]["rc"]), rows[7]["stages"]) == (QMCP_ERANGE, "")


def test_plan_accepts_rising_lists_and_names_the_entry_that_breaks_the_rule(driver):
    sixteen = list(range(1, 17))
    cases = [
        (100, [100], QMCP_OK, 0), (1, [1], QMCP_OK, 0), (20, [1, 20], QMCP_OK, 0), (20, [5, 10, 15, 20], QMCP_OK, 0),
        (16, sixteen, QMCP_OK, 0), (2**31 - 1, [7, 2**31 - 1], QMCP_OK, 0),
        (5, [], QMCP_EINVAL, 0),                            # no stage
        (17, list(range(1, 18)), QMCP_EINVAL, 0),           # 17 stages
        (5, [5, 5], QMCP_EINVAL, 1), (5, [6, 5], QMCP_EINVAL, 1), (9, [1, 4, 4, 9], QMCP_EINVAL, 2),
        (9, [1, 4, 3, 9], QMCP_EINVAL, 2),                  # a descending step
        (5, [0, 5], QMCP_EINVAL, 0), (5, [0], QMCP_EINVAL, 0),
        (20, [10, 19], QMCP_EINVAL, 1), (20, [10, 21], QMCP_EINVAL, 1), (20, [20, 21], QMCP_EINVAL, 1),   # last != M
        (0, [1], QMCP_EINVAL, 0),                           # M == 0
        (2**31, [2**31], QMCP_ERANGE, 0), (2**31 - 1, [5, 2**31, 2**31 - 1], QMCP_ERANGE, 1),
        (2**32 - 1, [5], QMCP_ERANGE, 0),
    ]
    rows = ask(driver, [f"s {M} {len(t)} " + " ".join(map(str, t)) for M, t, _, _ in cases])
    for (M, t, rc, bad), row in zip(cases, rows):
        assert (int(row["rc"]), int(row["bad"])) == (rc, bad), (M, t)
        assert row["stages"] == (",".join(map(str, t)) if rc == QMCP_OK else "")


def test_plan_candidate_offsets(driver):
    rows = ask(driver, [
        "n 3 0 10 10 25 | 0 4 4 9",        # the middle contig is empty and stays, with a zero-length run
        "n 1 0 7 | 0 7",                   # no read kept yet: every read is a candidate
        "n 2 0 4 9 | 0 0 0",               # every read kept already: no candidate
        "n 4 0 3 3 3 64 | 0 1 1 1 40",
        "n 2 0 5 9 | 1 3 5",               # ranks must start at 0
        "n 2 0 5 9 | 0 3 2",               # ... never fall
        "n 2 0 5 9 | 0 3 8",               # ... and give no contig more candidates than it has reads (5 of 4)
        "n 2 1 5 9 | 0 3 5",               # offsets must start at 0
    ])
    assert [r["next"] for r in rows[:4]] == ["0,4,4,9", "0,7", "0,0,0", "0,1,1,1,40"]
    assert all(int(r["rc"]) == QMCP_OK for r in rows[:4])
    assert all(int(r["rc"]) == QMCP_EINVAL and r["next"] == "" for r in rows[4:])
    rng = np.random.default_rng(12)
    lines, want = [], []
    for _ in range(40):
        n_contigs = int(rng.integers(1, 9))
        counts = rng.integers(0, 200, size=n_contigs)
        counts[rng.random(n_contigs) < 0.3] = 0
        offs = np.concatenate([[0], np.cumsum(counts)])
        rest = rng.random(int(offs[-1])) < rng.random()           # the complement of the kept set
        ranks = np.concatenate([[0], np.cumsum(rest)])[offs]
        lines.append(f"n {n_contigs} " + " ".join(map(str, offs)) + " | " + " ".join(map(str, ranks)))
        want.append(",".join(str(int(rest[:o].sum())) for o in offs))
    rows = ask(driver, lines)
    assert [r["next"] for r in rows] == want and all(int(r["rc"]) == QMCP_OK for r in rows)


# ------------------------------------------------------------------------------------------ the interface
def test_entries_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_pairs_host", "qmcp_hip_solve_pairs_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
    assert "#define QMCP_PAIR_MAX_STAGES 16" in text and pkg.PAIR_MAX_STAGES == 16
    assert "#define QMCP_HIP_ABI_VERSION 5" in text and pkg.abi_version() == 5
    assert hasattr(pkg.Solver, "solve_pairs") and hasattr(pkg.Solver, "solve_pairs_device")


def test_pair_stats_layout_matches_the_header(pkg, tmp_path):
    fields = ["n_selected", "n_kept", "capped_positions", "demand", "target", "sweeps", "ms_stage", "ms_pairs"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ '
           'printf("%zu", sizeof(qmcp_hip_pair_stats)); '
           + "".join(f'printf(" %zu", offsetof(qmcp_hip_pair_stats, {f})); ' for f in fields) + 'return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", str(exe)],
                         input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = pkg.PairStats
    assert got == [C.sizeof(P)] + [getattr(P, f).offset for f in fields]
