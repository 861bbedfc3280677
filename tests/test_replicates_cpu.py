"""Disjoint replicates, the parts that need no GPU: the model on the oracle (tests/replicates_model.py) gives disjoint
replicates that each meet the coverage guarantee; the host-side plan (genome-downsampler_amd/csrc/replicates_plan.h)
compiled with g++ alone into tests/cpp/replicates_plan_driver.cpp; the two entries, the flags and the struct are
declared, listed and exported, and refuse bad arguments before they look at a context."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import multi_reference as mr
import replicates_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QMCP_OK, QMCP_EINVAL, QMCP_ERANGE = 0, -1, -3
COVERAGE_LISTS = [[5, 5, 5, 5], [3] * 6, [30, 10, 30], [1, 1, 1], [8], [2, 40]]


def case(seed):
    rng = np.random.default_rng(7000 + seed)
    s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(1, 6)), max_reads_per_contig=1200)
    if s.size % 2:
        s, e, ids = s[:-1], e[:-1], ids[:-1]            # whole pairs need an even number of reads
    return s, e, ids, lengths, COVERAGE_LISTS[seed % len(COVERAGE_LISTS)]


@pytest.mark.parametrize("seed", range(48))
def test_model_replicates_are_disjoint_and_meet_the_guarantee(oracle, seed):
    s, e, ids, lengths, cov = case(seed)
    placed = ids != mr.NO_CONTIG
    for flags in (0, rm.WHOLE_PAIRS):
        labels, info = rm.replicate_labels(oracle, s, e, ids, lengths, cov, flags)
        assert labels.dtype == np.uint8 and labels.size == s.size and int(labels.max(initial=0)) <= len(cov)
        assert not labels[~placed].any()
        # one byte per read: a read lies in at most one replicate; the counts add up to what was offered
        assert info["n_kept"] == [int((labels == r).sum()) for r in range(1, len(cov) + 1)]
        assert info["n_offered"][0] == int(placed.sum())
        for r in range(1, len(cov)):
            assert info["n_offered"][r] == info["n_offered"][r - 1] - info["n_kept"][r - 1]
        assert rm.guarantee_holds(labels, s, e, ids, lengths, cov), f"seed {seed}, flags {flags}: {cov}"
        if flags:
            both = placed[0::2] & placed[1::2]
            assert np.array_equal(labels[0::2][both], labels[1::2][both])     # pairs move together
        else:
            assert not any(info["n_mates"])
            # replicate r is the plain selection of what was left
            left = placed.copy()
            for r, M in enumerate(cov, start=1):
                idx = np.flatnonzero(left)
                want = mr.oracle_by_contig(oracle, s[idx], e[idx], ids[idx], lengths, M)
                got = rm.replicate_mask(labels[idx], r)
                assert np.array_equal(got, want)
                left &= labels != r


def test_one_replicate_is_the_plain_mask(oracle):
    for seed in (2, 9, 17):
        s, e, ids, lengths, _ = case(seed)
        for c in (1, 8, 50):
            labels, info = rm.replicate_labels(oracle, s, e, ids, lengths, [c])
            assert np.array_equal(rm.replicate_mask(labels, 1), mr.oracle_by_contig(oracle, s, e, ids, lengths, c))


def test_sixteen_deep_replicates_run_dry(oracle):
    s, e, ids, lengths = mr.random_by_contig(np.random.default_rng(1), 3)
    labels, info = rm.replicate_labels(oracle, s, e, ids, lengths, [20] * 16)
    offered = info["n_offered"]
    assert offered[0] == int((ids != mr.NO_CONTIG).sum()) and offered == sorted(offered, reverse=True)
    dry = offered.index(0)
    assert 1 < dry < 16 and not any(offered[dry:]) and not any(info["n_kept"][dry:])
    assert sum(info["n_kept"]) == offered[0]                       # every placed read ends up in a replicate
    assert int(labels.max()) == dry
    sp, sb, n_full = rm.shortfall(labels, s, e, ids, lengths, [20] * 16)
    assert n_full >= 1 and sp[0] == 0 and all(p > 0 for p in sp[dry:])    # an empty replicate is short wherever cov > 0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("replicates_plan") / "replicates_plan_driver"
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "replicates_plan_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def ask(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = [dict(kv.split("=", 1) for kv in row.split()) for row in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def test_plan_accepts_any_order_and_names_the_replicate_that_breaks_the_rule(driver):
    top = (1 << 31) - 1
    cases = [
        # coverages, flags, n_reads, rc, bad
        ([100], 0, 7, QMCP_OK, 0), ([5, 5, 5, 5], 0, 0, QMCP_OK, 0), ([30, 10, 30], 3, 8, QMCP_OK, 0),
        ([2, 40], 2, 9, QMCP_OK, 0), ([1] * 16, 1, 2, QMCP_OK, 0), ([top, 1, top], 0, 1, QMCP_OK, 0),
        ([], 0, 4, QMCP_EINVAL, 0),                              # no replicate
        ([3] * 17, 0, 4, QMCP_EINVAL, 0),                        # 17 replicates
        ([0], 0, 4, QMCP_EINVAL, 0), ([3, 0, 2], 0, 4, QMCP_EINVAL, 1), ([3, 3, 0], 3, 4, QMCP_EINVAL, 2),
        ([1 << 31], 0, 4, QMCP_ERANGE, 0), ([7, 0xFFFFFFFF], 0, 4, QMCP_ERANGE, 1),
        ([7, 0, 1 << 31], 0, 4, QMCP_EINVAL, 1),                 # the first bad replicate decides
        ([5, 5], 4, 4, QMCP_EINVAL, 0), ([5, 5], 0x80000001, 4, QMCP_EINVAL, 0),   # unknown flag bits
        ([5, 5], 1, 5, QMCP_EINVAL, 0), ([5, 5], 3, 1, QMCP_EINVAL, 0),            # whole pairs, odd n_reads
    ]
    rows = ask(driver, [f"c {len(c)} {f} {n} " + " ".join(map(str, c)) for c, f, n, _, _ in cases] + ["c -1 0 4"])
    for (cov, f, n, rc, bad), row in zip(cases, rows):
        assert (int(row["rc"]), int(row["bad"])) == (rc, bad), (cov, f, n)
    assert (int(rows[-1]["rc"]), int(rows[-1]["bad"])) == (QMCP_EINVAL, 0)   # a NULL list


def test_plan_next_offsets_keep_emptied_contigs_and_refuse_ranks_that_fit_no_mask(driver):
    rows = ask(driver, [
        "n 3 0 10 10 25 | 0 6 6 16",       # the middle contig is empty and stays, with a zero-length run
        "n 3 0 10 14 25 | 0 6 6 16",       # the middle contig's reads are all taken: it stays, with a zero-length run
        "n 1 0 7 | 0 7",                   # nothing taken
        "n 1 0 7 | 0 0",                   # everything taken
        "n 2 0 0 0 | 0 0 0",               # no read at all
        "n 4 0 3 3 3 64 | 0 2 2 2 24",
        "n 2 0 5 9 | 1 3 5",               # ranks must start at 0
        "n 2 0 5 9 | 0 3 2",               # ... never fall
        "n 2 0 5 9 | 0 3 8",               # ... and leave no contig more reads than it had (5 of 4)
        "n 2 1 5 9 | 0 3 5",               # offsets must start at 0
        "n 2 0 5 3 | 0 3 3",               # ... and never fall
    ])
    assert [r["next"] for r in rows[:6]] == ["0,6,6,16", "0,6,6,16", "0,7", "0,0", "0,0,0", "0,2,2,2,24"]
    assert all(int(r["rc"]) == QMCP_OK for r in rows[:6])
    assert all(int(r["rc"]) == QMCP_EINVAL and r["next"] == "" for r in rows[6:])


def test_plan_matches_the_model_step_on_random_masks(driver):
    rng = np.random.default_rng(12)
    lines, want = [], []
    for _ in range(60):
        n_contigs = int(rng.integers(1, 9))
        counts = rng.integers(0, 200, size=n_contigs)
        counts[rng.random(n_contigs) < 0.3] = 0
        offs = np.concatenate([[0], np.cumsum(counts)])
        taken = rng.random(int(offs[-1])) < rng.random() * 0.2
        if rng.random() < 0.3 and n_contigs > 1:
            taken[offs[1]:offs[2]] = True                                  # a contig that loses every read
        free_ranks = offs - np.concatenate([[0], np.cumsum(taken)])[offs]
        lines.append(f"n {n_contigs} " + " ".join(map(str, offs)) + " | " + " ".join(map(str, free_ranks)))
        want.append(",".join(str(int((~taken[:o]).sum())) for o in offs))
    rows = ask(driver, lines)
    assert [r["next"] for r in rows] == want and all(int(r["rc"]) == QMCP_OK for r in rows)


def test_plan_n_full_counts_the_leading_replicates_without_a_short_position(driver):
    rows = ask(driver, ["f 0 0 3 0", "f 5 0", "f 0 0 0", "f"])
    assert [int(r["full"]) for r in rows] == [2, 0, 3, 0]


def test_entries_flags_and_struct_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_replicates_host", "qmcp_hip_solve_replicates_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
    assert "#define QMCP_REPLICATES_MAX 16" in text and pkg.REPLICATES_MAX == 16
    assert "#define QMCP_REPLICATES_WHOLE_PAIRS 1u" in text and pkg.REPLICATES_WHOLE_PAIRS == 1 == rm.WHOLE_PAIRS
    assert "#define QMCP_REPLICATES_SHORTFALL 2u" in text and pkg.REPLICATES_SHORTFALL == 2 == rm.SHORTFALL
    assert pkg.abi_version() == 5


def test_replicates_stats_layout_matches_the_header(pkg, tmp_path):
    fields = ["n_full", "n_offered", "n_kept", "n_mates", "short_positions", "short_bases", "ms_replicate", "ms_split"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ '
           'printf("%zu", sizeof(qmcp_hip_replicates_stats)); '
           + "".join(f'printf(" %zu", offsetof(qmcp_hip_replicates_stats, {f})); ' for f in fields)
           + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", str(exe)],
                         input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R = pkg.ReplicatesStats
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f in fields]


def test_replicate_mask_is_the_label_bytes_compared(pkg):
    labels = np.array([0, 3, 1, 2, 0, 3] * 23, dtype=np.uint8)     # 138 reads: more than two words
    for r in range(1, 4):
        m = pkg.replicate_mask(labels, r)
        assert m.dtype == np.uint64 and m.size == pkg.mask_words(labels.size)
        assert np.array_equal(pkg.mask_to_indices(m, labels.size), np.flatnonzero(labels == r))
        assert np.array_equal(m, rm.replicate_mask(labels, r))
    assert pkg.replicate_mask(np.zeros(0, np.uint8), 1).size == 0


def test_argument_errors_return_before_a_context_is_looked_at(pkg):
    """every host-side refusal comes back with its own code from a NULL context; a well-formed call then fails on the
    context (QMCP_EINVAL, "null context"), which is the next thing either entry looks at"""
    s = np.array([0, 5, 9, 2], np.uint32)
    e = np.array([3, 8, 9, 6], np.uint32)
    ids = np.array([0, 1, 1, 0], np.uint32)
    lengths = np.array([10, 10], np.uint32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))

    def both(cov, k, flags, n=4, null_cov=False):
        cov = np.ascontiguousarray(cov or [1], dtype=np.uint32)
        labels = np.full(4, 0xFF, np.uint8)
        codes = []
        for entry, extra in ((pkg._hip.qmcp_hip_solve_replicates_host, ()),
                             (pkg._hip.qmcp_hip_solve_replicates_device, (None,))):
            codes.append(entry(None, p(s), p(e), p(ids), n, p(lengths), 2, None if null_cov else p(cov), k, flags,
                               C.c_void_p(labels.ctypes.data), *extra, None, None, None))
        assert (labels == 0xFF).all()
        assert codes[0] == codes[1]
        return codes[0], pkg._hip.qmcp_hip_last_error().decode()

    assert both([1 << 31], 1, 0)[0] == QMCP_ERANGE
    assert both([3, 0xFFFFFFFF], 2, 0)[0] == QMCP_ERANGE
    for args, word in [(([], 0, 0), "n_replicates"), (([3] * 17, 17, 0), "n_replicates"), (([3, 0], 2, 0), "is 0"),
                       (([3, 3], 2, 4), "flag"), (([3, 3], 2, 1, 3), "odd")]:
        code, msg = both(*args)
        assert code == QMCP_EINVAL and word in msg, (args, msg)
    code, msg = both([3, 3], 2, 0, null_cov=True)
    assert code == QMCP_EINVAL and "coverages" in msg
    code, msg = both([3, 3], 2, 3)
    assert code == QMCP_EINVAL and "context" in msg
