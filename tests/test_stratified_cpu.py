"""Stratified downsampling, the parts that need no GPU: the host-side plan (genome-downsampler_amd/csrc/
stratified_plan.h) compiled with g++ alone into tests/cpp/stratified_plan_driver.cpp; the two entries are declared,
listed and exported and the row's layout matches the header; the model on the oracle (tests/stratified_model.py) keeps
every stratum valid at its cap; read_bam(stratify=...) against an independent reading of a BAM written by
tests/bam_py.py; the combinations that are refused."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bam_py
import multi_reference as mr
import stratified_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QMCP_OK, QMCP_EINVAL, QMCP_ERANGE = 0, -1, -3


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stratified_plan") / "stratified_plan_driver"
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "stratified_plan_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def ask(driver, requests):
    """requests: (counts[n_strata, n_contigs], lengths, caps, max_reads, max_positions) -> (rc, (bad_s, bad_c), batches)"""
    lines = []
    for counts, lengths, caps, max_reads, max_positions in requests:
        counts = np.asarray(counts)
        lines.append(f"p {counts.shape[0]} {counts.shape[1]} {max_reads} {max_positions} | " +
                     " ".join(map(str, counts.flatten())) + " | " + " ".join(map(str, lengths)) + " | " +
                     " ".join(map(str, caps)))
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = [dict(kv.split("=", 1) for kv in row.split()) for row in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    keys = ("stratum", "first_contig", "n_contigs", "first_read", "n_reads", "positions", "M")
    return [(int(r["rc"]), tuple(int(x) for x in r["bad"].split(",")),
             [] if r["batches"] == "-" else [dict(zip(keys, map(int, b.split(":")))) for b in r["batches"].split(";")])
            for r in rows]


def test_plan_covers_every_solved_pair_once_and_never_crosses_a_stratum(driver):
    rng = np.random.default_rng(3)
    requests = []
    for _ in range(80):
        n_strata, n_contigs = int(rng.integers(1, 7)), int(rng.integers(1, 8))
        counts = rng.integers(0, 40, size=(n_strata, n_contigs))
        counts[rng.random((n_strata, n_contigs)) < 0.3] = 0
        counts[rng.random(n_strata) < 0.2] = 0                    # strata without reads
        lengths = rng.integers(1, 50, size=n_contigs)
        caps = rng.choice([0, 1, 3, 12], size=n_strata)
        requests.append((counts, lengths, caps, 40, 50))          # one pair always fits: counts < 40, lengths < 50
    for (counts, lengths, caps, max_reads, max_positions), (rc, _, batches) in zip(requests, ask(driver, requests)):
        assert rc == QMCP_OK
        n_strata, n_contigs = counts.shape
        first_of = np.concatenate([[0], np.cumsum(counts.flatten())])   # grouped order is stratum-major
        seen = np.zeros((n_strata, n_contigs), dtype=int)
        for b in batches:
            s = b["stratum"]
            assert b["n_contigs"] >= 1 and b["first_contig"] + b["n_contigs"] <= n_contigs   # inside one stratum
            assert b["M"] == caps[s] != 0
            cs = slice(b["first_contig"], b["first_contig"] + b["n_contigs"])
            seen[s, cs] += 1
            assert b["first_read"] == first_of[s * n_contigs + b["first_contig"]]
            assert b["n_reads"] == counts[s, cs].sum() <= max_reads
            assert b["positions"] == lengths[cs].sum() <= max_positions
        solved = (caps != 0) & (counts.sum(axis=1) != 0)
        assert (seen[solved] == 1).all() and (seen[~solved] == 0).all()   # cap 0 and empty strata produce nothing
        assert [(b["stratum"], b["first_contig"]) for b in batches] == sorted((b["stratum"], b["first_contig"]) for b in batches)


def test_plan_names_the_pair_that_exceeds_a_limit_and_ignores_unsolved_strata(driver):
    counts = [[5, 5, 5], [5, 41, 5], [5, 5, 5]]
    got = ask(driver, [
        (counts, [10, 10, 10], [3, 3, 3], 40, 50),          # stratum 1, contig 1: 41 reads against 40
        (counts, [10, 10, 10], [3, 0, 3], 40, 50),          # ... in a stratum without a cap: not solved, no error
        ([[5, 5], [5, 5]], [10, 51], [0, 2], 40, 50),       # contig 1 has 51 positions against 50; stratum 1 is solved
        ([[0, 0], [0, 0]], [10, 51], [4, 2], 40, 50),       # ... but no stratum has reads: nothing to solve
        ([[1 << 31]], [100], [7], 1 << 30, (1 << 31) - 2),  # the real limits
    ])
    assert got[0][0] == QMCP_ERANGE and got[0][1] == (1, 1) and got[0][2] == []
    assert got[1][0] == QMCP_OK and {b["stratum"] for b in got[1][2]} == {0, 2}
    assert got[2][0] == QMCP_ERANGE and got[2][1] == (1, 1)
    assert got[3][0] == QMCP_OK and got[3][2] == []
    assert got[4][0] == QMCP_ERANGE and got[4][1] == (0, 0)


def test_plan_one_stratum_is_the_by_contig_plan(driver):
    (rc, _, batches), = ask(driver, [([[30, 0, 20, 15, 0, 39]], [10, 10, 10, 10, 10, 10], [9], 40, 35)])
    assert rc == QMCP_OK
    assert [(b["first_contig"], b["n_contigs"], b["first_read"], b["n_reads"]) for b in batches] == \
        [(0, 2, 0, 30), (2, 3, 30, 35), (5, 1, 65, 39)]   # greedy: contig 2 would make 50 reads, contig 5 74
    assert all(b["stratum"] == 0 and b["M"] == 9 for b in batches)


def test_entries_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_stratified_host", "qmcp_hip_solve_stratified_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
    assert "#define QMCP_NO_STRATUM 0xFFFFFFFFu" in text and pkg.NO_STRATUM == 0xFFFFFFFF == sm.NO_STRATUM
    assert "#define QMCP_HIP_ABI_VERSION 5" in text and pkg.abi_version() == 5
    kernels_h = open(os.path.join(ROOT, "genome-downsampler_amd", "csrc", "qmcp_kernels.h")).read()
    assert f"kStratumTallyTile = {pkg.STRATUM_TALLY_TILE};" in kernels_h and pkg.STRATUM_TALLY_TILE % 256 == 0


def test_stratum_row_layout_matches_the_header_and_the_header_is_c99(pkg, tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ '
           'printf("%zu %zu %zu %zu %zu\\n", sizeof(qmcp_hip_stratum_row), offsetof(qmcp_hip_stratum_row, n_reads), '
           'offsetof(qmcp_hip_stratum_row, n_kept), offsetof(qmcp_hip_stratum_row, bases_in), '
           'offsetof(qmcp_hip_stratum_row, bases_kept)); return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c",
                          "-", "-o", str(exe)], input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R = pkg.StratumRow
    assert got == [32, 0, 8, 16, 24] == [C.sizeof(R), R.n_reads.offset, R.n_kept.offset, R.bases_in.offset,
                                         R.bases_kept.offset]


@pytest.mark.parametrize("seed", range(30))
def test_model_keeps_every_stratum_valid_at_its_cap(oracle, seed):
    rng = np.random.default_rng(4000 + seed)
    s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(1, 5)), max_reads_per_contig=1200)
    n_strata = int(rng.choice([1, 2, 3, 7]))
    strata = sm.random_strata(rng, s.size, n_strata)
    caps = rng.choice([0, 1, 3, 12, 50, 200], size=n_strata)
    keep = sm.stratified_bits(oracle, s, e, ids, strata, lengths, caps)
    assert not keep[(ids == mr.NO_CONTIG) | (strata == sm.NO_STRATUM)].any()
    rows = sm.rows(s, e, ids, strata, n_strata, keep)
    assert rows[:, 1].sum() == keep.sum() and (rows[:, 1] <= rows[:, 0]).all() and (rows[:, 3] <= rows[:, 2]).all()
    for k in range(n_strata):
        if caps[k] == 0:
            assert not keep[strata == k].any()
        for c in range(lengths.size):
            on = np.flatnonzero((ids == c) & (strata == k))
            L = int(lengths[c])
            cov = oracle.cover(s[on], e[on], L)
            out = oracle.cover(s[on[keep[on]]], e[on[keep[on]]], L)
            assert oracle.is_out_cover_valid(cov, out, int(caps[k])), f"stratum {k} (cap {caps[k]}), contig {c}"
    if n_strata == 1 and not (strata == sm.NO_STRATUM).any():
        assert np.array_equal(sm.pack(keep), mr.oracle_by_contig(oracle, s, e, ids, lengths, int(caps[0])))


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("stratified_bam") / "groups.bam"
    header, parsed, ref_lengths = sm.write_stratified_bam(path, np.random.default_rng(23))
    return path, header, parsed, ref_lengths


@pytest.mark.parametrize("stratify", ["read_group", "strand"])
def test_read_bam_strata_equal_an_independent_reading(pkg, bam, stratify):
    path, header, parsed, ref_lengths = bam
    groups = [r["rg"] for r in parsed]
    assert groups.count(None) > 10 and groups.count("rgX") == 1 and set(sm.READ_GROUPS) <= set(groups)
    assert {r["reverse"] for r in parsed} == {True, False}
    reads, ids, filtered = mr.expected_per_reference_reads(parsed)
    want, names = sm.expected_strata(parsed, reads, stratify)
    got = pkg.read_bam(path, per_reference=True, stratify=stratify)
    assert got["stratum_names"] == names
    assert got["strata"].dtype == np.uint32 and np.array_equal(got["strata"], want)
    assert set(np.unique(want)) == set(range(len(names)))              # every stratum occurs, "*" included
    plain = pkg.read_bam(path, per_reference=True)                      # nothing else changes
    for key in ("bam_ids", "starts", "ends", "contig_ids", "contig_lengths", "filtered_out", "is_first"):
        assert np.array_equal(got[key], plain[key]), key
    assert np.array_equal(got["contig_ids"], ids) and list(got["contig_lengths"]) == ref_lengths
    assert "strata" not in plain and "stratum_names" not in plain


def test_refused_combinations(pkg, bam, tmp_path):
    path = bam[0]
    out = tmp_path / "out.bam"
    with pytest.raises(ValueError, match="per_reference"):
        pkg.read_bam(path, stratify="strand")
    with pytest.raises(ValueError, match="strand.*read_group"):
        pkg.read_bam(path, per_reference=True, stratify="sample")
    base = dict(per_reference=True, stratify="read_group")
    for kwargs, word in [(dict(per_reference=False), "per_reference"), (dict(stratify="sample"), "read_group"),
                         (dict(targets=tmp_path / "t.bed"), "targets"), (dict(report=tmp_path / "r.tsv"), "report"),
                         (dict(ladder=[5, 2], ladder_out=tmp_path / "o.{M}.bam"), "ladder")]:
        args = dict(base)
        args.update(kwargs)
        with pytest.raises(ValueError, match=word):
            pkg.downsample_bam("quasi-mcp-hip", path, out, 20, **args)
    with pytest.raises(ValueError, match="quality"):
        pkg.downsample_bam("quasi-mcp-hip-quality", path, out, 20, **base)
    with pytest.raises(ValueError, match="stratify"):
        pkg.downsample_bam("quasi-mcp-hip", path, out, 20, per_reference=True, strata_report=tmp_path / "s.tsv")
    # BamApiConfig's own rules (std::invalid_argument, brought back as -4 and its message), without the Python checks
    for per_ref, targets, report, ladder, word in [(0, None, None, None, "needs per_reference"),
                                                   (1, "t.bed", None, None, "does not take targets"),
                                                   (1, None, "r.tsv", None, "does not take a depth report"),
                                                   (1, None, None, [5, 2], "does not take a coverage ladder")]:
        err = C.create_string_buffer(1024)
        request = pkg._downsample_request(solver_name="quasi-mcp-hip", in_path=path, out_path=out, max_coverage=20,
                                          per_reference=per_ref, stratify="strand", targets=targets, report=report,
                                          ladder_levels=ladder)
        rc = pkg._host.qmcp_host_downsample_bam(C.byref(request), None, 0, None, None, None, None, None, err, 1024)
        assert rc == -4 and word in err.value.decode(), err.value
    assert not out.exists()
    assert pkg.solver_names() == ["quasi-mcp-hip"]      # the registry lists what it listed before
