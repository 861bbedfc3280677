"""Proportional downsampling, the parts that need no GPU: the model (tests/proportional_model.py) computes its need in
exact integers, keeps the fewest reads on small random instances and agrees with the second restatement of the
canonical rule -- these tests pin the definition --; both ends of the fraction's range are the oracle; as_ratio; header,
library and package agree on the two entries, the limit and the stats struct; downsample_bam(proportion=...) refuses
what it does not go together with."""
import ctypes as C
import fractions
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bam_py
import profile_model as pm
import proportional_model as qm
import template_bams as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["reads_placed", "bases_in", "bases_kept", "demand", "whole_positions", "floor_positions", "capped_positions",
          "max_depth", "max_need", "num", "den", "floor", "plain_route", "ms_need", "ms_tally"]
FRACTIONS = [(1, 7), (1, 4), (1, 3), (1, 2), (2, 3), (9, 10), (1048575, 1048576)]


# ------------------------------------------------------------------------------------------ the model
def test_integer_quota_agrees_with_fractions():
    rng = np.random.default_rng(2001)
    depths = [0, 1, 2, 3, 6, 7, 8, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 3 << 20, (3 << 20) + 1, (1 << 31) - 1]
    depths += rng.integers(0, 1 << 31, 200).tolist()
    ratios = FRACTIONS + [(0, 1), (1, 1), (999983, 1048576), (1, 1048576), (5, 5)]
    ratios += [(int(rng.integers(0, d + 1)), d) for d in rng.integers(1, (1 << 20) + 1, 40).tolist()]
    for num, den in ratios:
        for cov in depths:
            want = math.ceil(fractions.Fraction(cov) * fractions.Fraction(num, den))
            assert qm.quota(cov, num, den) == want, (cov, num, den)
            for floor, M in ((0, qm.NO_LIMIT), (3, qm.NO_LIMIT), (3, 5), (9, 5), (0, 1)):
                assert qm.need_of(cov, num, den, floor, M) == min(cov, M, max(want, floor))


def tiny_instance(rng):
    """at most 11 reads on at most 12 positions"""
    L = int(rng.integers(1, 13))
    n = int(rng.integers(0, 12))
    s = rng.integers(0, L, n)
    e = np.minimum(s + rng.integers(0, L, n), L - 1)
    return s.astype(np.int64), e.astype(np.int64), L


@pytest.mark.parametrize("seed", range(2))
def test_model_keeps_the_fewest_reads_and_both_restatements_agree(seed):
    """2 x 160 tiny instances: the selection meets the need, has the brute-force minimum size, and fast_select on the
    need's runs (default cap 0) gives the same set"""
    rng = np.random.default_rng(2010 + seed)
    for _ in range(160):
        s, e, L = tiny_instance(rng)
        num, den = FRACTIONS[int(rng.integers(0, len(FRACTIONS)))]
        floor, M = int(rng.choice([0, 1, 3])), int(rng.choice([1, 5, qm.NO_LIMIT]))
        ids = np.zeros(s.size, np.uint32)
        cov, need = qm.need_array(s, e, L, num, den, floor, M)
        assert np.all(need <= cov) and np.all(need <= M)
        assert np.all(need * den >= np.minimum(cov, M) * num)                     # at least the fraction, up to the limit
        want = qm.expected_mask(s, e, ids, [L], num, den, floor, M)
        kept = pm.unpack(want, s.size)
        assert np.all(pm.coverage(s[kept], e[kept], L) >= need), (s, e, need)
        assert int(kept.sum()) == pm.brute_minimum(s, e, need), (s, e, need)
        assert np.array_equal(qm.expected_mask(s, e, ids, [L], num, den, floor, M, fast=True), want)
        offs, r0, r1, caps = qm.region_table(s, e, ids, [L], num, den, floor, M)
        assert np.array_equal(pm.expected_mask(s, e, ids, [L], 0, offs, r0, r1, caps), want)
        st = qm.stats(s, e, ids, [L], num, den, floor, M, want)
        assert st["demand"] == int(need.sum()) and st["max_need"] == (int(need.max()) if L else 0)
        assert st["bases_kept"] == int((e - s + 1)[kept].sum()) <= st["bases_in"]


# ------------------------------------------------------------------------------------------ both ends are the oracle
def test_whole_fraction_and_zero_fraction_are_the_oracle(oracle):
    rng = np.random.default_rng(2020)
    for _ in range(40):
        L = int(rng.integers(1, 200))
        n = int(rng.integers(0, 300))
        span = np.minimum(rng.integers(1, 41, n), L)
        s = (rng.random(n) * (L - span + 1)).astype(np.int64)
        e = s + span - 1
        ids = np.zeros(n, np.uint32)
        for M in (1, 5, 1000):
            for den in (1, 7):
                got = qm.expected_mask(s, e, ids, [L], den, den, int(rng.integers(0, 4)), M)
                assert np.array_equal(got, oracle.solve(s, e, [L], M)), (M, den)
            for floor in (1, 3, 2000):
                got = qm.expected_mask(s, e, ids, [L], 0, 7, floor, M)
                assert np.array_equal(got, oracle.solve(s, e, [L], min(floor, M))), (M, floor)
            assert not pm.unpack(qm.expected_mask(s, e, ids, [L], 0, 7, 0, M), n).any()
            got = qm.expected_mask(s, e, ids, [L], 1, 3, M, M)                    # floor >= M: flat at M
            assert np.array_equal(got, oracle.solve(s, e, [L], M))


# ------------------------------------------------------------------------------------------ as_ratio
def test_as_ratio_edges(pkg):
    F = fractions.Fraction
    assert pkg.PROPORTION_DEN_MAX == 1 << 20
    assert pkg.as_ratio((2, 4)) == (2, 4) and pkg.as_ratio([0, 5]) == (0, 5) and pkg.as_ratio((5, 5)) == (5, 5)
    assert pkg.as_ratio(F(2, 4)) == (1, 2) and pkg.as_ratio(F(0)) == (0, 1) and pkg.as_ratio(F(1)) == (1, 1)
    assert pkg.as_ratio(F(1, 3_000_000)) == (1, 3_000_000)                       # as is: the library refuses it
    assert pkg.as_ratio((np.uint32(1), np.int64(3))) == (1, 3)
    assert pkg.as_ratio(0.25) == (1, 4) and pkg.as_ratio(0.0) == (0, 1) and pkg.as_ratio(1.0) == (1, 1)
    assert pkg.as_ratio(0) == (0, 1) and pkg.as_ratio(1) == (1, 1) and pkg.as_ratio(np.float64(0.5)) == (1, 2)
    num, den = pkg.as_ratio(1 / 3)
    assert F(num, den) == F(1 / 3).limit_denominator(1 << 20) == F(1, 3)
    num, den = pkg.as_ratio(1e-9)                                                 # below 1 / 2^20: rounds to nothing
    assert (num, den) == (0, 1)
    num, den = pkg.as_ratio(math.pi / 4)
    assert den <= 1 << 20 and abs(num / den - math.pi / 4) < 2.0 ** -39
    assert all(isinstance(v, int) for v in pkg.as_ratio(np.float32(0.5)))
    for bad in (-0.1, 1.0000001, (3, 2), (-1, 2), (1, 0), (1, -2), F(3, 2), F(-1, 2), 2, -1, float("nan"),
                float("inf"), (1, 2, 3), (1,)):
        with pytest.raises(ValueError):
            pkg.as_ratio(bad)
    with pytest.raises(TypeError):
        pkg.as_ratio((0.5, 1))                                                   # a pair holds integers


# ------------------------------------------------------------------------------------------ header, library, package
def test_entries_limit_and_stats_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_proportional_host", "qmcp_hip_solve_proportional_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
        assert hasattr(pkg._hip, name)
    assert "#define QMCP_PROPORTION_DEN_MAX (1u << 20)" in text
    assert hasattr(pkg.Solver, "solve_proportional") and hasattr(pkg.Solver, "solve_proportional_device")
    assert pkg.abi_version() == 5
    body = re.search(r"typedef struct qmcp_hip_proportional_stats \{(.*?)\} qmcp_hip_proportional_stats;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert declared == FIELDS == [name for name, _ in pkg.ProportionalStats._fields_]


def test_proportional_stats_layout_matches_the_header(pkg, tmp_path):
    args = ", ".join(f"offsetof(qmcp_hip_proportional_stats, {f})" for f in FIELDS)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ '
           f'size_t v[] = {{sizeof(qmcp_hip_proportional_stats), {args}, QMCP_PROPORTION_DEN_MAX}}; '
           'for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]); return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-",
                          "-o", str(exe)], input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = pkg.ProportionalStats
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [pkg.PROPORTION_DEN_MAX]
    assert C.sizeof(S) == 88


def test_request_mirror_ends_with_the_proportion_fields(pkg):
    names = [name for name, _ in pkg.DownsampleRequest._fields_]
    tail = ["proportional_report", "proportion_num", "proportion_den", "proportion_floor", "has_proportion"]
    assert names[-5:] == tail
    text = open(os.path.join(ROOT, "genome-downsampler_amd", "host", "include", "qmcp_host_request.h")).read()
    body = re.search(r"typedef struct qmcp_host_downsample_request \{(.*?)\} qmcp_host_downsample_request;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
    assert declared == names


# ------------------------------------------------------------------------------------------ downsample_bam
def test_downsample_bam_proportion_refuses_what_it_does_not_go_together_with(pkg, tmp_path):
    refs = [("chrA", 4000)]
    path = tmp_path / "in.bam"
    bam_py.write_bam(path, refs, tb.single_end_records(np.random.default_rng(1), refs, 50))
    bed = tmp_path / "t.bed"
    bed.write_text("chrA\t10\t500\n")
    caps = tmp_path / "caps.bedgraph"
    caps.write_text("chrA\t10\t500\t2\n")
    go = lambda **kw: pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", 40, **kw)
    on = dict(per_reference=True, proportion=0.25)
    refused = [
        (dict(proportion=0.25), "per_reference"),
        (dict(on, targets=bed), "targets"), (dict(on, report=tmp_path / "r.tsv"), "depth report"),
        (dict(on, track=tmp_path / "t.bedgraph"), "depth track"),
        (dict(on, ladder=[3], ladder_out=tmp_path / "l{M}.bam"), "ladder"), (dict(on, stratify="strand"), "stratify"),
        (dict(on, dedup=True), "dedup"), (dict(on, profile=caps), "coverage profile"),
        (dict(on, pair_aware=True), "pair_aware"), (dict(on, template_aware=True), "template_aware"),
        (dict(on, ceiling=True), "ceiling"), (dict(on, budget_reads=10), "budget"),
        (dict(on, replicates=2, replicates_out=tmp_path / "r{R}.bam"), "replicates"),
        (dict(on, bed=bed, amplicons_by_reference=True), "amplicon"), (dict(on, tsv=bed), "amplicon"),
        (dict(per_reference=True, proportional_report=tmp_path / "p.tsv"), "need proportion"),
        (dict(per_reference=True, proportion_floor=2), "need proportion"),
        (dict(per_reference=True, proportion=1.5), "0 .. 1"), (dict(per_reference=True, proportion=(1, 0)), "denominator"),
        (dict(per_reference=True, proportion=(1, (1 << 20) + 1)), "denominator"),
        (dict(on, proportion_floor=-1), "proportion_floor"),
    ]
    for kw, word in refused:
        with pytest.raises(ValueError, match=word):
            go(**kw)
    with pytest.raises(ValueError, match="max_coverage"):
        pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", 1 << 31, **on)
    with pytest.raises(ValueError, match="quality"):
        pkg.downsample_bam("quasi-mcp-hip-quality", path, tmp_path / "no.bam", 40, **on)
    assert not (tmp_path / "no.bam").exists() and not (tmp_path / "p.tsv").exists()
