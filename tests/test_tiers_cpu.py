"""Tiered downsampling, the parts that need no GPU: the model (tests/tiers_model.py) against the contract's four
guarantees, the oracle's by-contig selection and brute force on small instances; the host-side plan
(genome-downsampler_amd/csrc/tiers_plan.h) compiled with g++ alone into tests/cpp/tiers_plan_driver.cpp;
tiers_from_mapq and write_tiers_report; the two entries are declared, listed and exported and the two structs' layouts
match the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import multi_reference as mr
import profile_model as pm
import tiers_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QMCP_OK, QMCP_EINVAL, QMCP_ERANGE = 0, -1, -3
INSTANCES = 320


def small_instance(seed):
    """1-4 contigs, spans 1-40, 1-5 tiers, M of 1-6, some NO_TIER and NO_CONTIG reads, now and then a stretch without
    tier 0; at most 14 reads per (tier, contig) on every third seed, for brute force"""
    rng = np.random.default_rng(90_000 + seed)
    n_contigs, n_tiers, M = int(rng.integers(1, 5)), int(rng.integers(1, 6)), int(rng.integers(1, 7))
    lengths = rng.integers(20, 140, size=n_contigs)
    tiny = seed % 3 == 0
    n = int(rng.integers(1, 12 if tiny else 90))
    weights = rng.random(n_tiers) + 0.05
    repeats = []
    if rng.random() < 0.5:
        c = int(rng.integers(0, n_contigs))
        a = int(rng.integers(0, lengths[c]))
        repeats.append((c, a, min(a + int(rng.integers(5, 40)), int(lengths[c]) - 1)))
    s, e, ids, tiers = tm.instance(rng, lengths, n, (1, 40), weights, repeats, no_tier=0.06, no_contig=0.05)
    return s, e, ids, tiers, lengths.astype(np.uint32), M, n_tiers


@pytest.mark.parametrize("block", range(8))
def test_model_keeps_the_four_guarantees(oracle, block):
    brute = 0
    for seed in range(block * INSTANCES // 8, (block + 1) * INSTANCES // 8):
        s, e, ids, tiers, lengths, M, n_tiers = small_instance(seed)
        S, rows, picks = tm.tiered(s, e, ids, tiers, lengths, M, n_tiers)
        S_fast, rows_fast, picks_fast = tm.tiered(s, e, ids, tiers, lengths, M, n_tiers, fast=True)
        assert np.array_equal(S, S_fast) and np.array_equal(rows, rows_fast), seed       # the two forms agree
        assert all(np.array_equal(a, b) for a, b in zip(picks, picks_fast)), seed
        placed = (ids != tm.NO_CONTIG) & (tiers != tm.NO_TIER)
        assert not S[~placed].any()
        # 1: the kept depth reaches min(cov of all tiered reads, M), and after every tier that of the tiers so far
        assert tm.covers(s, e, ids, tiers, lengths, M, n_tiers, S), seed
        so_far = np.zeros(s.size, bool)
        for t in range(n_tiers):
            so_far |= picks[t]
            upto = np.where(tiers <= t, tiers, tm.NO_TIER)
            assert tm.covers(s, e, ids, upto, lengths, M, t + 1, so_far), (seed, t)
        # 2: tier 0 alone is the oracle's by-contig selection of its reads at M
        on0 = np.flatnonzero(placed & (tiers == 0))
        want0 = pm.unpack(mr.oracle_by_contig(oracle, s[on0], e[on0], ids[on0], lengths, M), on0.size)
        assert np.array_equal(picks[0][on0], want0), seed
        on = tm.members(ids, tiers, lengths.size, n_tiers)
        all_on = [np.flatnonzero((ids == c) & placed) for c in range(lengths.size)]
        before = np.zeros(s.size, bool)
        first_seen = [False] * lengths.size
        for t in range(n_tiers):
            need = tm.needs(s, e, on[t], lengths.tolist(), before, M, all_on)
            for c, (nd, cov, cap) in enumerate(need):
                sel = on[t][c]
                kept = sel[picks[t][sel]]
                # 3: a read of tier t is kept only through need_t: none where nothing is asked, and every kept read
                # covers a position that asks
                if nd.sum() == 0:
                    assert kept.size == 0, (seed, t, c)
                for i in kept.tolist():
                    assert nd[s[i]:e[i] + 1].max() > 0, (seed, t, c, i)
                # 4: the first tier with reads on a contig is solved there with zero credit: the by-contig selection
                if sel.size and not first_seen[c]:
                    first_seen[c] = True
                    assert (cap == M).all()
                    alone = pm.unpack(mr.oracle_by_contig(oracle, s[sel], e[sel], np.zeros(sel.size, np.uint32),
                                                          [int(lengths[c])], M), sel.size)
                    assert np.array_equal(picks[t][sel], alone), (seed, t, c)
                # every K_t has the brute-force minimum size for need_t
                if 0 < sel.size <= 14:
                    assert kept.size == pm.brute_minimum(s[sel], e[sel], cap), (seed, t, c)
                    brute += 1
            before |= picks[t]
        # the rows' counts
        for t in range(n_tiers):
            mine = placed & (tiers == t)
            assert rows[t, 0] == mine.sum() and rows[t, 1] == (S & mine).sum()
            assert rows[t, 2] == (e[mine].astype(np.int64) - s[mine] + 1).sum()
        assert (rows[0, 4:] == 0).all()
    assert brute > 40


def test_order_between_tiers_does_not_matter():
    """shuffling reads of DIFFERENT tiers against each other (every tier keeps its own order) changes no tier's
    selection: a tier sees the others only through their kept reads' depth"""
    for seed in range(40):
        s, e, ids, tiers, lengths, M, n_tiers = small_instance(1000 + seed)
        S, rows, _ = tm.tiered(s, e, ids, tiers, lengths, M, n_tiers)
        rng = np.random.default_rng(seed)
        # a random interleaving of the tiers' index lists that keeps each list's order
        lists = [np.flatnonzero(tiers == t).tolist() for t in np.unique(tiers).tolist()]
        lanes = rng.permutation(np.repeat(np.arange(len(lists)), [len(l) for l in lists]))
        heads = [0] * len(lists)
        order = []
        for k in lanes.tolist():
            order.append(lists[k][heads[k]])
            heads[k] += 1
        order = np.array(order, np.int64)
        S2, rows2, _ = tm.tiered(s[order], e[order], ids[order], tiers[order], lengths, M, n_tiers)
        assert np.array_equal(S2, S[order]) and np.array_equal(rows2, rows), seed


def test_repeat_stretches_are_filled_from_later_tiers_only_there():
    """the issue's picture in small: a stretch without tier 0 is filled by tiers 1 and 2; away from it tier 0 alone
    reaches M nearly everywhere, so hardly a later read is kept"""
    rng = np.random.default_rng(5)
    L, M = 3000, 10
    s, e, ids, tiers = tm.instance(rng, [L], 900, (80, 120), [85, 10, 5], repeats=[(0, 1000, 1299)])
    S, rows, picks = tm.tiered(s, e, ids, tiers, [L], M, 3, fast=True)
    assert tm.covers(s, e, ids, tiers, [L], M, 3, S)
    only0 = np.where(tiers == 0, 0, tm.NO_TIER).astype(np.uint32)
    assert not tm.covers(s, e, ids, tiers, [L], M, 3, tm.tiered(s, e, ids, only0, [L], M, 1, fast=True)[0])
    later = np.flatnonzero(S & (tiers > 0))
    outside = later[(e[later] < 1000 - 120) | (s[later] > 1299 + 120)]
    assert later.size > 20 and outside.size < later.size / 4


# ------------------------------------------------------------------------------------------ the plan
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tiers_plan") / "tiers_plan_driver"
    out = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all", "-g", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "tiers_plan_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def run_driver(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = [dict(kv.split("=", 1) for kv in row.split()) for row in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def plan(driver, requests):
    """requests: (counts[n_tiers, n_contigs], lengths, M, max_reads, max_positions) -> (rc, (bad_t, bad_c), batches)"""
    lines = []
    for counts, lengths, M, max_reads, max_positions in requests:
        counts = np.asarray(counts)
        lines.append(f"p {counts.shape[0]} {counts.shape[1]} {M} {max_reads} {max_positions} | " +
                     " ".join(map(str, counts.flatten())) + " | " + " ".join(map(str, lengths)))
    keys = ("tier", "first_contig", "n_contigs", "first_read", "n_reads", "positions")
    return [(int(r["rc"]), tuple(int(x) for x in r["bad"].split(",")),
             [] if r["batches"] == "-" else [dict(zip(keys, map(int, b.split(":")))) for b in r["batches"].split(";")])
            for r in run_driver(driver, lines)]


def test_plan_refuses_what_the_contract_refuses(driver):
    calls = [
        ("c 1 3 1 2 5 100", QMCP_OK, 0),
        ("c 0 3 1 2 5 100", QMCP_EINVAL, 1),                    # no contig lengths
        ("c 1 0 1 2 5 100", QMCP_EINVAL, 1),                    # n_contigs == 0
        ("c 1 3 0 2 5 100", QMCP_EINVAL, 2),                    # no tier column
        ("c 1 3 1 0 5 100", QMCP_EINVAL, 3),                    # n_tiers == 0
        ("c 1 3 1 16 5 100", QMCP_OK, 0),
        ("c 1 3 1 17 5 100", QMCP_ERANGE, 4),                   # more than QMCP_TIERS_MAX
        (f"c 1 {1 << 20} 1 16 5 100", QMCP_OK, 0),              # 2^24 groups exactly
        (f"c 1 {(1 << 20) + 1} 1 16 5 100", QMCP_ERANGE, 5),
        (f"c 1 3 1 2 {(1 << 31) - 1} 100", QMCP_OK, 0),
        (f"c 1 3 1 2 {1 << 31} 100", QMCP_ERANGE, 6),           # M >= 2^31
        (f"c 1 3 1 2 5 {1 << 31}", QMCP_OK, 0),
        (f"c 1 3 1 2 5 {(1 << 31) + 1}", QMCP_ERANGE, 7),
        ("c 1 3 1 0 5 0", QMCP_EINVAL, 3),                      # ... also without reads
    ]
    got = run_driver(driver, [c[0] for c in calls])
    assert [(int(r["rc"]), int(r["why"])) for r in got] == [(rc, why) for _, rc, why in calls]


def test_plan_cuts_every_tier_with_reads_and_never_across_a_tier(driver):
    rng = np.random.default_rng(3)
    requests = []
    for _ in range(80):
        n_tiers, n_contigs = int(rng.integers(1, 7)), int(rng.integers(1, 8))
        counts = rng.integers(0, 40, size=(n_tiers, n_contigs))
        counts[rng.random((n_tiers, n_contigs)) < 0.3] = 0
        counts[rng.random(n_tiers) < 0.2] = 0                     # tiers without reads
        lengths = rng.integers(1, 50, size=n_contigs)
        requests.append((counts, lengths, int(rng.integers(1, 9)), 40, 50))   # one pair always fits
    for (counts, lengths, M, max_reads, max_positions), (rc, _, batches) in zip(requests, plan(driver, requests)):
        assert rc == QMCP_OK
        n_tiers, n_contigs = counts.shape
        first_of = np.concatenate([[0], np.cumsum(counts.flatten())])     # grouped order is tier-major
        seen = np.zeros((n_tiers, n_contigs), dtype=int)
        for b in batches:
            t = b["tier"]
            assert b["n_contigs"] >= 1 and b["first_contig"] + b["n_contigs"] <= n_contigs   # inside one tier
            cs = slice(b["first_contig"], b["first_contig"] + b["n_contigs"])
            seen[t, cs] += 1
            assert b["first_read"] == first_of[t * n_contigs + b["first_contig"]]
            assert b["n_reads"] == counts[t, cs].sum() <= max_reads
            assert b["positions"] == lengths[cs].sum() <= max_positions                      # position batches
        solved = counts.sum(axis=1) != 0
        assert (seen[solved] == 1).all() and (seen[~solved] == 0).all()
        assert [(b["tier"], b["first_contig"]) for b in batches] == sorted((b["tier"], b["first_contig"]) for b in batches)


def test_plan_names_the_pair_that_exceeds_a_limit(driver):
    got = plan(driver, [
        ([[5, 5, 5], [5, 41, 5]], [10, 10, 10], 3, 40, 50),     # tier 1, contig 1: 41 reads against 40
        ([[5, 5], [5, 5]], [10, 51], 2, 40, 50),                # contig 1 has 51 positions against 50
        ([[5, 5], [5, 5]], [30, 30], 0, 40, 50),                # M == 0: nothing is solved
        ([[30, 0, 20, 15, 0, 39]], [10] * 6, 9, 40, 35),        # one tier: the by-contig plan
        ([[1 << 31]], [100], 7, 1 << 30, (1 << 31) - 2),        # the real limits
    ])
    assert got[0][0] == QMCP_ERANGE and got[0][1] == (1, 1) and got[0][2] == []
    assert got[1][0] == QMCP_ERANGE and got[1][1] == (0, 1)
    assert got[2][0] == QMCP_OK and got[2][2] == []
    assert [(b["first_contig"], b["n_contigs"], b["first_read"], b["n_reads"]) for b in got[3][2]] == \
        [(0, 2, 0, 30), (2, 3, 30, 35), (5, 1, 65, 39)]
    assert got[4][0] == QMCP_ERANGE and got[4][1] == (0, 0)


# ------------------------------------------------------------------------------------------ the Python surface
def test_tiers_from_mapq(pkg):
    q = np.array([60, 30, 29, 10, 9, 1, 0, 255])
    assert pkg.tiers_from_mapq(q, [30, 10, 0]).tolist() == [0, 0, 1, 1, 2, 2, 2, 0]
    assert pkg.tiers_from_mapq(q, [30, 10]).tolist() == [0, 0, 1, 1, pkg.NO_TIER, pkg.NO_TIER, pkg.NO_TIER, 0]
    assert pkg.tiers_from_mapq(q, [1]).tolist() == [0, 0, 0, 0, 0, 0, pkg.NO_TIER, 0]
    assert pkg.tiers_from_mapq(q, [0]).dtype == np.uint32 and not pkg.tiers_from_mapq(q, [0]).any()
    assert pkg.tiers_from_mapq([], [30, 0]).size == 0
    for bad in ([], [10, 30], [30, 30, 0], [30, -1], list(range(17, 0, -1))):
        with pytest.raises(ValueError):
            pkg.tiers_from_mapq(q, bad)
    assert pkg.NO_TIER == tm.NO_TIER == 0xFFFFFFFF and pkg.TIERS_MAX == tm.TIERS_MAX == 16


def test_tiers_report_lines(pkg, tmp_path):
    rows = [pkg.TierRow(n_reads=10, n_kept=4, bases_in=1000, bases_kept=400),
            pkg.TierRow(n_reads=3, n_kept=1, bases_in=300, bases_kept=100, demand=7, asked_positions=5)]
    path = tmp_path / "tiers.tsv"
    pkg.write_tiers_report(path, rows, ["mapq>=30", "mapq>=0"], 200, records_written=6, mates_added=1)
    lines = open(path).read().splitlines()
    assert lines[0].startswith("#tier\t") and len(lines) == 5
    assert lines[1].split("\t") == ["0", "mapq>=30", "10", "4", "5.000000", "2.000000", "0", "0"]
    assert lines[2].split("\t") == ["1", "mapq>=0", "3", "1", "1.500000", "0.500000", "7", "5"]
    assert lines[3:] == ["records_written\t6", "mates_added\t1"]


def test_entries_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_tiers_host", "qmcp_hip_solve_tiers_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
    assert "#define QMCP_NO_TIER 0xFFFFFFFFu" in text and "#define QMCP_TIERS_MAX 16" in text
    assert "#define QMCP_HIP_ABI_VERSION 5" in text and pkg.abi_version() == 5
    for name in ("solve_tiers", "solve_tiers_device"):
        assert callable(getattr(pkg.Solver, name))


def test_struct_layouts_match_the_header_and_the_header_is_c99(pkg, tmp_path):
    row = ("n_reads", "n_kept", "bases_in", "bases_kept", "demand", "asked_positions", "capped_positions", "sweeps",
           "ms_stage")
    stats = ("n_tiers", "tiers_used", "reads_untiered", "ms_tiers", "reserved")
    args = ["sizeof(qmcp_hip_tier_row)"] + [f"offsetof(qmcp_hip_tier_row, {f})" for f in row] + \
           ["sizeof(qmcp_hip_tiers_stats)"] + [f"offsetof(qmcp_hip_tiers_stats, {f})" for f in stats]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ ' +
           " ".join(f'printf("%zu\\n", {a});' for a in args) + " return 0; }\n")
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c",
                          "-", "-o", str(exe)], input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R, S = pkg.TierRow, pkg.TiersStats
    want = [C.sizeof(R)] + [getattr(R, f).offset for f in row] + [C.sizeof(S)] + [getattr(S, f).offset for f in stats]
    assert got == want and got[0] == 64 and got[len(row) + 1] == 24
    assert [n for n, _ in R._fields_] == list(row) and [n for n, _ in S._fields_] == list(stats)


# ------------------------------------------------------------------------------------------ the file flow, without a device
def test_request_mirror_has_the_three_fields_between_amplicon_and_proportional_report(pkg, tmp_path):
    names = [n for n, _ in pkg.DownsampleRequest._fields_]
    k = names.index("amplicon_report")
    assert names[k:k + 5] == ["amplicon_report", "mapq_tiers", "n_mapq_tiers", "tiers_report", "proportional_report"]
    assert pkg._COUNT_FIELDS["mapq_tiers"] == "n_mapq_tiers"
    header = open(os.path.join(ROOT, "genome-downsampler_amd", "host", "include", "qmcp_host_request.h")).read()
    body = header[header.index("typedef struct qmcp_host_downsample_request {"):header.index("} qmcp_host_downsample_request;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"(\w+);", body)
    assert declared == names                                     # the mirror equals the header, field for field
    fields = ("amplicon_report", "mapq_tiers", "n_mapq_tiers", "tiers_report", "proportional_report")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_host_request.h"\nint main(void){ ' +
           " ".join(f'printf("%zu\\n", offsetof(qmcp_host_downsample_request, {f}));' for f in fields) +
           ' printf("%zu\\n", sizeof(qmcp_host_downsample_request)); return 0; }\n')
    exe = tmp_path / "request_layout"
    out = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                          os.path.join(ROOT, "genome-downsampler_amd", "host", "include"), "-x", "c", "-", "-o", str(exe)],
                         input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R = pkg.DownsampleRequest
    assert got == [getattr(R, f).offset for f in fields] + [C.sizeof(R)]
    request = pkg._downsample_request(mapq_tiers=[30, 10, 0], tiers_report="t.tsv")
    assert request.n_mapq_tiers == 3 and [request.mapq_tiers[k] for k in range(3)] == [30, 10, 0]
    assert request.tiers_report == b"t.tsv"


def test_downsample_bam_refusals(pkg, tmp_path):
    """every refusal is raised before the input is opened"""
    src, out = tmp_path / "absent.bam", tmp_path / "out.bam"

    def refused(word, solver="quasi-mcp-hip", **kwargs):
        args = dict(per_reference=True, min_mapq=0, mapq_tiers=[30, 10, 0])
        args.update(kwargs)
        with pytest.raises(ValueError) as ex:
            pkg.downsample_bam(solver, src, out, 5, **args)
        assert word in str(ex.value), str(ex.value)

    refused("tiers_report needs mapq_tiers", mapq_tiers=None, tiers_report=tmp_path / "t.tsv")
    refused("must equal min_mapq", min_mapq=5)
    refused("must equal min_mapq", mapq_tiers=[30, 10])
    refused("fall strictly", mapq_tiers=[10, 30, 0])
    refused("fall strictly", mapq_tiers=[30, 30, 0])
    refused("non-empty", mapq_tiers=[])
    refused("at most 16", mapq_tiers=list(range(16, -1, -1)))
    refused("needs per_reference=True", per_reference=False)
    refused("take amplicon files", bed=tmp_path / "a.bed", amplicons_by_reference=True)
    refused("grades by quality", solver="quasi-mcp-hip-quality")
    others = dict(primer_clip=True, start_cap=2, thresholds=9, mean_depth=3.0, budget_bases=10, proportion=0.5, replicates=2,
                  budget_reads=10, budget_fraction=0.5, ceiling=True, pair_aware=True, template_aware=True,
                  targets=tmp_path / "t.bed", report=tmp_path / "r.tsv", track=tmp_path / "t.bg", ladder=[3],
                  stratify="strand", dedup=True, profile=tmp_path / "p.bg")
    for name, value in others.items():
        refused("tiered downsampling does not go together with", **{name: value})
