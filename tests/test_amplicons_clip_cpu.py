"""Amplicon-aware downsampling without a device: csrc/amplicon_assign.h's host search against the model's brute-force
assignment (through tests/cpp/amplicon_assign_check.cpp), BED / TSV to inserts, the ABI's symbols, the refusals of
downsample_bam's new keywords, and the motivating experiment as a property of the model (tests/amplicon_clip_model.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import amplicon_clip_model as am
import multi_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "amplicon_assign_check.cpp")
INC = [os.path.join(ROOT, "genome-downsampler_amd", "csrc"), os.path.join(ROOT, "include")]
SYMBOLS = ("qmcp_hip_solve_amplicons_host", "qmcp_hip_solve_amplicons_device")


# ------------------------------------------------------------------------------------------ the host search
@pytest.fixture(scope="module")
def assign_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("assign") / "amplicon_assign_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *("-I" + d for d in INC),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", SRC, "-o", exe], check=True)
    return exe


def host_assign(exe, offs, a0, a1, units):
    """units: (contig, smallest start, largest end) -> [(label, several)] from amplicon_assign.h"""
    text = [str(len(offs) - 1), " ".join(str(int(o)) for o in offs)]
    text += [f"{int(a)} {int(b)}" for a, b in zip(a0, a1)]
    text += [str(len(units))] + [f"{c} {s} {e}" for c, s, e in units]
    out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = out.stdout.split("\n")
    assert lines[0] == "table ok"
    return [(int(l.split()[0]), bool(int(l.split()[1]))) for l in lines[1:1 + len(units)]]


def boundary_units(rng, offs, a0, a1, lengths, n_random):
    """for every amplicon: itself, each edge moved one base in and one base out, single bases at its edges; and random
    intervals"""
    units = []
    for c in range(len(lengths)):
        L = int(lengths[c])
        for k in range(int(offs[c]), int(offs[c + 1])):
            lo, hi = int(a0[k]), int(a1[k])
            for s, e in ((lo, hi), (lo + 1, hi), (lo, hi - 1), (lo - 1, hi), (lo, hi + 1), (lo, lo), (hi, hi),
                         (lo - 1, lo - 1), (hi + 1, hi + 1)):
                if 0 <= s <= e < L:
                    units.append((c, s, e))
        for _ in range(n_random):
            s = int(rng.integers(0, L))
            units.append((c, s, int(min(L - 1, s + rng.integers(0, 300)))))
    return units


def tables(kind, rng):
    lengths = [4000, 50, 2500]                       # (the second contig has no amplicons)
    per = []
    for L in (4000, 0, 2500):
        if L == 0:
            per.append([])
        elif kind == "tiled":
            per.append([(s, s + 399) for s in range(0, L - 400, 300)])
        elif kind == "overlapping":
            st = rng.integers(0, L - 500, size=30)
            per.append([(int(s), int(s + rng.integers(50, 500))) for s in st])
        elif kind == "duplicated":
            base = [(int(s), int(s) + 299) for s in rng.integers(0, L - 300, size=8)]
            per.append([base[i] for i in rng.integers(0, 8, size=30)])
        else:                                        # nested: every amplicon inside the one before
            per.append([(10 * i, L - 1 - 7 * i) for i in range(40)] + [(0, L - 1)])
    for v in per:
        order = rng.permutation(len(v))              # the caller's table is in no particular order
        v[:] = [v[i] for i in order]
    offs = np.concatenate([[0], np.cumsum([len(v) for v in per])]).astype(np.uint32)
    flat = [a for v in per for a in v]
    return lengths, offs, np.array([a[0] for a in flat], np.uint32), np.array([a[1] for a in flat], np.uint32)


@pytest.mark.parametrize("kind", ["tiled", "overlapping", "duplicated", "nested"])
def test_host_search_equals_the_brute_force_rule(assign_check, kind):
    rng = np.random.default_rng(len(kind))
    lengths, offs, a0, a1 = tables(kind, rng)
    units = boundary_units(rng, offs, a0, a1, lengths, 300)
    got = host_assign(assign_check, offs, a0, a1, units)
    want = [am.assign_unit(offs, a0, a1, [c], [s], [e]) for c, s, e in units]
    assert got == want
    assert sum(l != am.NO_AMPLICON for l, _ in want) > 100 and sum(l == am.NO_AMPLICON for l, _ in want) > 10
    if kind != "tiled":
        assert sum(sev for _, sev in want) > 100


def test_model_assignment_by_hand():
    offs, a0, a1 = [0, 4], [100, 100, 50, 120], [300, 300, 400, 250]
    assert am.assign_unit(offs, a0, a1, [0, 0], [130, 150], [200, 250]) == (3, True)      # the greatest start
    assert am.assign_unit(offs, a0, a1, [0, 0], [130, 150], [200, 251]) == (0, True)      # then the smallest index
    assert am.assign_unit(offs, a0, a1, [0, 0], [60, 150], [200, 301]) == (2, False)
    assert am.assign_unit(offs, a0, a1, [0, 0], [49, 150], [200, 300]) == (am.NO_AMPLICON, False)
    assert am.assign_unit(offs, a0, a1, [0, mr.NO_CONTIG], [130, 150], [200, 250]) == (am.NO_AMPLICON, False)
    assert am.assign_unit([0, 4, 4], a0, a1, [0, 1], [130, 150], [200, 250]) == (am.NO_AMPLICON, False)


# ------------------------------------------------------------------------------------------ BED / TSV -> inserts
def test_inserts_from_bed_and_tsv(pkg, tmp_path):
    bed, tsv = tmp_path / "p.bed", tmp_path / "p.tsv"
    bed.write_text("chrA\t100\t125\tA1_LEFT\nchrA\t475\t500\tA1_RIGHT\n"
                   "chrA\t900\t930\tA2_RIGHT\nchrA\t400\t422\tA2_LEFT\n"
                   "chrB\t0\t20\tB1_LEFT\nchrB\t20\t45\tB1_RIGHT\n")
    tsv.write_text("A1_LEFT\tA1_RIGHT\nA2_RIGHT\tA2_LEFT\n")          # (the second pair names its primers right first)
    names = ["chrA", "chrB"]
    offs, a0, a1 = pkg.amplicons_by_reference(bed, tsv, names)
    i0, i1, left = pkg.amplicon_inserts_by_reference(bed, tsv, names)
    assert offs.tolist() == [0, 2, 2] and a0.tolist() == [100, 400] and a1.tolist() == [500, 930]   # the inclusive quirk
    # the BED end is exclusive: primer [100, 125) ends at base 124, the insert starts at 125 and ends before base 475
    assert i0.tolist() == [125, 422] and i1.tolist() == [474, 899] and left == ["A1_LEFT", "A2_LEFT"]
    # a pair whose primers touch leaves no insert: refused where the inserts are asked for, naming the pair ...
    tsv.write_text("A1_LEFT\tA1_RIGHT\nB1_LEFT\tB1_RIGHT\n")
    with pytest.raises(ValueError, match="B1_LEFT / B1_RIGHT leaves no insert"):
        pkg.amplicon_inserts_by_reference(bed, tsv, names)
    # ... while the amplicons themselves, and so the FILTER, are what they were
    offs, a0, a1 = pkg.amplicons_by_reference(bed, tsv, names)
    assert offs.tolist() == [0, 1, 2] and a0.tolist() == [100, 0] and a1.tolist() == [500, 45]
    # without a TSV: name order within each chrom
    bed.write_text("chrA\t100\t125\tp1\nchrA\t475\t500\tp2\n")
    i0, i1, left = pkg.amplicon_inserts_by_reference(bed, None, names)
    assert i0.tolist() == [125] and i1.tolist() == [474] and left == ["p1"]


# ------------------------------------------------------------------------------------------ ABI
def test_symbols_are_declared_exported_and_listed(pkg):
    header = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", code) and name in pkg.ABI_SYMBOLS and f" T {name}\n" in nm
    assert pkg.abi_version() == 5
    for flag, value in (("SINGLE_END", 1), ("PER_AMPLICON", 2), ("COMPLETE_PAIRS", 4)):
        assert re.search(rf"#define QMCP_AMPLICONS_{flag} {value}u", code) and getattr(pkg, "AMPLICONS_" + flag) == value
    assert "#define QMCP_NO_AMPLICON 0xFFFFFFFFu" in code and pkg.NO_AMPLICON == am.NO_AMPLICON == 0xFFFFFFFF
    assert pkg.AMPLICON_LDS_MAX == int(re.search(r"kAcLdsMax = (\d+);", open(os.path.join(
        ROOT, "genome-downsampler_amd", "csrc", "kernels", "amplicon_clip.inc.hip")).read()).group(1))
    import ctypes as C
    assert C.sizeof(pkg.AmpliconsStats) == 88


# ------------------------------------------------------------------------------------------ downsample_bam
def test_downsample_bam_refuses_what_the_amplicon_keywords_do_not_go_together_with(pkg, tmp_path):
    import bam_py
    import template_bams as tb
    refs = [("chrA", 4000)]
    path = tmp_path / "in.bam"
    bam_py.write_bam(path, refs, tb.single_end_records(np.random.default_rng(1), refs, 50))
    bed = tmp_path / "t.bed"
    bed.write_text("chrA\t10\t35\tL\nchrA\t475\t500\tR\n")
    graph = tmp_path / "p.bedgraph"
    graph.write_text("chrA\t10\t500\t3\n")
    go = lambda **kw: pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", 4, **kw)
    base = dict(per_reference=True, bed=bed, amplicons_by_reference=True)
    need = "primer_clip, per_amplicon and amplicon_report need bed, per_reference=True and amplicons_by_reference=True"
    together = "amplicon-aware downsampling does not go together with "
    for new in (dict(primer_clip=True), dict(per_amplicon=True), dict(amplicon_report=tmp_path / "a.tsv")):
        on = dict(base, **new)
        refused = [
            (new, need), (dict(new, per_reference=True), need), (dict(new, per_reference=True, bed=bed), need),
            (dict(new, bed=bed, amplicons_by_reference=True), need),
            (dict(on, start_cap=2), together + "a start cap"), (dict(on, thresholds=9), together + "coverage thresholds"),
            (dict(on, mean_depth=2.0), together + "a mean depth"), (dict(on, proportion=0.5), together + "a proportion"),
            (dict(on, replicates=2, replicates_out=tmp_path / "r{R}.bam"), together + "replicates"),
            (dict(on, budget_reads=5), together + "a budget"), (dict(on, ceiling=True), together + "ceiling"),
            (dict(on, pair_aware=True), together + "pair_aware"), (dict(on, template_aware=True), together + "template_aware"),
            (dict(on, targets=bed), together + "targets"), (dict(on, report=tmp_path / "r.tsv"), together + "a depth report"),
            (dict(on, track=tmp_path / "t.bedgraph"), together + "a depth track"),
            (dict(on, ladder=[3], ladder_out=tmp_path / "l{M}.bam"), together + "a coverage ladder"),
            (dict(on, stratify="strand"), together + "stratify"), (dict(on, dedup=True), together + "dedup"),
            (dict(on, profile=graph), together + "a coverage profile"),
        ]
        for kw, message in refused:
            with pytest.raises(ValueError, match=re.escape(message)):
                go(**kw)
        with pytest.raises(ValueError, match="amplicon-aware downsampling does not take a solver that grades by quality"):
            pkg.downsample_bam("quasi-mcp-hip-quality", path, tmp_path / "no.bam", 4, **on)
    assert not (tmp_path / "no.bam").exists() and not (tmp_path / "a.tsv").exists()


# ------------------------------------------------------------------------------------------ the motivating experiment
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_contig_wide_selection_is_short_of_trimmed_depth_and_both_modes_are_not(oracle, seed):
    """one 3 000-base contig, 9 amplicons of 400 bases every 300, 25-base primers, log-normal yields, reads of 60 - 200
    bases with 40 % flush with an amplicon edge, M = 50: what FILTER + solve selects today leaves positions short of
    min(primer-trimmed coverage, M); the clipped solves leave none, pooled or per amplicon"""
    M = 50
    s, e, ids, lengths, offs, a0, a1, i0, i1 = am.fragmented_panel(seed)
    assert lengths[0] == 3000 and a0.size == 9
    today = am.unpack(mr.oracle_by_contig(oracle, s, e, ids, lengths, M), s.size)
    short, worst = am.trimmed_shortfall(s, e, ids, lengths, offs, a0, a1, i0, i1, M, today, single_end=True)
    assert short > 100 and worst >= 10
    pooled, _, _, st = am.solve(oracle, s, e, ids, lengths, M, offs, a0, a1, i0, i1, single_end=True)
    per, _, rows, _ = am.solve(oracle, s, e, ids, lengths, M, offs, a0, a1, i0, i1, single_end=True, per_amplicon=True)
    assert st["units_assigned"] == s.size and st["reads_clipped_away"] == 0 and st["reads_shortened"] > s.size // 4
    for keep in (pooled, per):
        assert am.trimmed_shortfall(s, e, ids, lengths, offs, a0, a1, i0, i1, M, keep, single_end=True) == (0, 0)
    assert all(r[12] == 0 for r in rows)                 # every amplicon on its own insert
    # the price, in kept reads: the per-amplicon set also meets the pooled demand (sum_k min(cov_k, M) >= min(sum_k cov_k,
    # M)), so the pooled minimum cannot be larger -- and where two deep inserts overlap it asks for 2 M, not M
    assert pooled.sum() < per.sum()
