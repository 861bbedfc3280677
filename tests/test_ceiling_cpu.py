"""Ceiling downsampling, the parts that need no GPU: the model (tests/ceiling_model.py) respects the ceiling, has the
brute-force maximum size and is deterministic on small random instances -- these tests pin the definition --; the two
restatements of the canonical rule agree under the dual cap array; header, library and package agree on the two entries,
the flag and the stats struct; downsample_bam(ceiling=...) refuses what it does not go together with."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bam_py
import ceiling_model as cm
import profile_model as pm
import template_bams as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["reads_placed", "reads_dropped", "mates_dropped", "over_positions", "over_bases", "short_positions",
          "short_bases", "excess_positions", "max_kept_depth", "regions_in", "regions_used", "ms_ceiling"]


def tiny_instance(rng):
    """at most 11 reads on at most 12 positions, caps 0..5 in runs"""
    L = int(rng.integers(1, 13))
    n = int(rng.integers(0, 12))
    s = rng.integers(0, L, n)
    e = np.minimum(s + rng.integers(0, L, n), L - 1)
    cap = np.zeros(L, np.int64)
    p = 0
    while p < L:
        run = int(rng.integers(1, 6))
        cap[p:p + run] = int(rng.integers(0, 6))
        p += run
    return s.astype(np.int64), e.astype(np.int64), cap


@pytest.mark.parametrize("seed", range(4))
def test_model_respects_the_ceiling_and_keeps_the_most_reads(seed):
    """4 x 320 = 1 280 instances; how many of them end below min(cov, cap) somewhere is printed, not asserted"""
    rng = np.random.default_rng(1700 + seed)
    short = 0
    for _ in range(320):
        s, e, cap = tiny_instance(rng)
        L, n = cap.size, s.size
        ids = np.zeros(n, np.uint32)
        offs, r0, r1, caps = pm.regions_of(cap)
        args = (s, e, ids, [L], 0, offs, r0, r1, caps)
        kept = pm.unpack(cm.expected_mask(*args), n)
        cov, have = pm.coverage(s, e, L), pm.coverage(s[kept], e[kept], L)
        assert np.all(have <= cap), (s, e, cap)                                   # the ceiling
        assert int(kept.sum()) == cm.brute_maximum(s, e, cap), (s, e, cap)        # the most reads
        assert np.array_equal(cm.expected_mask(*args), pm.pack(kept))             # deterministic
        assert np.array_equal(cm.expected_mask(*args, fast=True), pm.pack(kept))  # select == fast_select under the dual
        assert np.all(have[cap == 0] == 0)                                        # a cap of 0 keeps nothing over it
        top = int(cov.max()) if L else 0
        assert pm.unpack(cm.expected_mask(s, e, ids, [L], top), n).all()          # caps at the largest depth: everything
        assert pm.unpack(cm.expected_mask(s, e, ids, [L], top + 1), n).all()
        st = cm.stats(*args)
        assert st["excess_positions"] == 0 and st["reads_dropped"] == n - int(kept.sum()) and st["mates_dropped"] == 0
        assert st["max_kept_depth"] == (int(have.max()) if L else 0)
        assert st["short_positions"] == int((have < np.minimum(cov, cap)).sum())
        short += st["short_positions"] > 0
    print(f"seed {seed}: {short} of 320 instances end below min(cov, cap) somewhere")


def test_select_and_fast_select_agree_under_the_dual_on_several_contigs():
    rng = np.random.default_rng(1711)
    for _ in range(30):
        lengths = rng.integers(20, 300, int(rng.integers(1, 4))).astype(np.uint32)
        n = int(rng.integers(0, 400))
        ids = rng.integers(0, lengths.size, n).astype(np.uint32)
        span = rng.integers(1, 40, n)
        s = (rng.random(n) * np.maximum(lengths[ids].astype(np.int64) - span + 1, 1)).astype(np.int64)
        e = np.minimum(s + span - 1, lengths[ids].astype(np.int64) - 1)
        ids[rng.random(n) < 0.1] = cm.NO_CONTIG
        table = pm.random_regions(rng, lengths, 5, zero_run=8)
        default = int(rng.integers(0, 4))
        slow = cm.expected_mask(s, e, ids, lengths, default, *table)
        assert np.array_equal(slow, cm.expected_mask(s, e, ids, lengths, default, *table, fast=True))
        kept = pm.unpack(slow, n)
        assert not kept[ids == cm.NO_CONTIG].any()
        for c, (cov, cap, _) in enumerate(cm.dual_caps(s, e, ids, lengths, default, *table)):
            sel = kept & (ids == c)
            assert np.all(pm.coverage(s[sel], e[sel], cap.size) <= cap)


def test_whole_pairs_drop_the_mate_and_never_keep_an_unplaced_read():
    # pair 0: both placed, read 1 must go (depth 2 over a cap of 1) and takes read 0 with it; pair 1: read 2 kept, its
    # mate unplaced; pair 2: read 4 kept as well, its mate unplaced: neither unplaced read is ever kept
    s = np.array([50, 0, 20, 0, 0, 0])
    e = np.array([59, 9, 29, 0, 9, 0])
    ids = np.array([0, 0, 0, cm.NO_CONTIG, 0, cm.NO_CONTIG], np.uint32)
    plain = pm.unpack(cm.expected_mask(s, e, ids, [100], 1), 6)
    assert plain.tolist() == [True, False, True, False, True, False]              # the lowest index is dropped first
    whole = pm.unpack(cm.expected_mask(s, e, ids, [100], 1, whole_pairs=True), 6)
    assert whole.tolist() == [False, False, True, False, True, False]
    st = cm.stats(s, e, ids, [100], 1, whole_pairs=True)
    assert (st["reads_placed"], st["reads_dropped"], st["mates_dropped"]) == (4, 2, 1)
    assert (st["over_positions"], st["over_bases"], st["short_positions"], st["max_kept_depth"]) == (10, 10, 0, 1)


# ------------------------------------------------------------------------------------------ header, library, package
def test_entries_flag_and_stats_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_ceiling_host", "qmcp_hip_solve_ceiling_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
        assert hasattr(pkg._hip, name)
    assert "#define QMCP_CEILING_WHOLE_PAIRS 1u" in text and pkg.CEILING_WHOLE_PAIRS == 1
    assert hasattr(pkg.Solver, "solve_ceiling") and hasattr(pkg.Solver, "solve_ceiling_device")
    assert pkg.abi_version() == 5
    body = re.search(r"typedef struct qmcp_hip_ceiling_stats \{(.*?)\} qmcp_hip_ceiling_stats;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert declared == FIELDS == [name for name, _ in pkg.CeilingStats._fields_]
    host_nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HOST_LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T qmcp_host_downsample_bam\b", host_nm)


def test_ceiling_stats_layout_matches_the_header(pkg, tmp_path):
    args = ", ".join(f"offsetof(qmcp_hip_ceiling_stats, {f})" for f in FIELDS)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ '
           f'size_t v[] = {{sizeof(qmcp_hip_ceiling_stats), {args}}}; '
           'for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]); return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", str(exe)],
                         input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = pkg.CeilingStats
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS]
    assert C.sizeof(S) == 80


# ------------------------------------------------------------------------------------------ downsample_bam
def test_downsample_bam_ceiling_refuses_what_it_does_not_go_together_with(pkg, tmp_path):
    refs = [("chrA", 4000)]
    path = tmp_path / "in.bam"
    bam_py.write_bam(path, refs, tb.single_end_records(np.random.default_rng(1), refs, 50))
    bed = tmp_path / "t.bed"
    bed.write_text("chrA\t10\t500\n")
    go = lambda **kw: pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", 4, **kw)
    on = dict(per_reference=True, ceiling=True)
    refused = [
        (dict(ceiling=True), "per_reference"),
        (dict(on, targets=bed), "targets"), (dict(on, report=tmp_path / "r.tsv"), "depth report"),
        (dict(on, track=tmp_path / "t.bedgraph"), "depth track"),
        (dict(on, ladder=[3], ladder_out=tmp_path / "l{M}.bam"), "ladder"), (dict(on, stratify="strand"), "stratify"),
        (dict(on, dedup=True), "dedup"), (dict(on, pair_aware=True), "pair_aware"),
        (dict(on, template_aware=True), "template_aware"), (dict(on, bed=bed, amplicons_by_reference=True), "amplicon"),
        (dict(on, tsv=bed), "amplicon"),
        (dict(per_reference=True, ceiling_report=tmp_path / "c.tsv"), "ceiling_report"),
        (dict(ceiling_report=tmp_path / "c.tsv"), "ceiling_report"),
    ]
    for kw, word in refused:
        with pytest.raises(ValueError, match=word):
            go(**kw)
    with pytest.raises(ValueError, match="quality"):
        pkg.downsample_bam("quasi-mcp-hip-quality", path, tmp_path / "no.bam", 4, **on)
    assert not (tmp_path / "no.bam").exists() and not (tmp_path / "c.tsv").exists()
