"""The start cap, the parts that need no GPU: the literal model (tests/start_cap_model.py) against brute force on tiny
inputs and on the deep one-length shape the feature exists for; the entries declared, listed and exported with the ABI
version unchanged and the stats structure laid out as the C99 header says; the request's new fields; the combinations
downsample_bam and the C++ host layer refuse."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import multi_reference as mr
import start_cap_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["reads_placed", "cells", "cells_over_cap", "reads_capped", "largest_cell", "reads_survived", "cells_kept",
          "largest_kept_cell", "short_positions", "short_bases", "key_bits", "sort_passes", "cap", "ms_cap"]


def tiny(rng):
    n_contigs = int(rng.integers(1, 3))
    lengths = rng.integers(12, 30, size=n_contigs).astype(np.uint32)
    n = int(rng.integers(0, 21))
    ids = rng.integers(0, n_contigs, size=n)
    s = rng.integers(0, 3, size=n)                               # (few starts: cells of several reads)
    e = s + rng.integers(0, 8, size=n)
    ids = np.where(rng.random(n) < 0.1, mr.NO_CONTIG, ids)
    g = rng.integers(0, 2, size=n).astype(np.uint32)
    q = rng.integers(0, 3, size=n).astype(np.uint32)
    return s.astype(np.uint32), e.astype(np.uint32), ids.astype(np.uint32), lengths, g, q


def better(i, j, s, e, q):
    """read i comes before read j in a cell's order: priority descending, span descending, index ascending"""
    return (-int(q[i]), -(int(e[i]) - int(s[i])), i) < (-int(q[j]), -(int(e[j]) - int(s[j])), j)


def test_model_survivors_are_the_best_k_of_every_cell_by_brute_force(oracle):
    rng = np.random.default_rng(1)
    capped_some = 0
    for _ in range(300):
        s, e, ids, lengths, g, q = tiny(rng)
        n = s.size
        K = int(rng.integers(1, 4))
        use_g, use_q = rng.random() < 0.7, rng.random() < 0.7
        keep, capped, st, hist = sm.start_cap(oracle, s, e, ids, lengths, 2, K, groups=g if use_g else None,
                                              priorities=q if use_q else None, shortfall=True, hist_bins=4)
        gg = g if use_g else np.zeros(n, np.uint32)
        qq = q if use_q else np.zeros(n, np.uint32)
        placed = ids != mr.NO_CONTIG
        survive = placed & ~capped
        cell_of = lambda i: (int(ids[i]), int(s[i]), int(gg[i]))
        cells = {}
        for i in np.flatnonzero(placed):
            cells.setdefault(cell_of(i), []).append(int(i))
        for members in cells.values():
            # a read survives iff fewer than K members of its cell come before it
            for i in members:
                ahead = sum(better(j, i, s, e, qq) for j in members if j != i)
                assert survive[i] == (ahead < K)
            # every subset check: no set of more than K members survives whole, and the survivors beat the rest
            for r in range(K + 1, min(len(members), K + 2) + 1):
                assert not any(all(survive[i] for i in sub) for sub in itertools.combinations(members, r))
            assert all(better(i, j, s, e, qq) for i in members for j in members if survive[i] and not survive[j])
            assert sum(keep[i] for i in members) <= K
        assert not capped[~placed].any() and not keep[~survive].any()
        on = np.flatnonzero(survive)
        want = sm.unpack(mr.oracle_by_contig(oracle, s[on], e[on], ids[on], lengths, 2), on.size)
        assert np.array_equal(keep[on], want)
        sizes = np.array([len(m) for m in cells.values()], np.int64)
        assert st["cells"] == len(cells) and st["reads_placed"] == placed.sum() and st["reads_survived"] == survive.sum()
        assert st["cells_over_cap"] == (sizes > K).sum() and st["reads_capped"] == np.maximum(sizes - K, 0).sum()
        assert st["largest_cell"] == (sizes.max() if sizes.size else 0)
        kept_cells = [sum(keep[i] for i in m) for m in cells.values()]
        assert st["cells_kept"] == sum(k > 0 for k in kept_cells) and st["largest_kept_cell"] == max(kept_cells, default=0)
        assert hist.sum() == len(cells) and all(hist[k] == (np.minimum(sizes, 4) == k + 1).sum() for k in range(4))
        # the shortfall, position by position
        short_p = short_b = 0
        for c, L in enumerate(lengths):
            for p in range(int(L)):
                cov = sum(1 for i in np.flatnonzero(placed) if ids[i] == c and s[i] <= p <= e[i])
                got = sum(1 for i in np.flatnonzero(keep) if ids[i] == c and s[i] <= p <= e[i])
                lack = max(min(cov, 2) - got, 0)
                short_p += lack > 0
                short_b += lack
        assert (st["short_positions"], st["short_bases"]) == (short_p, short_b)
        capped_some += bool(capped.any())
    assert capped_some > 100


def test_model_with_no_cell_over_the_cap_is_the_plain_selection(oracle):
    rng = np.random.default_rng(2)
    for _ in range(100):
        s, e, ids, lengths, g, q = tiny(rng)
        K = max(int(sm.cells_and_ranks(s, e, ids, g, q)[3].max(initial=1)), 1)
        for M in (1, 3):
            keep, capped, st, _ = sm.start_cap(oracle, s, e, ids, lengths, M, K, groups=g, priorities=q, shortfall=True)
            assert np.array_equal(keep, sm.unpack(mr.oracle_by_contig(oracle, s, e, ids, lengths, M), s.size))
            assert not capped.any() and st["short_positions"] == st["short_bases"] == 0


def test_deep_one_length_data_piles_up_and_a_cap_of_one_spreads_it_at_no_cost(oracle):
    """12 000 positions, reads of 150 bases, 12.5 reads per start, M = 100 (cfg4's shape in small): the plain selection
    uses fewer than a fifth of the occupied starts; K = 1 keeps within 1 % of the plain count on as many starts as it
    keeps reads, and is short only on the two ramps where min(cov, M) needs all the reads of the first few starts.
    (The ramps cost K = 1 about M / 2 reads whatever the length, of M * L / 150 kept: 0.6 % here.)"""
    rng = np.random.default_rng(3)
    L, length, M = 12_000, 150, 100
    n_starts = L - length + 1
    s = rng.integers(0, n_starts, size=int(n_starts * 12.5)).astype(np.uint32)
    e = (s + length - 1).astype(np.uint32)
    ids = np.zeros(s.size, np.uint32)
    plain = sm.unpack(mr.oracle_by_contig(oracle, s, e, ids, [L], M), s.size)
    occupied = np.unique(s).size
    assert np.unique(s[plain]).size < occupied / 5
    keep, capped, st, _ = sm.start_cap(oracle, s, e, ids, [L], M, 1, shortfall=True)
    assert abs(int(keep.sum()) - int(plain.sum())) <= 0.01 * plain.sum()
    assert st["cells_kept"] == keep.sum() == np.unique(s[keep]).size and st["largest_kept_cell"] == 1
    assert st["cells"] == occupied and st["reads_survived"] == occupied
    want = np.minimum(sm.depth(s, e, ids, [L], np.ones(s.size, bool)), M)
    short = np.flatnonzero(sm.depth(s, e, ids, [L], keep) < want)
    assert short.size == st["short_positions"] > 0
    assert ((short < length) | (short >= L - length)).all()
    # K = 4: still no reads lost, fewer positions short, at most four reads a start
    keep4, _, st4, _ = sm.start_cap(oracle, s, e, ids, [L], M, 4, shortfall=True)
    assert abs(int(keep4.sum()) - int(plain.sum())) <= 0.01 * plain.sum()
    assert st4["short_positions"] < st["short_positions"] and st4["largest_kept_cell"] <= 4
    assert st["cells_kept"] > st4["cells_kept"] > np.unique(s[plain]).size


def test_entries_are_declared_listed_and_exported(pkg, tmp_path):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_start_cap_host", "qmcp_hip_solve_start_cap_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
    assert re.search(r"#define QMCP_HIP_ABI_VERSION 5\b", text) and pkg.abi_version() == 5
    assert re.search(r"#define QMCP_START_CAP_SHORTFALL 1u", text) and pkg.START_CAP_SHORTFALL == 1
    # the stats structure: ten u64, three u32, one float, no padding hole -- by name, and against a C99 compile
    S = pkg.StartCapStats
    assert [n for n, _ in S._fields_] == FIELDS and C.sizeof(S) == 96
    assert sum(C.sizeof(t) for _, t in S._fields_) == C.sizeof(S)
    assert set(S().as_dict()) == set(FIELDS)
    m = re.search(r"typedef struct qmcp_hip_start_cap_stats \{(.*?)\} qmcp_hip_start_cap_stats;", text, re.S)
    assert re.findall(r"^\s*(?:uint64_t|uint32_t|float)\s+(\w+);", m.group(1), re.M) == FIELDS
    args = ", ".join(f"offsetof(qmcp_hip_start_cap_stats, {f})" for f in FIELDS)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ '
           f'size_t v[] = {{sizeof(qmcp_hip_start_cap_stats), {args}, QMCP_START_CAP_SHORTFALL}}; '
           'for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]); return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-",
                          "-o", str(exe)], input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [pkg.START_CAP_SHORTFALL]


def test_request_mirror_has_the_start_cap_fields(pkg):
    names = [name for name, _ in pkg.DownsampleRequest._fields_]
    at = names.index("has_thresholds")
    assert names[at + 1:at + 4] == ["start_cap_by_strand", "start_cap", "start_cap_report"]
    types = dict(pkg.DownsampleRequest._fields_)
    assert (types["start_cap"], types["start_cap_by_strand"], types["start_cap_report"]) == (C.c_uint32, C.c_int32, C.c_char_p)
    text = open(os.path.join(ROOT, "genome-downsampler_amd", "host", "include", "qmcp_host_request.h")).read()
    body = re.search(r"typedef struct qmcp_host_downsample_request \{(.*?)\} qmcp_host_downsample_request;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()] == names
    zero = pkg._downsample_request(solver_name="x", in_path="a", out_path="b", max_coverage=1)
    assert zero.start_cap == 0 and zero.start_cap_by_strand == 0 and zero.start_cap_report is None
    set_ = pkg._downsample_request(start_cap=3, start_cap_by_strand=True, start_cap_report="r.tsv")
    assert set_.start_cap == 3 and set_.start_cap_by_strand == 1 and set_.start_cap_report == b"r.tsv"


# ------------------------------------------------------------------------------------------ downsample_bam
def small_bam(tmp_path):
    import bam_py
    import template_bams as tb
    refs = [("chrA", 4000)]
    path = tmp_path / "in.bam"
    bam_py.write_bam(path, refs, tb.single_end_records(np.random.default_rng(1), refs, 50))
    bed = tmp_path / "t.bed"
    bed.write_text("chrA\t10\t500\n")
    graph = tmp_path / "p.bedgraph"
    graph.write_text("chrA\t10\t500\t3\n")
    return path, bed, graph


def test_downsample_bam_refuses_what_a_start_cap_does_not_go_together_with(pkg, tmp_path):
    path, bed, graph = small_bam(tmp_path)
    go = lambda **kw: pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", 4, **kw)
    on = dict(per_reference=True, start_cap=2)
    together = "a start cap does not go together with "
    refused = [
        (dict(start_cap=2), "a start cap needs per_reference=True"),
        (dict(on, thresholds=9), together + "coverage thresholds"), (dict(on, mean_depth=2.0), together + "a mean depth"),
        (dict(on, budget_bases=20), together + "a mean depth"), (dict(on, proportion=0.5), together + "a proportion"),
        (dict(on, replicates=2, replicates_out=tmp_path / "r{R}.bam"), together + "replicates"),
        (dict(on, budget_reads=5), together + "a budget"), (dict(on, budget_fraction=0.5), together + "a budget"),
        (dict(on, ceiling=True), together + "ceiling"), (dict(on, pair_aware=True), together + "pair_aware"),
        (dict(on, template_aware=True), together + "template_aware"), (dict(on, targets=bed), together + "targets"),
        (dict(on, report=tmp_path / "r.tsv"), together + "a depth report"),
        (dict(on, track=tmp_path / "t.bedgraph"), together + "a depth track"),
        (dict(on, ladder=[3], ladder_out=tmp_path / "l{M}.bam"), together + "a coverage ladder"),
        (dict(on, stratify="strand"), together + "stratify"), (dict(on, dedup=True), together + "dedup"),
        (dict(on, profile=graph), together + "a coverage profile"),
        (dict(on, ceiling=True, dedup=True), together + "ceiling"),                      # the first offence is named
        (dict(on, bed=bed, amplicons_by_reference=True), "a start cap does not take amplicon files"),
        (dict(on, tsv=bed), "a start cap does not take amplicon files"),
        (dict(per_reference=True, start_cap_report=tmp_path / "s.tsv"), "start_cap_by_strand and start_cap_report need start_cap"),
        (dict(per_reference=True, start_cap_by_strand=True), "start_cap_by_strand and start_cap_report need start_cap"),
        (dict(start_cap_report=tmp_path / "s.tsv"), "need start_cap"),
        (dict(per_reference=True, start_cap=0), "start_cap must lie in 1"),
        (dict(per_reference=True, start_cap=1 << 32), "start_cap must lie in 1"),
    ]
    for kw, message in refused:
        with pytest.raises(ValueError, match=re.escape(message)):
            go(**kw)
    with pytest.raises(ValueError, match="a start cap does not take a solver that grades by quality"):
        pkg.downsample_bam("quasi-mcp-hip-quality", path, tmp_path / "no.bam", 4, **on)
    assert not (tmp_path / "no.bam").exists() and not (tmp_path / "s.tsv").exists()


def test_host_config_refuses_the_same_combinations(pkg, tmp_path):
    """BamApiConfig's own refusals, reached through the C entry with everything handed on as given"""
    path, bed, _ = small_bam(tmp_path)

    def call(solver="quasi-mcp-hip", per_reference=1, start_cap=2, **more):
        err = C.create_string_buffer(1024)
        request = pkg._downsample_request(solver_name=solver, in_path=path, out_path=tmp_path / "no.bam", max_coverage=4,
                                          min_len=0, min_mapq=0, per_reference=per_reference, start_cap=start_cap, **more)
        n = pkg._host.qmcp_host_downsample_bam(C.byref(request), None, 0, None, None, None, None, None, err, 1024)
        return n, err.value.decode()

    together = "a start cap does not go together with "
    refused = [
        (dict(per_reference=0), "a start cap needs per_reference"),
        (dict(start_cap=0, start_cap_by_strand=1), "start_cap_by_strand and start_cap_report need start_cap"),
        (dict(start_cap=0, start_cap_report=tmp_path / "s.tsv"), "start_cap_by_strand and start_cap_report need start_cap"),
        (dict(has_thresholds=1, thresholds_lo=1, thresholds_hi=9), together + "coverage thresholds"),
        (dict(has_mean_depth=1, mean_depth=2.0), together + "a mean depth"),
        (dict(has_budget_bases=1, budget_bases=20), together + "a mean depth"),
        (dict(has_proportion=1, proportion_num=1, proportion_den=2), together + "a proportion"),
        (dict(has_replicates=1), together + "replicates"),
        (dict(has_budget_reads=1, budget_reads=20), together + "a budget"), (dict(budget_fraction=0.5), together + "a budget"),
        (dict(ceiling=1), together + "ceiling"), (dict(pair_aware=1), together + "pair_aware"),
        (dict(template_aware=1), together + "template_aware"), (dict(targets=bed), together + "targets"),
        (dict(report=tmp_path / "r.tsv"), together + "a depth report"), (dict(track=tmp_path / "t.bg"), together + "a depth track"),
        (dict(ladder_levels=[3]), together + "a coverage ladder"), (dict(stratify="strand"), together + "stratify"),
        (dict(dedup=1), together + "dedup"),
        (dict(has_regions=1, n_refs=1, region_offsets=[0, 0]), together + "a coverage profile"),
        (dict(bed=bed, amplicons_by_reference=1), "a start cap does not take amplicon files"),
        (dict(tsv=bed), "a start cap does not take amplicon files"),
    ]
    for kw, word in refused:
        n, message = call(**kw)
        assert n == -4 and word in message, (kw, n, message)
    n, message = call(solver="quasi-mcp-hip-quality")
    assert n == -4 and "a start cap does not take a solver that grades by quality" in message
    assert call(solver="no-such-solver")[0] == -1
    assert not (tmp_path / "no.bam").exists() and not (tmp_path / "s.tsv").exists()
