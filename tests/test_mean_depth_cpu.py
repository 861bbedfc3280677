"""Mean-depth downsampling, the parts that need no GPU: the model (tests/mean_depth_model.py) respects the bound
bases(M) >= S_R(M) and is monotone on the inputs of the GPU test (which is what makes that test's uniqueness claim say
something); header, library and package agree on the two entries, the flag and the stats struct; the entries refuse on the
host what they refuse (no context is needed for that); the package turns a mean depth into a base budget over the merged,
clipped regions."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mean_depth_model as mm
import multi_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["budget", "positions", "reads_placed", "n_kept", "kept_bases", "bases_above", "bound_above", "total_bases",
          "coverage", "max_depth", "top", "probes", "curve_entries", "saturated", "regions_in", "regions_used",
          "ms_mean_depth", "ms_solves"]
QMCP_EINVAL, QMCP_ERANGE = -1, -3


# ------------------------------------------------------------------------------------------ the model
def inputs(seed):
    """the GPU test's case 1 and 5: random_by_contig(rng, 4, 2500) and regions from a generator of its own"""
    s, e, ids, lengths = mr.random_by_contig(np.random.default_rng(seed), 4, 2500)
    return s, e, ids, lengths, mm.random_regions(np.random.default_rng(1000 + seed), lengths)


def test_region_generator_reaches_every_kind_of_region():
    kinds = {"none": 0, "nested": 0, "overlap": 0, "last": 0, "beyond": 0, "clipped": 0}
    for seed in range(6):
        _, _, _, lengths, (offs, r0, r1) = inputs(seed)
        assert offs.size == lengths.size + 1 and offs[0] == 0 and np.all(np.diff(offs.astype(np.int64)) <= 4)
        for c, length in enumerate(lengths.tolist()):
            regs = [(int(r0[k]), int(r1[k])) for k in range(int(offs[c]), int(offs[c + 1]))]
            kinds["none"] += not regs
            kinds["beyond"] += any(s >= length for s, _ in regs)
            kinds["last"] += any(s < length and e == length - 1 for s, e in regs)
            kinds["clipped"] += any(s < length <= e for s, e in regs)
            for i, (s, e) in enumerate(regs):
                for j, (s2, e2) in enumerate(regs):
                    if i != j:
                        kinds["nested"] += s < s2 and e2 < e
                        kinds["overlap"] += s < s2 <= e < e2
    assert all(kinds.values()), kinds


@pytest.mark.parametrize("seed", range(6))
def test_model_respects_the_bound_and_is_monotone_on_the_gpu_tests_inputs(oracle, seed):
    s, e, ids, lengths, regions = inputs(seed)
    steps = 0
    for reg in (None, regions):
        for pairs in (False, True):
            n = s.size & ~1 if pairs else s.size
            model = mm.Model(oracle, s[:n], e[:n], ids[:n], lengths, 64, regions=reg, whole_pairs=pairs)
            bases, curve = model.all_bases(), model.curve_R().astype(np.int64)
            assert curve.size == model.top + 1 and curve[0] == 0 and bases[0] == 0
            assert np.all(bases >= curve), (seed, reg is not None, pairs)                 # S_R(M) <= bases(M)
            assert np.all(np.diff(bases) >= 0), (seed, reg is not None, pairs, bases)     # observed, not proven
            steps += model.top
            if reg is None:
                assert model.positions == int(lengths.astype(np.int64).sum())
                on = model.ids != mm.NO_CONTIG
                assert model.total_bases == int((model.e[on].astype(np.int64) - model.s[on] + 1).sum())
            if model.top == model.max_depth and not pairs:
                assert bases[model.top] == model.total_bases                              # every placed read kept
            for budget in (0, 1, model.total_bases // 3, model.total_bases):
                assert model.answers(budget) == [model.largest(budget)]
    print(f"seed {seed}: {steps} steps")


def test_membership_is_painted_from_the_raw_regions():
    inside = mm.membership([10, 0, 5], [0, 3, 4, 6], [8, 2, 3, 0, 5, 4], [20, 4, 3, 9, 9, 4])
    assert np.flatnonzero(inside).tolist() == [2, 3, 4, 8, 9, 14]
    assert mm.membership([4, 3], None, None, None).all() and not mm.membership([4, 3], [0, 0, 0], [], []).any()


# ------------------------------------------------------------------------------------------ header, library, package
def test_entries_flag_and_stats_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_mean_depth_host", "qmcp_hip_solve_mean_depth_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
        assert hasattr(pkg._hip, name)
    assert "#define QMCP_MEAN_DEPTH_WHOLE_PAIRS 1u" in text and pkg.MEAN_DEPTH_WHOLE_PAIRS == 1
    assert hasattr(pkg.Solver, "solve_mean_depth") and hasattr(pkg.Solver, "solve_mean_depth_device")
    assert pkg.abi_version() == 5
    body = re.search(r"typedef struct qmcp_hip_mean_depth_stats \{(.*?)\} qmcp_hip_mean_depth_stats;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert declared == FIELDS == [name for name, _ in pkg.MeanDepthStats._fields_]
    comment = text[text.index("/* Mean-depth downsampling"):text.index("#define QMCP_MEAN_DEPTH_WHOLE_PAIRS")]
    assert "NOT proven" in comment                  # the header promises (1) and (2) only


def test_mean_depth_stats_layout_matches_the_header_which_is_c99(pkg, tmp_path):
    args = ", ".join(f"offsetof(qmcp_hip_mean_depth_stats, {f})" for f in FIELDS)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ '
           f'size_t v[] = {{sizeof(qmcp_hip_mean_depth_stats), {args}}}; '
           'for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]); return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c",
                          "-", "-o", str(exe)], input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = pkg.MeanDepthStats
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS]
    assert C.sizeof(S) == 8 * 8 + 8 * 4 + 2 * 4


def test_entries_refuse_on_the_host_before_a_context_is_needed(pkg):
    """every refusal is decided from the arguments alone: a NULL context is never looked at, the mask never written"""
    s, e, ids = (np.zeros(4, np.uint32) for _ in range(3))
    lengths = np.array([10, 20], np.uint32)
    mask = np.full(1, 0xDEADBEEF, np.uint64)
    curve = np.zeros(4, np.uint64)
    offs, r0, r1 = np.array([0, 1, 2], np.uint32), np.array([1, 30], np.uint32), np.array([5, 40], np.uint32)
    p32, p64 = pkg._p32, pkg._p64

    def host(starts=s, ends=e, cids=ids, n=4, lens=lengths, n_contigs=2, M=5, budget=2, ro=None, rs=None, re_=None,
             flags=0, table=None, cap=0, out=mask):
        rc = pkg._hip.qmcp_hip_solve_mean_depth_host(None, p32(starts), p32(ends), p32(cids), n, p32(lens), n_contigs, M,
                                                     budget, p32(ro), p32(rs), p32(re_), flags, p64(table), cap, p64(out),
                                                     None, None)
        return rc, pkg._hip.qmcp_hip_last_error().decode()

    def device(n=4, lens=lengths, n_contigs=2, M=5, ro=None, rs=None, re_=None, flags=0, d=0x1000, d_mask=0x1000):
        rc = pkg._hip.qmcp_hip_solve_mean_depth_device(None, C.c_void_p(d), C.c_void_p(d), C.c_void_p(d), n, p32(lens),
                                                       n_contigs, M, 2, p32(ro), p32(rs), p32(re_), flags, None, 0,
                                                       C.c_void_p(d_mask), None, None, None)
        return rc, pkg._hip.qmcp_hip_last_error().decode()

    u = lambda *v: np.array(v, np.uint32)
    many = np.zeros(3, np.uint32)
    refused = [
        # the budget entry's, word for word
        (host(starts=None), QMCP_EINVAL, "null buffer"), (host(ends=None), QMCP_EINVAL, "null buffer"),
        (host(cids=None), QMCP_EINVAL, "null buffer"), (host(out=None), QMCP_EINVAL, "null buffer"),
        (host(lens=None), QMCP_EINVAL, "contig_lengths"), (host(n_contigs=0), QMCP_EINVAL, "contig_lengths"),
        (host(flags=2), QMCP_EINVAL, "unknown flag"), (host(flags=0x80000001), QMCP_EINVAL, "unknown flag"),
        (host(n=3, flags=pkg.MEAN_DEPTH_WHOLE_PAIRS), QMCP_EINVAL, "odd"),
        (host(M=0), QMCP_EINVAL, "max_coverage == 0"),
        (host(M=1 << 31), QMCP_ERANGE, "2\\^31"), (host(M=0xFFFFFFFF), QMCP_ERANGE, "2\\^31"),
        (host(table=None, cap=3), QMCP_EINVAL, "curve_capacity"),
        (host(lens=many, n_contigs=(1 << 24) + 1), QMCP_ERANGE, "n_contigs"),
        (host(n=(1 << 31) + 2), QMCP_ERANGE, "n_reads"),
        (device(d=0), QMCP_EINVAL, "null buffer"), (device(d_mask=0), QMCP_EINVAL, "null buffer"),
        (device(lens=None), QMCP_EINVAL, "contig_lengths"), (device(flags=4), QMCP_EINVAL, "unknown flag"),
        (device(n=5, flags=pkg.MEAN_DEPTH_WHOLE_PAIRS), QMCP_EINVAL, "odd"), (device(M=0), QMCP_EINVAL, "max_coverage == 0"),
        (device(M=1 << 31), QMCP_ERANGE, "2\\^31"), (device(n=(1 << 31) + 2), QMCP_ERANGE, "n_reads"),
        # the targets entry's, for the region table
        (host(ro=u(1, 1, 2), rs=r0, re_=r1), QMCP_EINVAL, "region_offsets"),
        (host(ro=u(0, 2, 1), rs=r0, re_=r1), QMCP_EINVAL, "region_offsets"),
        (host(ro=offs, rs=None, re_=r1), QMCP_EINVAL, "null region table"),
        (host(ro=offs, rs=r0, re_=None), QMCP_EINVAL, "null region table"),
        (host(ro=offs, rs=u(6, 30), re_=r1), QMCP_EINVAL, "start > end"),
        (device(ro=u(0, 2, 1), rs=r0, re_=r1), QMCP_EINVAL, "region_offsets"),
        (device(ro=offs, rs=None, re_=r1), QMCP_EINVAL, "null region table"),
        (device(ro=offs, rs=r0, re_=u(5, 29)), QMCP_EINVAL, "start > end"),
    ]
    for (rc, message), want, word in refused:
        assert rc == want and re.search(word, message), (rc, message, want, word)
    # what is NOT refused gets as far as the context: valid arguments, the flag on an even count, a curve, a table (one
    # region beyond its contig), an empty table with NULL columns
    for rc, message in (host(), host(flags=pkg.MEAN_DEPTH_WHOLE_PAIRS), host(M=(1 << 31) - 1), host(table=curve, cap=4),
                        host(ro=offs, rs=r0, re_=r1), host(ro=u(0, 0, 0)), host(budget=(1 << 64) - 1), device(),
                        device(ro=offs, rs=r0, re_=r1)):
        assert rc == QMCP_EINVAL and "null context" in message, (rc, message)
    assert mask[0] == 0xDEADBEEF


def test_python_turns_a_mean_depth_into_a_base_budget_over_the_merged_clipped_regions(pkg):
    pos = pkg.region_positions
    lengths = [100, 50, 0, 30]
    # contig 0: [10, 19] and [15, 29] overlap, [12, 13] is nested, [30, 34] is adjacent -> 10 .. 34 = 25; [90, 200] is
    # clipped -> 10; contig 1: [50, 60] begins at the length: dropped; [49, 49] -> 1; contig 2 has no position;
    # contig 3: the same region twice -> 5
    offs = [0, 5, 7, 8, 10]
    r0 = [15, 10, 12, 90, 30, 50, 49, 0, 3, 3]
    r1 = [29, 19, 13, 200, 34, 60, 49, 5, 7, 7]
    assert pos(lengths, offs, r0, r1) == 25 + 10 + 1 + 0 + 5 == int(mm.membership(lengths, offs, r0, r1).sum())
    assert pos(lengths, None, None, None) == 180 and pos(lengths, [0, 0, 0, 0, 0], None, None) == 0
    for seed in range(6):                                           # and the generator's regions, against the painted array
        _, _, _, lens, (o, a, b) = inputs(seed)
        assert pos(lens, o, a, b) == int(mm.membership(lens, o, a, b).sum())
    with pytest.raises(ValueError):
        pos(lengths, [0, 1], [0], [1])
    f = pkg.Solver._base_budget_of
    assert f(None, 7, None) == 7 and f(None, 1 << 63, None) == 1 << 63 and f(None, 0, None) == 0
    assert f(30.0, None, 41) == 1230 and f(0.5, None, 41) == 20 and f(2.999, None, 1000) == 2999 and f(0.0, None, 41) == 0
    assert f(100.0, None, 0) == 0
    for args in ((None, None, 5), (3.0, 7, 5), (None, -1, 5), (None, 1 << 64, 5), (-0.5, None, 5), (float("nan"), None, 5),
                 (float("inf"), None, 5), (1e30, None, 5)):
        with pytest.raises(ValueError):
            f(*args)


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


def test_downsample_bam_mean_depth_refuses_what_it_does_not_go_together_with(pkg, tmp_path):
    path, bed, graph = small_bam(tmp_path)
    go = lambda **kw: pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", 4, **kw)
    on = dict(per_reference=True, mean_depth=2.0)
    refused = [
        (dict(mean_depth=2.0), "per_reference"), (dict(budget_bases=20), "per_reference"),
        (dict(on, budget_bases=20), "not both"), (dict(per_reference=True, mean_depth=-0.5), "finite"),
        (dict(per_reference=True, mean_depth=float("nan")), "finite"), (dict(per_reference=True, budget_bases=-1), "64-bit"),
        (dict(per_reference=True, budget_bases=1 << 64), "64-bit"),
        (dict(on, proportion=0.5), "a proportion"), (dict(on, replicates=2, replicates_out=tmp_path / "r{R}.bam"), "replicates"),
        (dict(on, budget_reads=5), "a budget"), (dict(on, budget_fraction=0.5), "a budget"),
        (dict(on, targets=bed), "targets"), (dict(on, report=tmp_path / "r.tsv"), "depth report"),
        (dict(on, track=tmp_path / "t.bedgraph"), "depth track"),
        (dict(on, ladder=[3], ladder_out=tmp_path / "l{M}.bam"), "ladder"), (dict(on, stratify="strand"), "stratify"),
        (dict(on, dedup=True), "dedup"), (dict(on, profile=graph), "profile"), (dict(on, pair_aware=True), "pair_aware"),
        (dict(on, template_aware=True), "template_aware"), (dict(on, ceiling=True), "ceiling"),
        (dict(on, bed=bed, amplicons_by_reference=True), "amplicon"), (dict(on, tsv=bed), "amplicon"),
        (dict(per_reference=True, mean_depth_report=tmp_path / "m.tsv"), "mean_depth_report"),
        (dict(per_reference=True, mean_depth_targets=bed), "mean_depth_targets"),
        (dict(mean_depth_report=tmp_path / "m.tsv"), "mean_depth_report"),
    ]
    for kw, word in refused:
        with pytest.raises(ValueError, match=word):
            go(**kw)
    with pytest.raises(ValueError, match="quality"):
        pkg.downsample_bam("quasi-mcp-hip-quality", path, tmp_path / "no.bam", 4, **on)
    assert not (tmp_path / "no.bam").exists() and not (tmp_path / "m.tsv").exists()


def test_host_config_refuses_the_same_combinations(pkg, tmp_path):
    """BamApiConfig's own refusals, reached through the C entry with everything handed on as given"""
    path, bed, _ = small_bam(tmp_path)

    def call(solver="quasi-mcp-hip", per_reference=1, has_mean=1, mean=2.0, has_bases=0, bases=0, **more):
        err = C.create_string_buffer(1024)
        request = pkg._downsample_request(
            solver_name=solver, in_path=path, out_path=tmp_path / "no.bam", max_coverage=4, min_len=0, min_mapq=0,
            per_reference=per_reference, has_mean_depth=has_mean, mean_depth=mean, has_budget_bases=has_bases,
            budget_bases=bases, **more)
        n = pkg._host.qmcp_host_downsample_bam(C.byref(request), None, 0, None, None, None, None, None, err, 1024)
        return n, err.value.decode()

    refused = [
        (dict(per_reference=0), "per_reference"), (dict(has_bases=1, bases=7), "not both"),
        (dict(mean=-1.0), "finite"), (dict(mean=float("nan")), "finite"), (dict(mean=float("inf")), "finite"),
        (dict(has_mean=0, mean_depth_report=tmp_path / "m.tsv"), "needs mean_depth or budget_bases"),
        (dict(has_mean=0, mean_depth_targets=bed), "needs mean_depth or budget_bases"),
        (dict(has_proportion=1, proportion_num=1, proportion_den=2), "a proportion"), (dict(has_replicates=1), "replicates"),
        (dict(has_budget_reads=1, budget_reads=20), "a budget"), (dict(budget_fraction=0.5), "a budget"),
        (dict(targets=bed), "targets"), (dict(report=tmp_path / "r.tsv"), "depth report"),
        (dict(track=tmp_path / "t.bg"), "depth track"), (dict(ladder_levels=[3]), "ladder"), (dict(stratify="strand"), "stratify"),
        (dict(dedup=1), "dedup"), (dict(pair_aware=1), "pair_aware"), (dict(template_aware=1), "template_aware"),
        (dict(ceiling=1), "ceiling"), (dict(bed=bed, amplicons_by_reference=1), "amplicon"), (dict(tsv=bed), "amplicon"),
        (dict(has_regions=1, n_refs=1, region_offsets=[0, 0]), "coverage profile"),
        (dict(mean_depth_targets=tmp_path / "t.bedgraph.missing"), "missing"),
    ]
    for kw, word in refused:
        n, message = call(**kw)
        assert n == -4 and word in message, (kw, n, message)
        assert message.startswith("mean-depth downsampling") or word in ("missing", "finite"), message
    bad = tmp_path / "bad.bed"
    bad.write_text("chrZ\t1\t5\n")
    n, message = call(mean_depth_targets=bad)
    assert n == -4 and "chrZ" in message
    n, message = call(solver="quasi-mcp-hip-quality")
    assert n == -4 and "quality" in message
    assert call(solver="no-such-solver")[0] == -1
    assert not (tmp_path / "no.bam").exists() and not (tmp_path / "m.tsv").exists()


def test_request_mirror_has_the_new_fields_beside_the_budget_fields(pkg):
    names = [name for name, _ in pkg.DownsampleRequest._fields_]
    at = names.index("budget_fraction")
    assert names[at + 1:at + 5] == ["mean_depth_targets", "mean_depth_report", "budget_bases", "mean_depth"]
    at = names.index("has_budget_reads")
    assert names[at + 1:at + 3] == ["has_budget_bases", "has_mean_depth"]
    zero = pkg._downsample_request(solver_name="x", in_path="a", out_path="b", max_coverage=1)
    assert not zero.has_mean_depth and not zero.has_budget_bases and zero.mean_depth_targets is None   # not given is zero
