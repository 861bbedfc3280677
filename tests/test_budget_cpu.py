"""Budget downsampling, the parts that need no GPU: the model (tests/budget_model.py) is monotone without pair completion
and keeps every placed read at the largest depth; the host-side planner (genome-downsampler_amd/csrc/budget_plan.h)
compiled with g++ alone into tests/cpp/budget_plan_driver.cpp ends on the boundary within its probe limit; header, library
and package agree on the two entries, the flag and the stats struct; the entries refuse on the host what they refuse
(no context is needed for that); downsample_bam(budget_...=) refuses what it does not go together with."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bam_py
import budget_model as bm
import multi_reference as mr
import template_bams as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["budget", "reads_placed", "n_kept", "kept_above", "bound_above", "total_bases", "coverage", "max_depth", "top",
          "probes", "curve_entries", "saturated", "ms_budget", "ms_solves"]
QMCP_EINVAL, QMCP_ERANGE = -1, -3


# ------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("seed", range(10))
def test_model_count_is_monotone_and_the_largest_depth_keeps_every_placed_read(oracle, seed):
    s, e, ids, lengths = mr.random_by_contig(np.random.default_rng(seed), 3, 1200)
    model = bm.Model(oracle, s, e, ids, lengths, 1 << 30)
    assert model.top == model.max_depth
    counts = model.all_counts()
    assert counts[0] == 0 and np.all(np.diff(counts) >= 0), counts
    assert counts[model.top] == model.placed
    assert not model.bits(model.top)[ids == bm.NO_CONTIG].any()
    curve = model.curve()
    assert curve[0] == 0 and curve[-1] == model.total_bases or model.top > bm.CURVE_MAX
    assert np.all(np.diff(curve.astype(np.int64), 2) <= 0)          # S is concave: its steps are the suffix counts
    for budget in (0, 1, model.placed // 3, model.placed - 1, model.placed):
        assert model.answers(budget) == [model.largest(budget)]     # monotone: one answer
    # the bound of the planner: an answer at M holds at least S(M) bases in reads of at most max_span bases
    on = ids != bm.NO_CONTIG
    if on.any():
        max_span = int((e[on].astype(np.int64) - s[on] + 1).max())
        assert np.all(counts[:curve.size] * max_span >= curve.astype(np.int64))


def test_model_completes_pairs_among_the_placed_reads_only(oracle):
    s = np.array([0, 50, 0, 0, 5, 0], np.uint32)
    e = np.array([9, 59, 9, 0, 14, 0], np.uint32)
    ids = np.array([0, 0, 0, bm.NO_CONTIG, 0, bm.NO_CONTIG], np.uint32)
    plain = bm.Model(oracle, s, e, ids, [100], 5)
    whole = bm.Model(oracle, s, e, ids, [100], 5, whole_pairs=True)
    for M in range(plain.top + 1):
        b, w = plain.bits(M), whole.bits(M)
        assert np.array_equal(w, bm.complete_pairs(b, ids)) and not w[[3, 5]].any()
        assert np.all(w[b]) and w[0] == w[1]
    assert whole.answers(10) == [whole.top] and plain.answers(0) == [0]


# ------------------------------------------------------------------------------------------ the planner
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("budget_plan") / "budget_plan_driver"
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "budget_plan_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def ask(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = [dict(kv.split("=", 1) for kv in row.split()) for row in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def step_functions():
    """(name, top, count(M) for M >= 1, the driver's curve and count parameters): monotone, with their true curves.
    linear: P positions of depth top under reads of span w -- count(M) = (P / w) * M + extra, S(M) = P * M.
    jump / constant: one position of depth top, S(M) = M, spans up to top -- the bound says no more than count >= 1."""
    out = []
    for top in (1, 2, 3, 1000, 10 ** 6):
        curve_n = min(top, bm.CURVE_MAX) + 1
        for a, w, extra in ((1, 1, 0), (7, 150, 0), (3, 40, 11)):
            out.append((f"linear a={a} w={w} +{extra} top={top}", top, (lambda M, a=a, x=extra: a * M + x),
                        f"{w} {curve_n} {a * w} {top} L {a} {extra} 0"))
        for jump in sorted({1, 2, top // 2 + 1, top}):
            out.append((f"jump at {jump} top={top}", top, (lambda M, j=jump: 5 if M < j else 5000),
                        f"{top} {curve_n} 1 {top} J {jump} 5 5000"))
        out.append((f"constant top={top}", top, (lambda M: 9), f"{top} {curve_n} 1 {top} J 1 9 9"))
    return out


def budgets_of(top, count):
    ms = range(1, top + 1) if top <= 1000 else sorted({1, 2, 3, 17, 8190, 8191, 8192, 8193, 123_456, top // 2, top - 1, top})
    values = sorted({count(M) for M in ms})
    return sorted({0, 1, values[-1] + 1, values[-1] * 3, 1 << 63} | {max(v + d, 0) for v in values for d in (-1, 0, 1)})


def boundary(top, count, budget):
    """the largest coverage in 0 .. top within the budget (count monotone, count(0) = 0)"""
    lo, hi = 0, top + 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if count(mid) <= budget else (lo, mid)
    return lo


def test_planner_ends_on_the_boundary_of_monotone_step_functions_within_its_limits(driver):
    lines, want = [], []
    for name, top, count, params in step_functions():
        budgets = budgets_of(top, count)
        if top == 1000:
            budgets = budgets[::7] + budgets[-3:]
        for budget in budgets:
            lines.append(f"{top} {budget} {params}")
            want.append((name, top, count, budget))
    rows = ask(driver, lines)
    most = 0
    for (name, top, count, budget), row in zip(want, rows):
        where = (name, budget, row)
        m, probes = int(row["m"]), int(row["probes"])
        assert m == boundary(top, count, budget), where                          # the one boundary
        assert int(row["limit"]) == bm.probe_limit(top) and probes <= int(row["limit"]), where
        assert int(row["outside"]) == 0 and int(row["twice"]) == 0, where
        seq = [int(x) for x in row["seq"].split(",")] if row.get("seq") else []
        assert len(seq) == probes == len(set(seq)) and all(1 <= M <= top for M in seq), where
        assert int(row["count"]) == (count(m) if m else 0), where
        if m < top:                                                              # what rules m + 1 out
            assert int(row["hi"]) == m + 1
            assert int(row["above"]) == count(m + 1) or (int(row["above"]) == 0 and 0 < int(row["bound"]) <= count(m + 1)), where
            assert int(row["above"]) > budget or int(row["bound"]) > budget, where
        if budget == 0:
            assert probes == 0 and m == 0, where                                 # the bound alone: count(1) >= 1 > 0
        most = max(most, probes)
    print(f"{len(rows)} searches, at most {most} probes")


def test_planner_first_probe_is_exact_on_one_read_length(driver):
    # P = 1050 positions of depth 1000 under reads of span 150: count(M) = 7 M; the mean span is the span
    for budget, m in ((7 * 400, 400), (7 * 400 + 6, 400), (7 * 999, 999)):
        row = ask(driver, [f"1000 {budget} 150 1001 1050 1000 L 7 0 0"])[0]
        seq = [int(x) for x in row["seq"].split(",")]
        assert int(row["m"]) == m and seq[0] == m and int(row["probes"]) <= 2, row


def test_planner_keeps_properties_one_and_two_on_functions_that_are_not_monotone(driver):
    rng = np.random.default_rng(18)
    lines, cases = [], []
    for _ in range(300):
        top = int(rng.integers(1, 40))
        if rng.random() < 0.5:      # a bound that says next to nothing: S(M) = M, spans up to top
            table = rng.integers(1, 60, top)
            max_span = top
        else:                       # a bound with teeth that is still true: count(M) >= ceil(M / 2) = ceil(S(M) / 2)
            table = np.array([(M + 1) // 2 + int(rng.integers(0, 12)) for M in range(1, top + 1)])
            max_span = 2
        budget = int(rng.integers(0, 70))
        lines.append(f"{top} {budget} {max_span} {top + 1} 1 {top} T 0 0 0 " + " ".join(map(str, table)))
        cases.append((top, budget, [0] + table.tolist()))
    for (top, budget, count), row in zip(cases, ask(driver, lines)):
        m = int(row["m"])
        assert 0 <= m <= top and count[m] <= budget, (row, count)                # (1)
        assert m == top or count[m + 1] > budget, (row, count)                   # (2)
        assert int(row["probes"]) <= int(row["limit"]) and int(row["outside"]) == 0 and int(row["twice"]) == 0, row
        assert int(row["count"]) == count[m]
        if m < top and int(row["above"]) == 0:
            assert budget < int(row["bound"]) <= count[m + 1], (row, count)


# ------------------------------------------------------------------------------------------ header, library, package
def test_entries_flag_and_stats_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_budget_host", "qmcp_hip_solve_budget_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
        assert hasattr(pkg._hip, name)
    assert "#define QMCP_BUDGET_WHOLE_PAIRS 1u" in text and pkg.BUDGET_WHOLE_PAIRS == 1
    assert "#define QMCP_BUDGET_CURVE_MAX 8191u" in text and pkg.BUDGET_CURVE_MAX == 8191 == bm.CURVE_MAX
    assert hasattr(pkg.Solver, "solve_budget") and hasattr(pkg.Solver, "solve_budget_device")
    assert pkg.abi_version() == 5
    body = re.search(r"typedef struct qmcp_hip_budget_stats \{(.*?)\} qmcp_hip_budget_stats;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert declared == FIELDS == [name for name, _ in pkg.BudgetStats._fields_]
    assert "NOT proven" in text                     # the header says what is only observed under the flag
    host_nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HOST_LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T qmcp_host_downsample_bam\b", host_nm)


def test_budget_stats_layout_matches_the_header_which_is_c99(pkg, tmp_path):
    args = ", ".join(f"offsetof(qmcp_hip_budget_stats, {f})" for f in FIELDS)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ '
           f'size_t v[] = {{sizeof(qmcp_hip_budget_stats), {args}}}; '
           'for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]); return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c",
                          "-", "-o", str(exe)], input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = pkg.BudgetStats
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS]
    assert C.sizeof(S) == 80


def test_entries_refuse_on_the_host_before_a_context_is_needed(pkg):
    """every refusal is decided from the arguments alone: a NULL context is never looked at, the mask never written"""
    s, e, ids = (np.zeros(4, np.uint32) for _ in range(3))
    lengths = np.array([10], np.uint32)
    mask = np.full(1, 0xDEADBEEF, np.uint64)
    curve = np.zeros(4, np.uint64)
    p32, p64 = pkg._p32, pkg._p64

    def host(starts=s, ends=e, cids=ids, n=4, lens=lengths, n_contigs=1, M=5, budget=2, flags=0, table=None, cap=0, out=mask):
        rc = pkg._hip.qmcp_hip_solve_budget_host(None, p32(starts), p32(ends), p32(cids), n, p32(lens), n_contigs, M, budget,
                                                 flags, p64(table), cap, p64(out), None, None)
        return rc, pkg._hip.qmcp_hip_last_error().decode()

    def device(n=4, lens=lengths, n_contigs=1, M=5, flags=0, d=0x1000, d_mask=0x1000):
        rc = pkg._hip.qmcp_hip_solve_budget_device(None, C.c_void_p(d), C.c_void_p(d), C.c_void_p(d), n, p32(lens),
                                                   n_contigs, M, 2, flags, None, 0, C.c_void_p(d_mask), None, None, None)
        return rc, pkg._hip.qmcp_hip_last_error().decode()

    refused = [
        (host(starts=None), QMCP_EINVAL, "null buffer"), (host(ends=None), QMCP_EINVAL, "null buffer"),
        (host(cids=None), QMCP_EINVAL, "null buffer"), (host(out=None), QMCP_EINVAL, "null buffer"),
        (host(lens=None), QMCP_EINVAL, "contig_lengths"), (host(n_contigs=0), QMCP_EINVAL, "contig_lengths"),
        (host(flags=2), QMCP_EINVAL, "unknown flag"), (host(flags=0x80000001), QMCP_EINVAL, "unknown flag"),
        (host(n=3, flags=pkg.BUDGET_WHOLE_PAIRS), QMCP_EINVAL, "odd"),
        (host(M=0), QMCP_EINVAL, "max_coverage == 0"),
        (host(M=1 << 31), QMCP_ERANGE, "2\\^31"), (host(M=0xFFFFFFFF), QMCP_ERANGE, "2\\^31"),
        (host(table=None, cap=3), QMCP_EINVAL, "curve_capacity"),
        (device(d=0), QMCP_EINVAL, "null buffer"), (device(d_mask=0), QMCP_EINVAL, "null buffer"),
        (device(lens=None), QMCP_EINVAL, "contig_lengths"), (device(flags=4), QMCP_EINVAL, "unknown flag"),
        (device(n=5, flags=pkg.BUDGET_WHOLE_PAIRS), QMCP_EINVAL, "odd"), (device(M=0), QMCP_EINVAL, "max_coverage == 0"),
        (device(M=1 << 31), QMCP_ERANGE, "2\\^31"),
    ]
    for (rc, message), want, word in refused:
        assert rc == want and re.search(word, message), (rc, message, want, word)
    # what is NOT refused gets as far as the context: valid arguments, an even count under the flag, a curve
    for rc, message in (host(), host(flags=pkg.BUDGET_WHOLE_PAIRS), host(M=(1 << 31) - 1), host(table=curve, cap=4), device()):
        assert rc == QMCP_EINVAL and "null context" in message, (rc, message)
    assert mask[0] == 0xDEADBEEF


def test_python_budget_arguments(pkg):
    f = pkg.Solver._budget_of
    assert f(7, None, 100) == 7 and f(None, 0.5, 101) == 50 and f(None, 1.0, 33) == 33 and f(None, 0.0, 33) == 0
    assert f(1 << 63, None, None) == 1 << 63
    for args in ((None, None, 5), (3, 0.5, 5), (-1, None, 5), (1 << 64, None, 5), (None, 1.5, 5), (None, -0.1, 5),
                 (None, 0.5, None)):
        with pytest.raises(ValueError):
            f(*args)


# ------------------------------------------------------------------------------------------ downsample_bam
def test_downsample_bam_budget_refuses_what_it_does_not_go_together_with(pkg, tmp_path):
    refs = [("chrA", 4000)]
    path = tmp_path / "in.bam"
    bam_py.write_bam(path, refs, tb.single_end_records(np.random.default_rng(1), refs, 50))
    bed = tmp_path / "t.bed"
    bed.write_text("chrA\t10\t500\n")
    graph = tmp_path / "p.bedgraph"
    graph.write_text("chrA\t10\t500\t3\n")
    go = lambda **kw: pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", 4, **kw)
    on = dict(per_reference=True, budget_reads=20)
    refused = [
        (dict(budget_reads=20), "per_reference"), (dict(budget_fraction=0.5), "per_reference"),
        (dict(on, budget_fraction=0.5), "not both"), (dict(per_reference=True, budget_fraction=1.5), "0 .. 1"),
        (dict(per_reference=True, budget_fraction=-0.5), "0 .. 1"), (dict(per_reference=True, budget_reads=-1), "64-bit"),
        (dict(on, targets=bed), "targets"), (dict(on, report=tmp_path / "r.tsv"), "depth report"),
        (dict(on, track=tmp_path / "t.bedgraph"), "depth track"),
        (dict(on, ladder=[3], ladder_out=tmp_path / "l{M}.bam"), "ladder"), (dict(on, stratify="strand"), "stratify"),
        (dict(on, dedup=True), "dedup"), (dict(on, profile=graph), "profile"), (dict(on, pair_aware=True), "pair_aware"),
        (dict(on, template_aware=True), "template_aware"), (dict(on, ceiling=True), "ceiling"),
        (dict(on, bed=bed, amplicons_by_reference=True), "amplicon"), (dict(on, tsv=bed), "amplicon"),
        (dict(per_reference=True, budget_report=tmp_path / "b.tsv"), "budget_report"),
        (dict(budget_report=tmp_path / "b.tsv"), "budget_report"),
        (dict(on, budget_fraction=0.5, budget_report=tmp_path / "b.tsv"), "budget_report"),
    ]
    for kw, word in refused:
        with pytest.raises(ValueError, match=word):
            go(**kw)
    with pytest.raises(ValueError, match="quality"):
        pkg.downsample_bam("quasi-mcp-hip-quality", path, tmp_path / "no.bam", 4, **on)
    assert not (tmp_path / "no.bam").exists() and not (tmp_path / "b.tsv").exists()


def test_host_config_refuses_the_same_combinations(pkg, tmp_path):
    """BamApiConfig's own refusals, reached through the C entry with everything handed on as given.  A request with
    neither budget is no budget request at all, so that case names a budget report, which asks for the mode"""
    refs = [("chrA", 4000)]
    path = tmp_path / "in.bam"
    bam_py.write_bam(path, refs, tb.single_end_records(np.random.default_rng(2), refs, 50))
    bed = tmp_path / "t.bed"
    bed.write_text("chrA\t10\t500\n")

    def call(solver=b"quasi-mcp-hip", per_reference=1, has_reads=1, reads=20, fraction=-1.0, targets=None, report=None,
             track=None, ladder=None, stratify=None, dedup=0, pair_aware=0, template_aware=0, ceiling=0, bed_=None, tsv=None,
             by_ref=0, budget_report=None):
        err = C.create_string_buffer(1024)
        request = pkg._downsample_request(
            solver_name=solver.decode(), in_path=path, out_path=tmp_path / "no.bam", max_coverage=4, min_len=0, min_mapq=0,
            per_reference=per_reference, has_budget_reads=has_reads, budget_reads=reads, budget_fraction=fraction,
            targets=targets, report=report, track=track, ladder_levels=ladder, stratify=stratify, dedup=dedup,
            pair_aware=pair_aware, template_aware=template_aware, ceiling=ceiling, bed=bed_, tsv=tsv,
            amplicons_by_reference=by_ref, budget_report=budget_report)
        n = pkg._host.qmcp_host_downsample_bam(C.byref(request), None, 0, None, None, None, None, None, err, 1024)
        return n, err.value.decode()

    refused = [
        (dict(per_reference=0), "per_reference"), (dict(has_reads=0, budget_report=tmp_path / "b.tsv"), "needs budget_reads or budget_fraction"),
        (dict(fraction=0.5), "not both"), (dict(has_reads=0, fraction=1.5), "0 .. 1"),
        (dict(has_reads=0, fraction=float("nan")), "0 .. 1"),
        (dict(targets=bed), "targets"), (dict(report=tmp_path / "r.tsv"), "depth report"),
        (dict(track=tmp_path / "t.bg"), "depth track"), (dict(ladder=[3]), "ladder"), (dict(stratify="strand"), "stratify"),
        (dict(dedup=1), "dedup"), (dict(pair_aware=1), "pair_aware"), (dict(template_aware=1), "template_aware"),
        (dict(ceiling=1), "ceiling"), (dict(bed_=bed, by_ref=1), "amplicon"), (dict(tsv=bed), "amplicon"),
    ]
    for kw, word in refused:
        n, message = call(**kw)
        assert n == -4 and word in message, (kw, n, message)
    assert call(solver=b"no-such-solver")[0] == -1
    assert not (tmp_path / "no.bam").exists() and not (tmp_path / "b.tsv").exists()
