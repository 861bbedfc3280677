"""Fragment depth without a GPU: tests/fragment_model.py's clip against a brute-force fragment depth that does not use
it, the staged solve on clipped columns, the issue's contrast input, the host-side plan (fragment_plan.h under g++ alone,
tests/cpp/fragment_plan_driver.cpp), and the interface: the four entries, the stats layout, the header's words, the
argument errors that need no context, the request's new fields, and the refusals of downsample_bam and BamApiConfig."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bam_py
import fragment_model as fm
import profile_model as pm
import template_bams as tb
import template_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QMCP_OK, QMCP_EINVAL, QMCP_ERANGE = 0, -1, -3
NO_CONTIG = 0xFFFFFFFF
ENTRIES = ("qmcp_hip_clip_templates_host", "qmcp_hip_clip_templates_device", "qmcp_hip_solve_fragments_host",
           "qmcp_hip_solve_fragments_device")


def random_call(rng):
    lengths = rng.integers(150, 900, size=int(rng.integers(1, 4))).astype(np.uint32)
    n = int(rng.integers(0, 260))
    large = int(rng.integers(0, 60)) if rng.random() < 0.5 else 0
    spare = None if rng.random() < 0.5 else n + 9
    s, e, ids, tids, n_templates = fm.random_fragments(rng, n, lengths, n_templates=spare, large=large)
    return s, e, ids, tids, n_templates, lengths


# ------------------------------------------------------------------------------------------ the model
def test_clip_on_300_random_calls():
    rng = np.random.default_rng(2024)
    seen = dict.fromkeys(("n_clipped", "n_emptied", "abutting", "other_contig", "unplaced"), 0)
    for _ in range(300):
        s, e, ids, tids, n_templates, lengths = random_call(rng)
        n = s.size
        cs, cc, stats = fm.clip(s, e, ids, tids)
        # the clipped segments of a template are pairwise disjoint: per-segment depth of one template never exceeds 1
        placed = np.flatnonzero(cc != NO_CONTIG)
        for t in np.unique(tids[placed]).tolist():
            rows = placed[tids[placed] == t]
            assert all(int(d.max(initial=0)) <= 1 for d in fm.segment_depth(cs[rows], e[rows], cc[rows], lengths))
        # per-segment depth of the clipped columns is the fragment depth of all rows, computed without clip
        want = fm.fragment_depth(s, e, ids, tids, lengths)
        got = fm.segment_depth(cs, e, cc, lengths)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        # idempotent
        cs2, cc2, stats2 = fm.clip(cs, e, cc, tids)
        assert np.array_equal(cs2, cs) and np.array_equal(cc2, cc)
        assert stats2["n_clipped"] == stats2["n_emptied"] == stats2["bases_removed"] == 0
        # bases_removed is the depth difference
        before = sum(int(d.sum()) for d in fm.segment_depth(s, e, ids, lengths))
        assert stats["bases_in"] == before and stats["bases_removed"] == before - sum(int(d.sum()) for d in want)
        # ends never change, only placed rows change, a clipped start lies inside its segment
        moved = cs != s
        assert (cs[moved] > s[moved]).all() and (cs[moved] <= e[moved]).all() and (ids[moved] != NO_CONTIG).all()
        assert stats["n_clipped"] == int(moved.sum()) and stats["n_emptied"] == int(((cc != ids)).sum())
        assert stats["n_placed"] == int((ids != NO_CONTIG).sum())
        for k in ("n_clipped", "n_emptied"):
            seen[k] += stats[k]
        seen["unplaced"] += int((ids == NO_CONTIG).sum())
        order = np.lexsort((s, ids, tids))
        same = (tids[order][1:] == tids[order][:-1]) & (ids[order][1:] == ids[order][:-1]) & (ids[order][1:] != NO_CONTIG)
        seen["abutting"] += int((same & (s[order][1:].astype(np.int64) == e[order][:-1].astype(np.int64) + 1)).sum())
        seen["other_contig"] += int(sum(np.unique(ids[(tids == t) & (ids != NO_CONTIG)]).size > 1
                                        for t in np.unique(tids).tolist()))
    assert all(v > 100 for v in seen.values()), seen


def test_staged_on_clipped_columns_holds_whole_templates_and_the_fragment_floor_at_every_stage():
    rng = np.random.default_rng(77)
    for _ in range(300):
        s, e, ids, tids, n_templates, lengths = random_call(rng)
        M = int(rng.integers(1, 9))
        stages = None if rng.random() < 0.5 else sorted(set(rng.integers(1, M + 1, size=2).tolist()) | {M})
        _, _, _, sets = fm.staged(s, e, ids, tids, n_templates, lengths, M, stages)
        full = fm.fragment_depth(s, e, ids, tids, lengths)
        for T, S in zip(tm.default_stages(M) if stages is None else stages, sets):
            assert tm.whole_templates(S, tids, n_templates)
            have = fm.fragment_depth(s, e, ids, tids, lengths, S)
            assert all((h >= np.minimum(f, T)).all() for h, f in zip(have, full)), (M, stages, T)


def test_contrast_input_per_segment_model_is_short_the_fragment_model_is_not():
    s, e, ids, tids, n_templates, lengths, M = fm.contrast_pairs()
    n = s.size
    full = fm.fragment_depth(s, e, ids, tids, lengths)[0]
    per_segment = pm.unpack(tm.staged(s, e, ids, tids, n_templates, lengths, M)[0], n)
    fragments = pm.unpack(fm.staged(s, e, ids, tids, n_templates, lengths, M)[0], n)
    short = int((fm.fragment_depth(s, e, ids, tids, lengths, per_segment)[0] < np.minimum(full, M)).sum())
    short_f = int((fm.fragment_depth(s, e, ids, tids, lengths, fragments)[0] < np.minimum(full, M)).sum())
    print(f"short positions: per segment {short}, fragments {short_f}; kept {int(per_segment.sum())} / {int(fragments.sum())}")
    assert short > 0 and short_f == 0


# ------------------------------------------------------------------------------------------ the plan
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fragment_plan") / "fragment_plan_driver"
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "fragment_plan_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def bytes_in_use(v):
    return (int(v).bit_length() + 7) // 8


def test_plan_sorts_only_the_digits_in_use(driver):
    values = [1, 2, 255, 256, 257, 65535, 65536, 65537, 2**24 - 1, 2**24, 2**24 + 1, 2**31, 2**32 - 1]
    cases = [(nt, nc, L) for nt in values for nc in [v for v in values if v <= 2**24] for L in values]
    out = subprocess.run([driver], input="\n".join(f"{a} {b} {c}" for a, b, c in cases) + "\n", capture_output=True,
                         text=True, check=True)
    rows = [dict(kv.split("=", 1) for kv in row.split()) for row in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    two_rounds = 0
    for (nt, nc, L), row in zip(cases, rows):
        tb_, cb, sb = bytes_in_use(nt - 1), bytes_in_use(nc - 1), bytes_in_use(L - 1)
        assert cb <= 3 and int(row["key_bytes"]) == tb_ + cb + sb
        if tb_ + cb + sb <= 8:
            assert row["rounds"] == "1" and row["r0"] == f"{max(tb_ + cb + sb, 1)},{sb},{cb},{tb_}"
            assert int(row["passes"]) == max(tb_ + cb + sb, 1)
        else:
            two_rounds += 1
            assert row["rounds"] == "2" and row["r0"] == f"{sb + cb},{sb},{cb},0" and row["r1"] == f"{tb_},0,0,{tb_}"
            assert int(row["passes"]) == tb_ + cb + sb and sb + cb <= 8
    assert two_rounds > 0
    # one contig of one position and one template: still one pass, which leaves the index column
    assert rows[cases.index((1, 1, 1))]["passes"] == "1"


# ------------------------------------------------------------------------------------------ the interface
def test_entries_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
    assert "#define QMCP_HIP_ABI_VERSION 5" in text and pkg.abi_version() == 5
    for method in ("clip_templates", "clip_templates_device", "solve_fragments", "solve_fragments_device"):
        assert hasattr(pkg.Solver, method)


def test_header_states_the_definition_the_identities_and_what_is_not_claimed():
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    start = text.index("/* Fragment depth:")
    comment = text[start:text.index("typedef struct qmcp_hip_fragment_stats", start)]
    for word in ("reach + 1", "becomes unplaced", "INPUT order", "idempotent", "Identities", "Not claimed",
                 "BEFORE anything is", "Ends never change", "pairwise", "qmcp_hip_solve_templates_* on clip(rows)"):
        assert word in " ".join(comment.replace("\n *", " ").split()), word
    # the templates entry keeps its words
    for word in ("counted per segment", "Not claimed"):
        assert word in text[text.index("/* Template-aware downsampling:"):start]


def test_fragment_stats_layout_matches_the_header(pkg, tmp_path):
    fields = ["n_placed", "n_clipped", "n_emptied", "bases_in", "bases_removed", "n_templates_overlapping", "max_group",
              "ms_clip"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ '
           'printf("%zu", sizeof(qmcp_hip_fragment_stats)); '
           + "".join(f'printf(" %zu", offsetof(qmcp_hip_fragment_stats, {f})); ' for f in fields) + 'return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", str(exe)],
                         input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    F = pkg.FragmentStats
    assert got == [C.sizeof(F)] + [getattr(F, f).offset for f in fields]
    assert [name for name, _ in F._fields_] == fields and set(F().as_dict()) == set(fields)


def test_argument_errors_come_back_before_a_context_is_needed(pkg):
    """a NULL context: the template entry's checks in its order for the solve, template_ids and n_templates for the clip;
    nothing is written"""
    s = np.arange(10, dtype=np.uint32)
    e = s + 5
    z = np.zeros(10, np.uint32)
    lengths = np.array([100], np.uint32)
    mask = np.full(2, 0xFFFFFFFFFFFFFFFF, np.uint64)
    out_s, out_c = np.full(10, 0xDEADBEEF, np.uint32), np.full(10, 0xDEADBEEF, np.uint32)
    u32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))

    def solve(entry, tids, n, n_templates, M, stages):
        tg = None if stages is None else np.asarray(stages, np.uint32)
        head = [None, u32(s), u32(e), u32(z), u32(tids), n, n_templates, u32(lengths), 1, M, u32(tg),
                0 if tg is None else tg.size]
        if entry == "host":
            rc = pkg._hip.qmcp_hip_solve_fragments_host(*head, mask.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, None)
        else:
            rc = pkg._hip.qmcp_hip_solve_fragments_device(*head, None, None, None, None, None)
        return rc, pkg._hip.qmcp_hip_last_error().decode()

    def clip(entry, tids, n, n_templates):
        head = [None, u32(s), u32(e), u32(z), u32(tids), n, n_templates, u32(lengths), 1, u32(out_s), u32(out_c)]
        if entry == "host":
            rc = pkg._hip.qmcp_hip_clip_templates_host(*head, None)
        else:
            rc = pkg._hip.qmcp_hip_clip_templates_device(*head, None, None)
        return rc, pkg._hip.qmcp_hip_last_error().decode()

    solve_cases = [
        (z, 10, 5, 5, [3, 2, 5], QMCP_EINVAL, "stages[1]"),
        (z, 10, 5, 5, [2, 4], QMCP_EINVAL, "max_coverage"),
        (z, 10, 5, 17, list(range(1, 18)), QMCP_EINVAL, "n_stages 17"),
        (z, 10, 5, 2**31, None, QMCP_ERANGE, "2^31"),
        (z, 10, 5, 0, None, QMCP_EINVAL, "max_coverage"),
        (None, 10, 5, 0, None, QMCP_EINVAL, "max_coverage"),              # the stage list before the ids
        (None, 10, 5, 5, None, QMCP_EINVAL, "template_ids"),
        (None, 10, 0, 5, None, QMCP_EINVAL, "template_ids"),              # the ids before n_templates
        (z, 10, 0, 5, None, QMCP_EINVAL, "n_templates"),
        (z, 9, 5, 5, None, QMCP_EINVAL, "null context"),
        (None, 0, 0, 5, None, QMCP_EINVAL, "null context"),
    ]
    clip_cases = [
        (None, 10, 5, QMCP_EINVAL, "template_ids"),
        (z, 10, 0, QMCP_EINVAL, "n_templates"),
        (z, 10, 5, QMCP_EINVAL, "null context"),
        (None, 0, 0, QMCP_EINVAL, "null context"),
    ]
    for entry in ("host", "device"):
        for tids, n, n_templates, M, stages, code, word in solve_cases:
            rc, msg = solve(entry, tids, n, n_templates, M, stages)
            assert rc == code and word in msg, (entry, n, n_templates, M, stages, rc, msg)
        for tids, n, n_templates, code, word in clip_cases:
            rc, msg = clip(entry, tids, n, n_templates)
            assert rc == code and word in msg, (entry, n, n_templates, rc, msg)
    assert (mask == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    assert (out_s == 0xDEADBEEF).all() and (out_c == 0xDEADBEEF).all()


# ------------------------------------------------------------------------------------------ the request and the file flow
def test_request_mirror_has_the_new_fields_beside_the_template_fields_and_keeps_its_tail(pkg, tmp_path):
    names = [name for name, _ in pkg.DownsampleRequest._fields_]
    assert names.index("fragment_report") == names.index("template_stages") + 1
    assert names.index("fragment_depth") == names.index("include_secondary") + 1
    assert names[-5:] == ["proportional_report", "proportion_num", "proportion_den", "proportion_floor", "has_proportion"]
    probe = ["template_stages", "fragment_report", "include_secondary", "fragment_depth", "ceiling", "proportional_report",
             "has_proportion"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_host_request.h"\nint main(void){ '
           'printf("%zu", sizeof(qmcp_host_downsample_request)); '
           + "".join(f'printf(" %zu", offsetof(qmcp_host_downsample_request, {f})); ' for f in probe) + 'return 0; }\n')
    exe = tmp_path / "request"
    out = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-I",
                          os.path.join(ROOT, "genome-downsampler_amd", "host", "include"), "-x", "c", "-", "-o", str(exe)],
                         input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R = pkg.DownsampleRequest
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f in probe]


def small_bam(tmp_path):
    refs = [("chrA", 4000)]
    path = tmp_path / "in.bam"
    bam_py.write_bam(path, refs, tb.single_end_records(np.random.default_rng(1), refs, 50))
    return path


def test_downsample_bam_refuses_fragment_options_without_template_aware(pkg, tmp_path):
    path = small_bam(tmp_path)
    bed = tmp_path / "t.bed"
    bed.write_text("chrA\t10\t500\n")
    go = lambda **kw: pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", 4, **kw)
    for kw in (dict(fragment_depth=True), dict(fragment_report=tmp_path / "f.tsv"),
               dict(fragment_depth=True, per_reference=True), dict(fragment_depth=True, pair_aware=True, per_reference=True),
               dict(fragment_depth=True, fragment_report=tmp_path / "f.tsv", per_reference=True)):
        with pytest.raises(ValueError, match="need template_aware=True"):
            go(**kw)
    with pytest.raises(ValueError, match="fragment_report needs fragment_depth=True"):
        go(per_reference=True, template_aware=True, fragment_report=tmp_path / "f.tsv")
    # with template_aware the mode's own refusals come as before
    both = dict(per_reference=True, template_aware=True, fragment_depth=True)
    for kw in (dict(pair_aware=True), dict(targets=bed), dict(dedup=True), dict(template_stages=[]),
               dict(template_targets=bed, template_profile=bed)):
        with pytest.raises(ValueError):
            go(**both, **kw)
    with pytest.raises(ValueError, match="per_reference"):
        go(template_aware=True, fragment_depth=True)
    assert not (tmp_path / "no.bam").exists() and not (tmp_path / "f.tsv").exists()


def test_bam_api_config_refuses_fragment_depth_without_template_aware(pkg, tmp_path):
    """straight through the request, past downsample_bam's own checks: BamApiConfig's rule, std::invalid_argument"""
    path = small_bam(tmp_path)
    err = C.create_string_buffer(1024)
    for fields in (dict(fragment_depth=1), dict(fragment_depth=1, per_reference=1)):
        request = pkg._downsample_request(solver_name="quasi-mcp-hip", in_path=path, out_path=tmp_path / "no.bam",
                                          max_coverage=4, **fields)
        rc = pkg._host.qmcp_host_downsample_bam(C.byref(request), None, 0, None, None, None, None, None, err, 1024)
        assert rc == -4 and err.value.decode() == "fragment_depth needs template_aware"
    request = pkg._downsample_request(solver_name="quasi-mcp-hip", in_path=path, out_path=tmp_path / "no.bam", max_coverage=4,
                                      per_reference=1, template_aware=1, fragment_report=tmp_path / "f.tsv")
    rc = pkg._host.qmcp_host_downsample_bam(C.byref(request), None, 0, None, None, None, None, None, err, 1024)
    assert rc == -4 and err.value.decode() == "a fragment report needs fragment_depth"
    assert not (tmp_path / "no.bam").exists()
