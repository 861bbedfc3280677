"""Template-aware downsampling under a cap table without a GPU: tests/template_profile_model.py against
tests/template_model.py and tests/profile_model.py (the four identities), every stage valid and whole templates on 300
random calls, the paired fixture under wide targets with its counts pinned, targets_as_regions against a brute-force
restatement, the symbols, the struct's layout against the header, the host-side argument errors on a NULL context, and
downsample_bam's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bam_py
import pair_model
import profile_model as pm
import template_bams as tb
import template_model as tm
import template_profile_model as tpm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QMCP_OK, QMCP_EINVAL, QMCP_ERANGE = 0, -1, -3
NO_CONTIG = 0xFFFFFFFF


def random_stages(rng, M):
    kind = int(rng.integers(0, 4))
    if kind == 0 or M == 1:
        return None
    if kind == 1:
        return [M]
    if kind == 2:
        return [1, M]
    k = int(rng.integers(1, min(M, 5) + 1))
    return sorted(rng.choice(np.arange(1, M), size=k - 1, replace=False).tolist()) + [M]


def random_call(rng, n_contigs, max_per_contig=150):
    """segments of spans 1 .. 120 on contigs of 150 .. 1 500 positions (some without a segment), a few unplaced,
    shuffled; templates of 1 .. 6 and sometimes a large one"""
    lengths = rng.integers(150, 1500, size=n_contigs).astype(np.uint32)
    counts = rng.integers(0, max_per_contig + 1, size=n_contigs)
    counts[rng.random(n_contigs) < 0.15] = 0
    ids = np.repeat(np.arange(n_contigs), counts)
    span = rng.integers(1, 121, size=ids.size)
    s = (rng.random(ids.size) * (lengths[ids].astype(np.int64) - span + 1)).astype(np.int64)
    e = s + span - 1
    ids = ids.astype(np.uint32)
    ids[rng.random(ids.size) < 0.04] = NO_CONTIG
    perm = rng.permutation(ids.size)
    n = ids.size
    tids, n_templates = tm.random_templates(rng, n, n_templates=None if rng.random() < 0.5 else n + 40,
                                            large=int(rng.integers(0, 60)))
    return s[perm].astype(np.uint32), e[perm].astype(np.uint32), ids[perm], tids, n_templates, lengths


# ------------------------------------------------------------------------------------------ the model
def test_every_stage_holds_whole_templates_and_covers_its_stage_cap_on_300_random_calls():
    rng = np.random.default_rng(2026)
    staged_calls = zero_runs = above = 0
    for call in range(300):
        s, e, ids, tids, n_templates, lengths = random_call(rng, int(rng.integers(1, 4)))
        n = s.size
        M = int(rng.choice([1, 2, 3, 7, 20]))
        default_cap = (0, M, 2 * M)[call % 3]
        table = pm.random_regions(rng, lengths, 2 * M, zero_run=int(rng.integers(0, 40)))
        stages = random_stages(rng, M)
        mask, selected, kept, sets = tpm.staged(s, e, ids, tids, n_templates, lengths, M, default_cap, *table, stages=stages)
        targets = tpm.default_stages(M) if stages is None else stages
        assert len(sets) == len(targets) == len(selected) == len(kept)
        caps = pm.cap_arrays(lengths, default_cap, *table)
        before = np.zeros(n, bool)
        for T, S, n_sel, n_kept in zip(targets, sets, selected, kept):
            stage_caps = [tpm.stage_cap(c, T, M) for c in caps]
            assert all((sc <= c).all() and ((sc == 0) == (c == 0)).all() for sc, c in zip(stage_caps, caps))
            assert tpm.covers(s, e, ids, stage_caps, S), (M, default_cap, stages, T)
            assert tm.whole_templates(S, tids, n_templates)
            assert not (before & ~S).any() and int(S.sum()) == n_kept >= int(before.sum()) + n_sel
            before = S
        assert all(np.array_equal(tpm.stage_cap(c, M, M), c) for c in caps)           # c_k = cap
        assert np.array_equal(pm.unpack(mask, n), sets[-1])
        # a segment that lies wholly on cap-0 positions enters only through its template
        hit = np.zeros(n, bool)
        for c, cap in enumerate(caps):
            pos = np.concatenate([[0], np.cumsum(cap > 0)])
            sel = np.flatnonzero(ids == c)
            hit[sel] = pos[e[sel].astype(np.int64) + 1] > pos[s[sel]]
        if n:
            reached = np.bincount(tids[sets[-1] & hit], minlength=n_templates) > 0
            assert np.array_equal(sets[-1][~hit], reached[tids[~hit]])
        assert tpm.on_cap(s, e, ids, tids, caps)[0] == int(hit.sum())
        staged_calls += len(targets) > 1
        zero_runs += any((c == 0).any() for c in caps)
        above += any((c > M).any() for c in caps)
    assert staged_calls > 150 and zero_runs > 150 and above > 150


def test_identity_1_no_region_and_default_cap_m_is_the_template_model():
    rng = np.random.default_rng(1)
    for _ in range(40):
        s, e, ids, tids, n_templates, lengths = random_call(rng, int(rng.integers(1, 4)))
        M = int(rng.choice([1, 2, 3, 7, 20]))
        stages = random_stages(rng, M)
        want = tm.staged(s, e, ids, tids, n_templates, lengths, M, stages)
        got = tpm.staged(s, e, ids, tids, n_templates, lengths, M, M, stages=stages)
        assert np.array_equal(got[0], want[0]) and got[1:3] == want[1:3]
        assert all(np.array_equal(a, b) for a, b in zip(got[3], want[3]))


def test_identity_2_distinct_ids_and_one_stage_are_the_profile_selection():
    rng = np.random.default_rng(2)
    for call in range(40):
        s, e, ids, _, _, lengths = random_call(rng, int(rng.integers(1, 4)))
        M = int(rng.choice([1, 2, 3, 7, 20]))
        default_cap = (0, M, 2 * M)[call % 3]
        table = pm.random_regions(rng, lengths, 2 * M, zero_run=20)
        tids = rng.permutation(s.size)
        mask, selected, kept, _ = tpm.staged(s, e, ids, tids, s.size, lengths, M, default_cap, *table, stages=[M])
        assert np.array_equal(mask, pm.expected_mask(s, e, ids, lengths, default_cap, *table)) and selected == kept


def test_identity_3_caps_all_m_with_regions_are_the_template_model():
    rng = np.random.default_rng(3)
    for _ in range(40):
        s, e, ids, tids, n_templates, lengths = random_call(rng, int(rng.integers(1, 4)))
        M = int(rng.choice([1, 2, 3, 7, 20]))
        stages = random_stages(rng, M)
        offs, r0, r1, _ = pm.random_regions(rng, lengths, 5)
        got = tpm.staged(s, e, ids, tids, n_templates, lengths, M, M, offs, r0, r1, np.full(r0.size, M), stages=stages)
        want = tm.staged(s, e, ids, tids, n_templates, lengths, M, stages)
        assert np.array_equal(got[0], want[0]) and got[1:3] == want[1:3]


def test_identity_4_one_stage_is_the_profile_selection_and_the_completion():
    rng = np.random.default_rng(4)
    for call in range(40):
        s, e, ids, tids, n_templates, lengths = random_call(rng, int(rng.integers(1, 4)))
        M = int(rng.choice([1, 2, 3, 7, 20]))
        default_cap = (0, M, 2 * M)[call % 3]
        table = pm.random_regions(rng, lengths, 2 * M, zero_run=20)
        plain = pm.unpack(pm.expected_mask(s, e, ids, lengths, default_cap, *table), s.size)
        mask, selected, kept, sets = tpm.staged(s, e, ids, tids, n_templates, lengths, M, default_cap, *table, stages=[M])
        assert np.array_equal(sets[0], tm.complete(plain, tids, n_templates)) and selected == [int(plain.sum())]


def test_select_equals_fast_select_on_the_staged_result():
    rng = np.random.default_rng(5)
    for call in range(60):
        s, e, ids, tids, n_templates, lengths = random_call(rng, int(rng.integers(1, 3)), max_per_contig=80)
        M = int(rng.choice([1, 2, 3, 7]))
        default_cap = (0, M, 2 * M)[call % 3]
        table = pm.random_regions(rng, lengths, 2 * M, zero_run=10)
        stages = random_stages(rng, M)
        slow = tpm.staged(s, e, ids, tids, n_templates, lengths, M, default_cap, *table, stages=stages, fast=False)
        fast = tpm.staged(s, e, ids, tids, n_templates, lengths, M, default_cap, *table, stages=stages, fast=True)
        assert np.array_equal(slow[0], fast[0]) and slow[1:3] == fast[1:3]


def mean_depth_on_target(s, e, kept, caps):
    on = caps[0] > 0
    return float(pm.coverage(s[kept].astype(np.int64), e[kept].astype(np.int64), caps[0].size)[on].mean())


PAIRED_FIXTURE = {  # (depth, stages) -> (segments kept, mean kept depth on target x 1000), computed by this model
    (3, "one"): (3732, 31857), (3, "default"): (2918, 24664),
    (8, "one"): (4128, 35086), (8, "default"): (2872, 24279),
}


@pytest.mark.parametrize("depth", [3, 8])
def test_paired_fixture_under_wide_targets_has_its_counts(depth):
    """one contig of 20 000 positions, 150-base mates 100 .. 499 apart, M = 20, cap M inside 1 500-base regions every
    2 000 and 0 elsewhere, `depth` x M deep.  One stage is solve + template completion; the default schedule {10, 20}
    credits the mates.  The counts are the model's, pinned as computed on the CPU: observations, not claims"""
    M = 20
    s, e, ids, tids, n_templates, lengths, *table = tpm.paired_targets(7, 20_000, M, depth, 1500, 2000)
    caps = pm.cap_arrays(lengths, 0, *table)
    got = {}
    for name, stages in (("one", [M]), ("default", None)):
        mask, selected, kept, sets = tpm.staged(s, e, ids, tids, n_templates, lengths, M, 0, *table, stages=stages)
        assert tpm.covers(s, e, ids, caps, sets[-1]) and tm.whole_templates(sets[-1], tids, n_templates)
        got[name] = (kept[-1], int(round(1000 * mean_depth_on_target(s, e, sets[-1], caps))))
        assert got[name] == PAIRED_FIXTURE[(depth, name)], (depth, name, got[name])
    assert got["default"][0] < got["one"][0] and M * 1000 <= got["default"][1] < got["one"][1]


# ------------------------------------------------------------------------------------------ targets_as_regions
def test_targets_as_regions_equals_the_brute_force_restatement(pkg):
    rng = np.random.default_rng(6)
    for _ in range(200):
        n_contigs = int(rng.integers(1, 4))
        lengths = rng.integers(0, 400, size=n_contigs).astype(np.uint32)
        lengths[rng.random(n_contigs) < 0.1] = 0
        counts = rng.integers(0, 8, size=n_contigs)
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        t0 = rng.integers(0, 450, size=int(offs[-1]))
        t1 = t0 + rng.integers(0, 60, size=t0.size)
        padding, cap = int(rng.choice([0, 1, 7, 500])), int(rng.integers(0, 50))
        got = pkg.targets_as_regions(offs, t0, t1, lengths, padding, cap)
        want = tpm.targets_as_regions(offs, t0, t1, lengths, padding, cap)
        for a, b in zip(got, want):
            assert a.dtype == np.uint32 and np.array_equal(a, b), (lengths, offs, t0, t1, padding, got, want)
        # disjoint, ascending and separated by at least one position inside every contig
        for c in range(n_contigs):
            a, b = got[1][got[0][c]:got[0][c + 1]].astype(np.int64), got[2][got[0][c]:got[0][c + 1]].astype(np.int64)
            assert (a <= b).all() and (a[1:] > b[:-1] + 1).all() and (b < int(lengths[c])).all()
    for bad in (dict(target_offsets=[1, 2]), dict(target_starts=[9], target_ends=[3]), dict(cap=2**31), dict(padding=-1)):
        args = dict(target_offsets=[0, 1], target_starts=[3], target_ends=[9], contig_lengths=[50], padding=0, cap=4)
        with pytest.raises(ValueError):
            pkg.targets_as_regions(**{**args, **bad})


# ------------------------------------------------------------------------------------------ the host table
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cap_prefix") / "cap_prefix_driver"
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "cap_prefix_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def test_scale_cap_and_the_prefix_counts_of_positive_positions(driver):
    """cap_table.h: scale_cap is ceil(cap * T / M) in 64 bits; cap_positive_before gives every kept region the positions
    of its contig below its start whose cap is positive -- against the cap arrays of the model"""
    rng = np.random.default_rng(8)
    triples = [(2**31 - 1, 2**31 - 2, 2**31 - 1), (2**31 - 1, 1, 4), (0, 3, 7), (1, 1, 2**31 - 1), (7, 3, 4), (5, 5, 5)]
    triples += [(int(c), int(T), int(M)) for c, T, M in zip(rng.integers(0, 2**31, 50), rng.integers(1, 40, 50), [40] * 50)]
    text = "".join(f"scale {c} {T} {M}\n" for c, T, M in triples)
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out[1::2]] == [-((-c * T) // M) for c, T, M in triples]
    assert [int(tpm.stage_cap(c, T, M)) for c, T, M in triples] == [-((-c * T) // M) for c, T, M in triples]
    for call in range(100):
        lengths = rng.integers(0, 3000, size=int(rng.integers(1, 5)))
        lengths[rng.random(lengths.size) < 0.1] = 0
        offs, r0, r1, caps = pm.random_regions(rng, lengths, 3, zero_run=int(rng.integers(0, 50)))
        default_cap = int(rng.integers(0, 2)) * 5
        tok = ["prefix", lengths.size, r0.size, default_cap, *lengths, *offs, *r0, *r1, *caps]
        rows = subprocess.run([driver], input=" ".join(str(x) for x in tok) + "\n", capture_output=True, text=True,
                              check=True).stdout.splitlines()
        assert rows[0] == "rc 0"
        for c, cap in enumerate(pm.cap_arrays(lengths, default_cap, offs, r0, r1, caps)):
            below = np.concatenate([[0], np.cumsum(cap > 0)])
            f = [int(x) for x in rows[1 + c].split(":")[1].split()]
            kept = pm.clipped_regions(int(lengths[c]), r0[offs[c]:offs[c + 1]], r1[offs[c]:offs[c + 1]], caps[offs[c]:offs[c + 1]])
            assert f[0::2] == [a for a, _, _ in kept] and f[1::2] == [int(below[a]) for a, _, _ in kept]


# ------------------------------------------------------------------------------------------ the interface
def test_entries_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_templates_profile_host", "qmcp_hip_solve_templates_profile_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
    assert "#define QMCP_HIP_ABI_VERSION 5" in text and pkg.abi_version() == 5
    assert hasattr(pkg.Solver, "solve_templates_profile") and hasattr(pkg.Solver, "solve_templates_profile_device")
    for word in ("c_j(p) = ceil(cap(p) * T_j / M)", "Identities: (1)", "Not claimed"):
        assert word in text
    nm_host = subprocess.run(["nm", "-D", "--defined-only", pkg.HOST_LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T qmcp_host_downsample_bam\b", nm_host)


def test_template_profile_stats_layout_matches_the_header(pkg, tmp_path):
    fields = ["positions_in_regions", "n_segments_on_cap", "n_templates_on_cap", "regions_in", "regions_used", "ms_need"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ '
           'printf("%zu", sizeof(qmcp_hip_template_profile_stats)); '
           + "".join(f'printf(" %zu", offsetof(qmcp_hip_template_profile_stats, {f})); ' for f in fields)
           + 'return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", str(exe)],
                         input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = pkg.TemplateProfileStats
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    assert set(T().as_dict()) == set(fields)


def test_argument_errors_come_back_before_a_context_is_needed(pkg):
    """a NULL context: the stage list, template_ids and n_templates, then the table, default_cap and flags are all
    checked on the host; only then is the context asked for"""
    s = np.arange(10, dtype=np.uint32)
    e = s + 5
    z = np.zeros(10, np.uint32)
    lengths = np.array([100, 50], np.uint32)
    mask = np.full(2, 0xFFFFFFFFFFFFFFFF, np.uint64)
    u32 = lambda a: None if a is None else np.asarray(a, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    good = dict(tids=z, n=10, n_templates=5, M=5, stages=None, lengths=lengths, offs=[0, 2, 2], r0=[10, 30], r1=[20, 40],
                caps=[1, 2], default_cap=3, flags=0)

    def call(entry, **kw):
        a = {**good, **kw}
        arrays = {k: u32(a[k]) for k in ("stages", "offs", "r0", "r1", "caps", "lengths")}      # kept alive for the call
        tg = arrays["stages"]
        head = [None, p(s), p(e), p(z), p(a["tids"]), a["n"], a["n_templates"], p(arrays["lengths"]),
                0 if arrays["lengths"] is None else arrays["lengths"].size, p(arrays["offs"]),
                p(arrays["r0"]), p(arrays["r1"]), p(arrays["caps"]), a["default_cap"], a["flags"], a["M"], p(tg),
                0 if tg is None else tg.size]
        if entry == "host":
            rc = pkg._hip.qmcp_hip_solve_templates_profile_host(*head, mask.ctypes.data_as(C.POINTER(C.c_uint64)), None,
                                                                None, None)
        else:
            rc = pkg._hip.qmcp_hip_solve_templates_profile_device(*head, None, None, None, None, None)
        return rc, pkg._hip.qmcp_hip_last_error().decode()

    cases = [
        (dict(stages=[3, 2, 5]), QMCP_EINVAL, "stages[1]"),
        (dict(stages=[2, 4]), QMCP_EINVAL, "max_coverage"),
        (dict(M=17, stages=list(range(1, 18))), QMCP_EINVAL, "n_stages 17"),
        (dict(M=2**31, stages=[2**31]), QMCP_ERANGE, "2^31"),
        (dict(M=2**31 - 1, stages=[5, 2**31, 2**31 - 1]), QMCP_ERANGE, "stages[1]"),
        (dict(M=0), QMCP_EINVAL, "max_coverage"),
        (dict(stages=[0, 5]), QMCP_EINVAL, "stages[0]"),
        (dict(tids=None), QMCP_EINVAL, "template_ids"),
        (dict(n_templates=0), QMCP_EINVAL, "n_templates"),
        (dict(lengths=None), QMCP_EINVAL, "contig_lengths"),
        (dict(flags=2), QMCP_EINVAL, "flag"),
        (dict(offs=[1, 2, 2]), QMCP_EINVAL, "region table"),
        (dict(offs=[0, 2, 1]), QMCP_EINVAL, "region table"),
        (dict(r0=[10, 15]), QMCP_EINVAL, "region table"),                 # overlap
        (dict(r0=[25, 30]), QMCP_EINVAL, "region table"),                 # start > end
        (dict(r0=None), QMCP_EINVAL, "region table"),
        (dict(caps=[1, 2**31]), QMCP_ERANGE, "cap"),
        (dict(default_cap=2**31), QMCP_ERANGE, "default_cap"),
        (dict(), QMCP_EINVAL, "null context"),                            # a good call: the context is asked for next
        (dict(default_cap=0, offs=None, r0=None, r1=None, caps=None), QMCP_EINVAL, "null context"),
        (dict(tids=None, n=0, n_templates=0), QMCP_EINVAL, "null context"),
    ]
    for entry in ("host", "device"):
        for kw, code, word in cases:
            rc, msg = call(entry, **kw)
            assert rc == code and word in msg, (entry, kw, rc, msg)
        rc, msg = call(entry, r0=[10, 30], r1=[120, 140], offs=[0, 1, 2])                  # clipped, one per contig: fine
        assert rc == QMCP_EINVAL and "null context" in msg
    assert (mask == np.uint64(0xFFFFFFFFFFFFFFFF)).all()


# ------------------------------------------------------------------------------------------ downsample_bam
def test_the_new_keywords_refuse_what_they_do_not_go_together_with(pkg, tmp_path):
    refs = [("chrA", 4000)]
    path = tmp_path / "in.bam"
    bam_py.write_bam(path, refs, tb.single_end_records(np.random.default_rng(1), refs, 50))
    bed = tmp_path / "t.bed"
    bed.write_text("chrA\t10\t500\n")
    graph = tmp_path / "caps.bedgraph"
    graph.write_text("chrA\t10\t500\t3\n")
    other = tmp_path / "other.bed"
    other.write_text("chrZ\t10\t500\n")
    go = lambda **kw: pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", 4, **kw)
    both = dict(per_reference=True, template_aware=True)
    refused = [
        dict(template_targets=bed), dict(template_profile=graph),                           # no template_aware
        dict(template_targets=bed, template_aware=True), dict(template_profile=graph, template_aware=True),   # no per_reference
        dict(template_targets=bed, per_reference=True), dict(template_profile=graph, per_reference=True),
        dict(template_targets=bed, per_reference=True, pair_aware=True),
        dict(both, template_targets=bed, template_profile=graph),                           # both tables
        dict(both, template_target_padding=5), dict(both, template_profile=graph, template_target_padding=5),
        dict(both, template_targets=bed, template_target_padding=-1),
        dict(both, template_targets=bed, targets=bed), dict(both, template_profile=graph, profile=graph),
        dict(both, template_targets=bed, pair_aware=True), dict(both, template_targets=bed, dedup=True),
        dict(both, template_profile=graph, stratify="strand"), dict(both, template_profile=graph, report=tmp_path / "r.tsv"),
        dict(both, template_targets=bed, track=tmp_path / "t.bedgraph"),
        dict(both, template_targets=bed, ladder=[3], ladder_out=tmp_path / "l{M}.bam"),
        dict(both, template_targets=bed, bed=bed, amplicons_by_reference=True),
        dict(both, template_targets=bed, template_stages=[]),
        dict(both, template_targets=other), dict(both, template_profile=other),             # a chrom of no reference; no cap column
    ]
    for kw in refused:
        with pytest.raises(ValueError):
            go(**kw)
    with pytest.raises(ValueError):
        pkg.downsample_bam("quasi-mcp-hip-quality", path, tmp_path / "no.bam", 4, **both, template_targets=bed)
    assert not (tmp_path / "no.bam").exists()
