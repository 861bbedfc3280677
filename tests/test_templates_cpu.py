"""Template-aware downsampling, the parts that need no GPU: the model (tests/template_model.py) against
tests/pair_model.py for ids i // 2, whole templates that are valid at every stage; the two entries declared, listed and
exported, the stats' layout against the header, host-side argument errors before a context is looked at; and the
template-aware ingest (read_bam(templates=True)) against the independent parse in tests/template_bams.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bam_py
import multi_reference as mr
import pair_model as pairs
import profile_model as pm
import template_bams as tb
import template_model as tm

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


# ------------------------------------------------------------------------------------------ the model
def test_ids_i_div_2_give_the_pair_model(oracle):
    rng = np.random.default_rng(7)
    for _ in range(40):
        s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(1, 4)), max_reads_per_contig=int(rng.integers(1, 200)))
        n = s.size - (s.size & 1)
        s, e, ids = s[:n], e[:n], ids[:n]
        M = int(rng.choice([1, 2, 3, 7, 20]))
        stages = random_stages(rng, M)
        tids = np.arange(n) // 2
        want = pairs.staged(oracle, s, e, ids, lengths, M, stages, fast=True)
        got = tm.staged(s, e, ids, tids, n // 2, lengths, M, stages)
        assert np.array_equal(got[0], want[0]) and got[1:3] == want[1:3]
        assert all(np.array_equal(a, b) for a, b in zip(got[3], want[3]))


def test_every_stage_holds_whole_templates_and_covers_its_target_on_300_random_calls():
    rng = np.random.default_rng(2025)
    staged_calls = 0
    for _ in range(300):
        s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(1, 4)), max_reads_per_contig=int(rng.integers(1, 120)))
        n = s.size                                                        # (odd counts included)
        M = int(rng.choice([1, 2, 3, 7, 20]))
        stages = random_stages(rng, M)
        tids, n_templates = tm.random_templates(rng, n, n_templates=None if rng.random() < 0.5 else n + 40,
                                                large=int(rng.integers(0, 60)))
        mask, selected, kept, sets = tm.staged(s, e, ids, tids, n_templates, lengths, M, stages)
        targets = tm.default_stages(M) if stages is None else stages
        assert len(sets) == len(targets) == len(selected) == len(kept)
        before = np.zeros(n, bool)
        for T, S, n_sel, n_kept in zip(targets, sets, selected, kept):
            assert tm.covers(s, e, ids, lengths, S, T), (M, stages, T)
            assert tm.whole_templates(S, tids, n_templates)
            assert not (before & ~S).any() and int(S.sum()) == n_kept >= int(before.sum()) + n_sel
            before = S
        assert np.array_equal(pm.unpack(mask, n), sets[-1])
        # an unplaced segment is kept only through a template with a kept placed segment
        if n:
            placed_kept = np.bincount(tids[sets[-1] & (ids != NO_CONTIG)], minlength=n_templates) > 0
            assert np.array_equal(sets[-1][ids == NO_CONTIG], placed_kept[tids[ids == NO_CONTIG]])
        hist, used, largest = tm.template_counts(tids, n_templates)
        assert sum(hist) == used == np.unique(tids).size and (largest == 0) == (n == 0)
        staged_calls += len(targets) > 1
    assert staged_calls > 150


def test_distinct_ids_and_one_stage_are_the_plain_selection(oracle):
    rng = np.random.default_rng(11)
    for M in (1, 3, 10):
        s, e, ids, lengths = mr.random_by_contig(rng, 3, max_reads_per_contig=300)
        tids = rng.permutation(s.size)
        mask, selected, kept, _ = tm.staged(s, e, ids, tids, s.size, lengths, M, [M])
        assert np.array_equal(mask, mr.oracle_by_contig(oracle, s, e, ids, lengths, M)) and selected == kept


# ------------------------------------------------------------------------------------------ the interface
def test_entries_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_templates_host", "qmcp_hip_solve_templates_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
    assert "#define QMCP_HIP_ABI_VERSION 5" in text and pkg.abi_version() == 5
    assert hasattr(pkg.Solver, "solve_templates") and hasattr(pkg.Solver, "solve_templates_device")
    for word in ("complete_templates(S)", "counted per segment", "Not claimed"):
        assert word in text


def test_template_stats_layout_matches_the_header(pkg, tmp_path):
    fields = ["n_stages", "n_selected", "n_kept", "capped_positions", "demand", "target", "sweeps", "ms_stage",
              "ms_templates", "max_template_size", "n_templates_used", "n_templates_kept", "size_hist"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){ '
           'printf("%zu", sizeof(qmcp_hip_template_stats)); '
           + "".join(f'printf(" %zu", offsetof(qmcp_hip_template_stats, {f})); ' for f in fields)
           + 'printf(" %zu", sizeof(((qmcp_hip_template_stats*)0)->size_hist)); return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", str(exe)],
                         input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = pkg.TemplateStats
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f in fields] + [8 * 8]
    # the per-stage part is laid out as qmcp_hip_pair_stats is
    P = pkg.PairStats
    for f in fields[:8]:
        assert getattr(T, f).offset == getattr(P, f).offset


def test_argument_errors_come_back_before_a_context_is_needed(pkg):
    """a NULL context: the stage list, template_ids and n_templates are checked first, on the host"""
    s = np.arange(10, dtype=np.uint32)
    e = s + 5
    z = np.zeros(10, np.uint32)
    lengths = np.array([100], np.uint32)
    mask = np.full(2, 0xFFFFFFFFFFFFFFFF, np.uint64)
    u32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))

    def call(entry, tids, n, n_templates, M, stages):
        tg = None if stages is None else np.asarray(stages, np.uint32)
        head = [None, u32(s), u32(e), u32(z), u32(tids), n, n_templates, u32(lengths), 1, M, u32(tg),
                0 if tg is None else tg.size]
        if entry == "host":
            rc = pkg._hip.qmcp_hip_solve_templates_host(*head, mask.ctypes.data_as(C.POINTER(C.c_uint64)), None, None)
        else:
            rc = pkg._hip.qmcp_hip_solve_templates_device(*head, None, None, None, None)
        return rc, pkg._hip.qmcp_hip_last_error().decode()

    cases = [
        (z, 10, 5, 5, [3, 2, 5], QMCP_EINVAL, "stages[1]"),
        (z, 10, 5, 5, [5, 3], QMCP_EINVAL, "stages[1]"),
        (z, 10, 5, 5, [2, 4], QMCP_EINVAL, "max_coverage"),
        (z, 10, 5, 17, list(range(1, 18)), QMCP_EINVAL, "n_stages 17"),
        (z, 10, 5, 2**31, [2**31], QMCP_ERANGE, "2^31"),
        (z, 10, 5, 2**31 - 1, [5, 2**31, 2**31 - 1], QMCP_ERANGE, "stages[1]"),
        (z, 10, 5, 2**31, None, QMCP_ERANGE, "2^31"),
        (z, 10, 5, 0, None, QMCP_EINVAL, "max_coverage"),
        (z, 10, 5, 5, [0, 5], QMCP_EINVAL, "stages[0]"),
        (None, 10, 5, 5, None, QMCP_EINVAL, "template_ids"),
        (z, 10, 0, 5, None, QMCP_EINVAL, "n_templates"),
        (z, 9, 5, 5, None, QMCP_EINVAL, "null context"),                  # an odd count is fine: the context is asked for next
        (None, 0, 0, 5, None, QMCP_EINVAL, "null context"),               # and so are no segments, no ids and no templates
    ]
    for entry in ("host", "device"):
        for tids, n, n_templates, M, stages, code, word in cases:
            rc, msg = call(entry, tids, n, n_templates, M, stages)
            assert rc == code and word in msg, (entry, n, n_templates, M, stages, rc, msg)
    assert (mask == np.uint64(0xFFFFFFFFFFFFFFFF)).all()


# ------------------------------------------------------------------------------------------ the ingest
REFS = [("chrA", 6000), ("chrB", 3000)]


def ingest(pkg, tmp_path, records, name="in.bam", **kw):
    path = tmp_path / name
    bam_py.write_bam(path, REFS, records)
    cols = pkg.read_bam(path, per_reference=True, templates=True, **kw)
    want = tb.expected_segments(records, **kw)
    for key in ("starts", "ends", "contig_ids", "template_ids", "qualities", "seq_lengths", "segment_records",
                "filtered_out"):
        assert np.array_equal(np.asarray(cols[key], np.int64), np.asarray(want[key], np.int64)), key
    assert cols["n_templates"] == want["n_templates"] and cols["contig_lengths"].tolist() == [L for _, L in REFS]
    # against bam_py's own parse: a segment lies inside its record's [pos, pos + rlen), and a record's blocks rise
    _, parsed, _ = bam_py.parse(path)
    for s, e, c, r in zip(cols["starts"], cols["ends"], cols["contig_ids"], cols["segment_records"]):
        rec = parsed[int(r)]
        if c != NO_CONTIG:
            assert rec["pos"] <= s <= e <= rec["pos"] + max(rec["rlen"], 1) - 1
    same = cols["segment_records"][1:] == cols["segment_records"][:-1]
    assert (cols["starts"][1:][same].astype(np.int64) > cols["ends"][:-1][same]).all()
    assert (np.diff(cols["segment_records"].astype(np.int64)) >= 0).all()
    return cols


def test_single_end_file_gives_one_template_per_record(pkg, tmp_path):
    records = tb.single_end_records(np.random.default_rng(1), REFS, 400)
    cols = ingest(pkg, tmp_path, records)
    assert cols["n_templates"] == 400 == cols["starts"].size and cols["filtered_out"].size == 0
    assert cols["template_ids"].tolist() == list(range(400)) and cols["segment_records"].tolist() == list(range(400))
    # the plain pairing loses every one of them
    plain = pkg.read_bam(tmp_path / "in.bam", per_reference=True)
    assert plain["starts"].size == 0 and plain["filtered_out"].size == 400


def test_paired_file_gives_templates_of_two(pkg, tmp_path):
    header, parsed, _ = mr.write_multi_reference_bam(tmp_path / "pairs.bam", np.random.default_rng(2), REFS, 300)
    cols = pkg.read_bam(tmp_path / "pairs.bam", per_reference=True, templates=True)
    assert cols["n_templates"] == 300 and cols["starts"].size == 600 and cols["filtered_out"].size == 0
    assert (np.bincount(cols["template_ids"]) == 2).all()
    names = [r["qname"] for r in parsed]
    first_seen = list(dict.fromkeys(names))
    assert [first_seen[t] for t in cols["template_ids"].tolist()] == names
    unmapped = np.array([r["ref_id"] < 0 for r in parsed])
    assert unmapped.any() and np.array_equal(cols["contig_ids"] == NO_CONTIG, unmapped)
    mapped = ~unmapped
    assert np.array_equal(cols["starts"][mapped], np.array([r["pos"] for r in parsed])[mapped])
    assert np.array_equal(cols["ends"][mapped], np.array([r["pos"] + r["rlen"] - 1 for r in parsed])[mapped])


def test_a_spliced_record_is_cut_at_its_introns(pkg, tmp_path):
    records = [tb.record("a", 0, 0, 100, 30, [(50, "M"), (1000, "N"), (50, "M")]),
               tb.record("b", 0, 1, 10, 30, [(5, "S"), (20, "M"), (3, "D"), (10, "M"), (2, "I"), (100, "N"), (7, "="), (8, "X"),
                                             (50, "N"), (30, "M")]),
               tb.record("c", 0, 0, 40, 30, [(10, "M"), (5, "N"), (6, "N"), (10, "M")]),   # two N in a row: no empty block
               tb.record("d", 0, 0, 77, 30, [(30, "S")]),                                    # consumes no reference
               tb.record("e", 0, 0, 90, 30, [(25, "N"), (10, "M")])]                         # begins with an intron
    cols = ingest(pkg, tmp_path, records)
    seg = lambda c, r: [(int(s), int(e)) for s, e, x in zip(c["starts"], c["ends"], c["segment_records"]) if x == r]
    assert seg(cols, 0) == [(100, 149), (1150, 1199)]
    assert seg(cols, 1) == [(10, 42), (143, 157), (208, 237)]
    assert seg(cols, 2) == [(40, 49), (61, 70)]
    assert seg(cols, 3) == [(77, 77)]
    assert seg(cols, 4) == [(115, 124)]
    assert cols["template_ids"].tolist() == [0, 0, 1, 1, 1, 2, 2, 3, 4]
    whole = ingest(pkg, tmp_path, records, split_spliced=False)
    assert [seg(whole, r) for r in range(5)] == [[(100, 1199)], [(10, 237)], [(40, 70)], [(77, 77)], [(90, 124)]]


def test_supplementary_secondary_and_unmapped_records(pkg, tmp_path):
    records = [tb.record("x", 0x41, 0, 100, 40, [(60, "M"), (40, "S")]),
               tb.record("y", 0, 1, 5, 40, [(70, "M")]),
               tb.record("x", 0x800 | 0x41, 1, 900, 40, [(60, "H"), (40, "M")]),           # joins x
               tb.record("y", 0x100, 0, 3000, 0, [(70, "M")]),                              # secondary of y
               tb.record("x", 0x81 | 0x4, -1, -1, 0, [], l_seq=100),                        # x's unmapped mate
               tb.record("z", 0x41, 0, 10, 40, [(50, "M")]),
               tb.record("z", 0x81 | 0x4, 0, 10, 0, [], l_seq=100)]                         # unmapped, placed with its mate
    cols = ingest(pkg, tmp_path, records)
    assert cols["template_ids"].tolist() == [0, 1, 0, 0, 2, 2] and cols["n_templates"] == 3
    assert cols["segment_records"].tolist() == [0, 1, 2, 4, 5, 6] and cols["filtered_out"].tolist() == [3]
    assert cols["contig_ids"].tolist() == [0, 1, 1, NO_CONTIG, 0, NO_CONTIG]
    taken = ingest(pkg, tmp_path, records, include_secondary=True)
    assert taken["template_ids"].tolist() == [0, 1, 0, 1, 0, 2, 2] and taken["filtered_out"].size == 0
    assert (int(taken["starts"][3]), int(taken["ends"][3]), int(taken["contig_ids"][3])) == (3000, 3069, 0)


def test_a_record_under_the_long_cigar_convention_is_decoded(pkg, tmp_path):
    real = [(40, "M"), (150, "N"), (35, "M"), (2, "D"), (25, "M")]
    records = [tb.cg_record("first", 0, 0, 700, 50, real),                                  # the field alone
               tb.cg_record("among", 0, 1, 20, 50, real, before=b"NMC\x03" + b"RGZgroup1\0" + b"ZBBs\x02\0\0\0\x01\0\x02\0",
                            after=b"XSi\xf9\xff\xff\xff"),
               tb.record("plain", 0, 0, 50, 50, [(30, "S"), (80, "N")], aux=b"NMC\x00", l_seq=30)]   # no CG field
    cols = ingest(pkg, tmp_path, records)
    seg = lambda r: [(int(s), int(e)) for s, e, x in zip(cols["starts"], cols["ends"], cols["segment_records"]) if x == r]
    assert seg(0) == [(700, 739), (890, 951)] and seg(1) == [(20, 59), (210, 271)]
    assert seg(2) == [(50, 129)]                                          # never a record without a segment
    whole = ingest(pkg, tmp_path, records, split_spliced=False)
    assert whole["starts"].tolist() == [700, 20, 50] and whole["ends"].tolist() == [951, 271, 129]


@pytest.mark.parametrize("aux", [b"CGBI" + b"\xe8\x03\0\0" + b"\0" * 8,     # a B array that claims 1 000 values
                                 b"XXZabc",                                   # a Z field without its NUL
                                 b"CG"])                                      # a field cut after its tag
def test_malformed_fields_behind_a_placeholder_cigar_are_refused(pkg, tmp_path, aux):
    records = tb.single_end_records(np.random.default_rng(4), REFS, 5)
    records.append(tb.record("bad", 0, 0, 10, 30, [(30, "S"), (80, "N")], aux=aux, l_seq=30))
    bam_py.write_bam(tmp_path / "bad.bam", REFS, records)
    with pytest.raises(OSError, match="fields past its end"):
        pkg.read_bam(tmp_path / "bad.bam", per_reference=True, templates=True)


def test_filters_drop_whole_templates(pkg, tmp_path):
    records = [tb.record("a", 0x41, 0, 100, 40, [(60, "M")]), tb.record("a", 0x81, 0, 300, 10, [(60, "M")]),
               tb.record("b", 0x41, 0, 200, 40, [(60, "M")]), tb.record("b", 0x81 | 0x4, -1, -1, 0, [], l_seq=100),
               tb.record("c", 0, 1, 100, 25, [(30, "M"), (100, "N"), (20, "M")]),
               tb.record("d", 0, 1, 400, 60, [(80, "M")]), tb.record("d", 0x800, 0, 900, 5, [(50, "H"), (30, "M")])]
    cols = ingest(pkg, tmp_path, records, min_mapq=20)
    # a: its second mate fails; b stays (the unmapped mate is exempt); c stays; d: its supplementary fails
    assert cols["segment_records"].tolist() == [2, 3, 4, 4] and cols["filtered_out"].tolist() == [0, 1, 5, 6]
    assert cols["template_ids"].tolist() == [0, 0, 1, 1] and cols["n_templates"] == 2
    cols = ingest(pkg, tmp_path, records, min_length=55)
    # c (50 bases) and d (its supplementary has 30) leave; b's unmapped mate is exempt
    assert cols["segment_records"].tolist() == [0, 1, 2, 3] and cols["n_templates"] == 2


def test_the_mixed_fixture_has_what_the_file_flow_test_is_for(pkg, tmp_path):
    refs3 = [("chrA", 5000), ("chrB", 3000), ("chrC", 800)]
    records = tb.mixed_records(np.random.default_rng(11), refs3, 700)
    path = tmp_path / "mixed.bam"
    bam_py.write_bam(path, refs3, records)
    for kw in ({}, dict(include_secondary=True), dict(split_spliced=False), dict(min_mapq=30)):
        cols = pkg.read_bam(path, per_reference=True, templates=True, **kw)
        want = tb.expected_segments(records, **kw)
        for key in ("starts", "ends", "contig_ids", "template_ids", "segment_records", "filtered_out"):
            assert np.array_equal(np.asarray(cols[key], np.int64), np.asarray(want[key], np.int64)), (kw, key)
        assert cols["n_templates"] == want["n_templates"]
    cols = pkg.read_bam(path, per_reference=True, templates=True)
    sizes = np.bincount(cols["template_ids"])
    assert sizes.max() >= 6 and (sizes == 1).any() and (sizes == 2).any() and (cols["contig_ids"] == NO_CONTIG).any()
    assert cols["filtered_out"].size > 20                                 # the secondaries


def test_templates_refuse_what_they_do_not_go_together_with(pkg, tmp_path):
    path = tmp_path / "in.bam"
    bam_py.write_bam(path, REFS, tb.single_end_records(np.random.default_rng(1), REFS, 10))
    bed = tmp_path / "a.bed"
    bed.write_text("chrA\t10\t500\n")
    for kw in (dict(per_reference=False), dict(per_reference=True, bed=bed),
               dict(per_reference=True, bed=bed, amplicons_by_reference=True), dict(per_reference=True, stratify="strand")):
        with pytest.raises(ValueError):
            pkg.read_bam(path, templates=True, **kw)
    for kw in (dict(split_spliced=False), dict(include_secondary=True)):
        with pytest.raises(ValueError):
            pkg.read_bam(path, per_reference=True, **kw)
    with pytest.raises(OSError):
        pkg.read_bam(tmp_path / "missing.bam", per_reference=True, templates=True)
