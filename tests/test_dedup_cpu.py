"""Duplicate-aware downsampling, the parts that need no GPU: the host-side plan (genome-downsampler_amd/csrc/
dedup_plan.h) compiled with g++ alone into tests/cpp/dedup_plan_driver.cpp against its restatement in
tests/dedup_model.py; the model's own properties on the oracle; the entries declared, listed and exported with the ABI
version unchanged; the combinations downsample_bam refuses."""
import os
import re
import subprocess

import numpy as np
import pytest

import dedup_model as dm
import multi_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dedup_plan") / "dedup_plan_driver"
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "dedup_plan_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def ask(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = [dict(kv.split("=", 1) for kv in row.split()) for row in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    got = []
    for r in rows:
        rounds = []
        for part in r["rounds"].split(";"):
            on, bits, passes, shifts = part.split(":")
            rounds.append((int(on), int(bits), int(passes), [] if shifts == "-" else [int(x) for x in shifts.split(",")]))
        got.append(dict(bits=[int(x) for x in r["bits"].split(",")], key_bits=int(r["key_bits"]), form=int(r["form"]),
                        passes=int(r["passes"]), rounds=rounds))
    return got


def check_plan(got, bits):
    want = dm.plan(bits)
    assert got["bits"] == bits
    assert {k: got[k] for k in ("key_bits", "form", "passes")} == {k: want[k] for k in ("key_bits", "form", "passes")}
    if want["form"] == 2:
        assert [r[:3] for r in got["rounds"]] == [r[:3] for r in want["rounds"]]
    else:
        assert got["rounds"] == want["rounds"]


def test_plan_equals_its_restatement_on_seeded_shapes(driver):
    rng = np.random.default_rng(11)
    lines, fields = [], []
    for _ in range(200):
        total = int(rng.integers(1, 1 << int(rng.integers(1, 57))))
        s0 = int(rng.integers(0, 1000))
        s1 = s0 + int(rng.integers(0, 1 << int(rng.integers(0, 33))))
        t0 = int(rng.integers(0, 1 << 16))
        t1 = min(t0 + int(rng.integers(0, 1 << int(rng.integers(0, 33)))), (1 << 32) - 1)
        q0 = int(rng.integers(0, 100))
        q1 = q0 + int(rng.integers(0, 1 << int(rng.integers(0, 17))))
        if rng.random() < 0.1:
            t0, t1, q0, q1, s0, s1 = (1 << 32) - 1, 0, (1 << 32) - 1, 0, (1 << 32) - 1, 0   # no placed read
        wq = int(rng.random() < 0.7)
        lines.append(f"r {total} {s0} {s1} {t0} {t1} {q0} {q1} {wq}")
        fields.append(dm.read_fields(total, s0, s1, t0, t1, q0, q1, bool(wq)))
        n_placed = int(rng.integers(0, 1 << int(rng.integers(1, 32))))
        lines.append(f"p {n_placed} {q0} {q1}")
        fields.append(dm.pair_fields(n_placed, q0, q1))
    forms = set()
    for got, bits in zip(ask(driver, lines), fields):
        check_plan(got, bits)
        forms.add(got["form"])
    assert forms == {0, 1, 2}


def test_plan_switches_forms_at_exactly_32_and_64_bits(driver):
    # 8 bits of quality, 12 of tag, 3 of span; gstart takes bit_length(total_length) bits and makes up the rest
    cases = []
    for key_bits in (31, 32, 33, 63, 64, 65, 66):
        cases.append((key_bits, f"r {(1 << (key_bits - 23)) - 1} 10 17 0 4095 0 255 1"))
    got = ask(driver, [c[1] for c in cases])
    for (key_bits, _), g in zip(cases, got):
        assert g["key_bits"] == key_bits and g["bits"] == [8, 12, 3, key_bits - 23]
        assert g["form"] == (0 if key_bits <= 32 else 1 if key_bits <= 64 else 2)
        check_plan(g, g["bits"])
        if key_bits <= 64:
            assert g["passes"] == (key_bits + 7) // 8 and len(g["rounds"]) == 1
            assert g["rounds"] == [(15, key_bits, (key_bits + 7) // 8, [0, 8, 20, 23])]
        else:
            # beyond 64 bits: one stable sort per field, least significant first
            assert [r[0] for r in g["rounds"]] == [1, 2, 4, 8]
            assert [r[1] for r in g["rounds"]] == g["bits"]
            assert g["passes"] == sum((b + 7) // 8 for b in g["bits"])


def test_plan_pays_for_no_field_the_call_does_not_use(driver):
    one_span_no_tags, no_quality, nothing = ask(driver, ["r 1000 99 99 0 0 3 60 1", "r 1000 99 99 0 0 3 60 0",
                                                         "r 0 4294967295 0 4294967295 0 4294967295 0 1"])
    assert one_span_no_tags["bits"] == [6, 0, 0, 10] and one_span_no_tags["rounds"] == [(9, 16, 2, [0, 6])]
    assert no_quality["bits"] == [0, 0, 0, 10] and no_quality["passes"] == 2
    assert nothing["key_bits"] == 0 and nothing["form"] == 0 and nothing["passes"] == 1   # a pass builds the index column


def tiny(rng):
    n_contigs = int(rng.integers(1, 4))
    lengths = rng.integers(20, 80, size=n_contigs).astype(np.uint32)
    n = int(rng.integers(0, 41))
    ids = rng.integers(0, n_contigs, size=n)
    span = rng.integers(1, 15, size=n)
    s = (rng.random(n) * (lengths[ids] - span + 1)).astype(np.int64)
    e = s + span - 1
    ids = np.where(rng.random(n) < 0.1, mr.NO_CONTIG, ids)
    return s.astype(np.uint32), e.astype(np.uint32), ids.astype(np.uint32), lengths


def make_unique(s, e, ids, rng):
    """tags that make every read's cell its own"""
    return rng.permutation(s.size).astype(np.uint32)


def test_model_without_duplicates_is_the_plain_selection(oracle):
    rng = np.random.default_rng(5)
    for k in range(150):
        s, e, ids, lengths = tiny(rng)
        M = int(rng.integers(1, 5))
        tags = make_unique(s, e, ids, rng)
        q = rng.integers(0, 61, size=s.size).astype(np.uint32)
        plain = dm.unpack(mr.oracle_by_contig(oracle, s, e, ids, lengths, M), s.size)
        keep, dup, st, hist = dm.dedup(oracle, s, e, ids, lengths, M, tags=tags, qualities=q, hist_bins=4)
        assert np.array_equal(keep, plain) and not dup.any()
        assert st["duplicate_units"] == 0 and st["families"] == st["units"] == (ids != mr.NO_CONTIG).sum()
        assert hist.sum() == st["families"] and hist[1:].sum() == 0
        if s.size % 2 == 0:
            # pair mode: a unit's signature holds a cell no other unit has
            keep, dup, st, hist = dm.dedup(oracle, s, e, ids, lengths, M, tags=tags, qualities=q, pairs=True, hist_bins=4)
            assert np.array_equal(keep, plain) and not dup.any() and hist.sum() == st["families"]


def test_model_keeps_exactly_the_originals_of_replicated_reads(oracle):
    rng = np.random.default_rng(6)
    for k in range(150):
        s, e, ids, lengths = tiny(rng)
        n = s.size
        M = int(rng.integers(1, 5))
        tags = make_unique(s, e, ids, rng)
        q = rng.integers(10, 61, size=n).astype(np.uint32)
        plain = dm.unpack(mr.oracle_by_contig(oracle, s, e, ids, lengths, M), n)
        copies = int(rng.integers(2, 4))
        # originals keep their relative order (the canonical selection breaks ties by index); copies go anywhere
        src = np.concatenate([np.arange(n)] + [np.arange(n)] * (copies - 1))
        original = np.concatenate([np.ones(n, bool), np.zeros(n * (copies - 1), bool)])
        qq = np.where(original, q[src], q[src] - rng.integers(1, 10, size=src.size)).astype(np.uint32)
        pos = rng.permutation(src.size)
        slot_of_original = np.sort(pos[:n])
        pos[:n] = slot_of_original
        perm = np.argsort(pos)
        src, original, qq = src[perm], original[perm], qq[perm]
        keep, dup, st, hist = dm.dedup(oracle, s[src], e[src], ids[src], lengths, M, tags=tags[src], qualities=qq, hist_bins=8)
        assert np.array_equal(src[original], np.arange(n))
        assert not keep[~original].any()
        assert np.array_equal(keep[original], plain)
        placed = ids[src] != mr.NO_CONTIG
        assert np.array_equal(dup, placed & ~original)
        assert not (keep & dup).any()
        assert hist.sum() == st["families"] and st["largest_family"] == (copies if placed.any() else 0)
        assert st["units"] == st["families"] + st["duplicate_units"]


def test_model_pair_mode_invariants(oracle):
    rng = np.random.default_rng(7)
    for k in range(100):
        s, e, ids, lengths = tiny(rng)
        n = s.size - s.size % 2
        s, e, ids = s[:n], e[:n], ids[:n]
        # heavy duplication: positions drawn from a few intervals
        pick = rng.integers(0, max(n // 4, 1), size=n)
        s, e, ids = s[pick], e[pick], ids[pick]
        q = rng.integers(0, 5, size=n).astype(np.uint32)
        for complete in (False, True):
            keep, dup, st, hist = dm.dedup(oracle, s, e, ids, lengths, 2, qualities=q, pairs=True, complete_pairs=complete,
                                           hist_bins=3)
            assert not (keep & dup).any()
            assert hist.sum() == st["families"] and st["units"] == st["families"] + st["duplicate_units"]
            assert np.array_equal(dup[0::2], dup[1::2])
            assert st["reads_survived"] == 2 * st["families"]
            if complete:
                assert np.array_equal(keep[0::2], keep[1::2])
        # swapping the mates of every other unit changes no family
        sw = np.arange(n).reshape(-1, 2)
        sw[::2] = sw[::2, ::-1]
        sw = sw.reshape(-1)
        _, dup2, st2, hist2 = dm.dedup(oracle, s[sw], e[sw], ids[sw], lengths, 2, qualities=q[sw], pairs=True, hist_bins=3)
        assert st2 == st and np.array_equal(hist2, hist) and np.array_equal(dup2, dup[sw])


def test_entries_are_declared_listed_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "qmcp_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("qmcp_hip_solve_dedup_host", "qmcp_hip_solve_dedup_device"):
        assert re.search(rf"\bint {name}\(", text)
        assert name in pkg.ABI_SYMBOLS and name in pkg.exported_symbols()
        assert re.search(rf" T {name}\b", nm)
    assert re.search(r"#define QMCP_HIP_ABI_VERSION 5\b", text) and pkg.abi_version() == 5
    assert re.search(r"#define QMCP_DEDUP_PAIRS 1u", text) and re.search(r"#define QMCP_DEDUP_COMPLETE_PAIRS 2u", text)
    assert (pkg.DEDUP_PAIRS, pkg.DEDUP_COMPLETE_PAIRS) == (1, 2)
    # the stats structure's layout: five u64, two u32, one float
    import ctypes as C
    assert C.sizeof(pkg.DedupStats) == 56
    assert [n for n, _ in pkg.DedupStats._fields_] == ["units", "families", "duplicate_units", "largest_family",
                                                      "reads_survived", "key_bits", "sort_passes", "ms_dedup"]
    m = re.search(r"typedef struct qmcp_hip_dedup_stats \{(.*?)\} qmcp_hip_dedup_stats;", text, re.S)
    declared = re.findall(r"^\s*(?:uint64_t|uint32_t|float)\s+(\w+);", m.group(1), re.M)
    assert declared == [n for n, _ in pkg.DedupStats._fields_]


def test_downsample_bam_refuses_what_dedup_does_not_go_with(pkg, tmp_path):
    a, b = tmp_path / "in.bam", tmp_path / "out.bam"
    call = lambda solver="quasi-mcp-hip", **kw: pkg.downsample_bam(solver, a, b, 5, **kw)
    with pytest.raises(ValueError, match="per_reference"):
        call(dedup=True)
    for kw in (dict(targets=tmp_path / "t.bed"), dict(report=tmp_path / "r.tsv"), dict(ladder=[3], ladder_out="x{M}.bam"),
               dict(stratify="strand"), dict(bed=tmp_path / "a.bed"), dict(tsv=tmp_path / "a.tsv"),
               dict(amplicons_by_reference=True)):
        with pytest.raises(ValueError, match="duplicate-aware"):
            call(dedup=True, per_reference=True, **kw)
    with pytest.raises(ValueError, match="quality"):
        call("quasi-mcp-hip-quality", dedup=True, per_reference=True)
    with pytest.raises(ValueError, match="dedup_report needs dedup"):
        call(per_reference=True, dedup_report=tmp_path / "d.tsv")
    assert not b.exists()
