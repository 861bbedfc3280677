"""Amplicons matched to references by name, the parts that need no GPU: the amplicon table of
genome-downsampler_amd/csrc/amplicon_table.h (compiled with g++ alone into tests/cpp/amplicon_table_driver.cpp) against
the brute-force predicate, BED / TSV parsing per reference against a Python restatement of its rules, and
per-reference ingest with FILTER and GRADE (BamApiConfig::amplicons_by_reference) on multi-reference files written by
the independent writer in tests/bam_py.py."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import amplicon_panels as ap
import bam_py
import multi_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QMCP_OK, QMCP_EINVAL = 0, -1


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("genome-downsampler_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("amplicon_table") / "amplicon_table_driver"
    out = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "amplicon_table_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def run_table(driver, cases):
    """cases: [(offs, starts, ends, n_amplicons or None, queries [(c, s1, e1, s2, e2)])] -> [(rc, [bool])]"""
    lines = []
    for offs, a0, a1, n_amp, queries in cases:
        n_amp = len(a0) if n_amp is None else n_amp
        lines.append(f"{len(offs) - 1} {n_amp}")
        lines.append(" ".join(str(int(x)) for x in list(offs) + list(a0) + list(a1)))
        lines.append(str(len(queries)))
        lines.extend(" ".join(str(int(x)) for x in q) for q in queries)
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = []
    for row in out.stdout.splitlines():
        parts = row.split()
        rows.append((int(parts[0][3:]), [ch == "1" for ch in (parts[1] if len(parts) > 1 else "")]))
    assert len(rows) == len(cases)
    return rows


def random_table(rng, n_contigs, max_amp, L):
    counts = rng.integers(0, max_amp + 1, size=n_contigs)
    counts[rng.random(n_contigs) < 0.2] = 0                       # empty contigs
    a0, a1 = [], []
    for k in counts:
        s = rng.integers(0, L, size=k)
        e = s + rng.integers(0, L // 3 + 1, size=k)
        if k > 1 and rng.random() < 0.5:                           # duplicates, touching and nested amplicons
            d = rng.integers(0, k, size=k // 3 + 1)
            s[:d.size], e[:d.size] = s[d], e[d]
            t = int(rng.integers(0, k))
            s[-1] = e[t]                                          # touching: starts where another ends
            n = int(rng.integers(0, k))
            s[0], e[0] = s[n] + 1, max(s[n] + 1, e[n] - 1)        # nested in another
        a0 += s.tolist()
        a1 += e.tolist()
    offs = np.concatenate([[0], np.cumsum(counts)])
    return offs, np.array(a0, np.int64), np.array(a1, np.int64)    # (unsorted: drawn in random order)


def brute(offs, a0, a1, q):
    c, s1, e1, s2, e2 = q
    return ap.in_one_amplicon(offs, a0, a1, c, s1, e1, c, s2, e2)


def test_table_predicate_equals_brute_force_on_a_seeded_grid(driver):
    rng = np.random.default_rng(2026)
    cases = []
    for _ in range(200):
        n_contigs = int(rng.integers(1, 12))
        L = int(rng.integers(50, 5000))
        offs, a0, a1 = random_table(rng, n_contigs, int(rng.integers(0, 30)), L)
        qs = []
        for _ in range(200):
            c = int(rng.integers(0, n_contigs))
            s = rng.integers(0, L + L // 3, size=2)
            e = s + rng.integers(0, 200, size=2)
            if rng.random() < 0.3 and offs[c + 1] > offs[c]:      # near an amplicon's bounds
                k = int(rng.integers(offs[c], offs[c + 1]))
                s = np.array([a0[k], a0[k] + rng.integers(0, 3)]) - rng.integers(0, 2)
                e = np.array([a1[k], a1[k] - rng.integers(0, 3)]) + rng.integers(0, 2)
                s, e = np.maximum(s, 0), np.maximum(e, np.maximum(s, 0))
            qs.append((c, int(s[0]), int(e[0]), int(s[1]), int(e[1])))
        cases.append((offs, a0, a1, None, qs))
    got = run_table(driver, cases)
    n_in = 0
    for (offs, a0, a1, _, qs), (rc, bits) in zip(cases, got):
        assert rc == QMCP_OK and len(bits) == len(qs)
        want = [brute(offs, a0, a1, q) for q in qs]
        assert bits == want
        n_in += sum(want)
    assert 0.05 * 200 * 200 < n_in < 0.95 * 200 * 200           # (both answers are exercised)


def test_table_handcrafted_cases_and_1e5_pairs(driver):
    # contig 0: nested, duplicated, touching, given out of order; contig 1 empty; contig 2 one amplicon
    offs = [0, 5, 5, 6]
    a0 = [100, 0, 50, 50, 300]
    a1 = [400, 200, 60, 60, 500]
    a0 += [10]
    a1 += [20]
    qs = [(0, 0, 10, 150, 200),    # inside [0, 200]
          (0, 0, 10, 150, 201),    # one past its end, and no other amplicon starts at 0
          (0, 100, 150, 300, 400),  # inside [100, 400], inclusive at both ends
          (0, 300, 310, 450, 500),  # inside [300, 500] only
          (0, 250, 260, 450, 501),  # past every end
          (0, 50, 55, 52, 60),     # the duplicate
          (1, 0, 1, 0, 1),         # an empty contig contains nothing
          (2, 10, 20, 10, 20),     # exactly the amplicon
          (2, 9, 20, 10, 20)]
    (rc, bits), = run_table(driver, [(offs, a0, a1, None, qs)])
    assert rc == QMCP_OK and bits == [True, False, True, True, False, True, False, True, False]
    # 10^5 pairs on one table
    rng = np.random.default_rng(5)
    offs, a0, a1 = random_table(rng, 40, 60, 30_000)
    c = rng.integers(0, 40, size=100_000)
    s = rng.integers(0, 30_000, size=(100_000, 2))
    e = s + rng.integers(0, 400, size=(100_000, 2))
    qs = np.stack([c, s[:, 0], e[:, 0], s[:, 1], e[:, 1]], axis=1)
    (rc, bits), = run_table(driver, [(offs, a0, a1, None, qs.tolist())])
    assert rc == QMCP_OK
    # brute force, vectorised per contig
    want = np.zeros(qs.shape[0], bool)
    lo_s, hi_e = np.minimum(qs[:, 1], qs[:, 3]), np.maximum(qs[:, 2], qs[:, 4])
    for k in range(40):
        sel = np.flatnonzero(qs[:, 0] == k)
        amps = slice(offs[k], offs[k + 1])
        if offs[k + 1] > offs[k]:
            want[sel] = ((a0[amps][None, :] <= lo_s[sel, None]) & (hi_e[sel, None] <= a1[amps][None, :])).any(axis=1)
    assert np.array_equal(np.array(bits), want) and want.any()


def test_table_refuses_bad_offsets(driver):
    good = ([0, 1, 2], [0, 5], [3, 9])
    cases = [(good[0], good[1], good[2], None, []),
             ([1, 1, 2], [0, 5], [3, 9], None, []),        # does not start at 0
             ([0, 2, 1], [0, 5], [3, 9], None, []),        # decreases
             ([0, 1, 1], [0, 5], [3, 9], 2, []),           # does not end at n_amplicons
             ([0, 0], [], [], None, [(0, 1, 2, 1, 2)])]    # no amplicons at all: valid, contains nothing
    got = run_table(driver, cases)
    assert [rc for rc, _ in got] == [QMCP_OK, QMCP_EINVAL, QMCP_EINVAL, QMCP_EINVAL, QMCP_OK]
    assert got[4][1] == [False]


# ---------------------------------------------------------------- BED / TSV by reference
def write_bed(path, lines):
    with open(path, "w") as f:
        for chrom, s, e, name in lines:
            f.write(f"{chrom}\t{s}\t{e}\t{name}\t1\t+\n")


def random_bed(rng, chroms, n):
    lines = []
    for _ in range(n):
        chrom = chroms[int(rng.integers(0, len(chroms)))]
        s = int(rng.integers(0, 10_000))
        lines.append((chrom, s, s + 25, f"p{int(rng.integers(0, n))}_{'LR'[int(rng.integers(0, 2))]}"))
    return lines


def test_bed_and_tsv_by_reference_equal_the_restated_rules(pkg, tmp_path):
    rng = np.random.default_rng(17)
    refs = ["chr1", "chr2", "MN908947.3", "seg_4", "chrM"]
    for trial in range(60):
        chroms = list(rng.choice(refs, size=int(rng.integers(1, len(refs) + 1)), replace=False))
        lines = random_bed(rng, chroms, int(rng.integers(0, 80)))
        bed = tmp_path / f"t{trial}.bed"
        write_bed(bed, lines)
        want = ap.restate_amplicons(lines, None, refs)       # per-chrom pairing in name order
        got = pkg.amplicons_by_reference(bed, None, refs)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), trial
        # TSV pairs within a chrom (some names missing from the BED, some primers reused)
        names = sorted({ln[3] for ln in lines})
        chrom_of = {}
        for c, _, _, n in lines:
            chrom_of.setdefault(n, c)
        pairs = []
        for _ in range(int(rng.integers(0, 30))):
            if not names:
                break
            a = names[int(rng.integers(0, len(names)))]
            same = [n for n in names if chrom_of[n] == chrom_of[a]]
            b = same[int(rng.integers(0, len(same)))] if rng.random() < 0.9 else f"missing_{chrom_of[a]}_{int(rng.integers(0, 3))}"
            pairs.append((a, b) if rng.random() < 0.5 else (b, a))
        tsv = tmp_path / f"t{trial}.tsv"
        tsv.write_text("".join(f"{a}\t{b}\n" for a, b in pairs))
        want = ap.restate_amplicons(lines, pairs, refs)
        got = pkg.amplicons_by_reference(bed, tsv, refs)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), trial


def test_by_reference_errors_name_the_culprit(pkg, tmp_path):
    refs = ["chr1", "chr2"]
    bed = tmp_path / "p.bed"
    write_bed(bed, [("chr1", 0, 25, "a_LEFT"), ("chr1", 300, 325, "a_RIGHT"), ("1", 500, 525, "b_LEFT"),
                    ("1", 800, 825, "b_RIGHT")])
    with pytest.raises(ValueError, match='"1"'):             # no aliases: "1" is not "chr1"
        pkg.amplicons_by_reference(bed, None, refs)
    write_bed(bed, [("chr1", 0, 25, "a_LEFT"), ("chr2", 300, 325, "a_RIGHT")])
    tsv = tmp_path / "p.tsv"
    tsv.write_text("a_LEFT\ta_RIGHT\n")
    with pytest.raises(ValueError, match="a_LEFT / a_RIGHT"):
        pkg.amplicons_by_reference(bed, tsv, refs)
    # without the TSV the same BED is fine: one primer per chrom, nothing to pair
    offs, a0, a1 = pkg.amplicons_by_reference(bed, None, refs)
    assert offs.tolist() == [0, 0, 0] and a0.size == 0


def test_one_chrom_equals_amplicons_from_files(pkg, tmp_path):
    import workloads
    a0, a1 = workloads.amplicon_panel()
    bed, tsv = tmp_path / "primers.bed", tmp_path / "pairs.tsv"
    ap.write_panel_files({"MN908947.3": list(zip(a0.tolist(), a1.tolist()))}, bed, tsv)
    for t in (tsv, None):
        f0, f1 = pkg.amplicons_from_files(str(bed), str(t) if t else None)
        offs, b0, b1 = pkg.amplicons_by_reference(bed, t, ["MN908947.3"])
        assert offs.tolist() == [0, f0.size] and np.array_equal(b0, f0) and np.array_equal(b1, f1)
        # the reference order of the header decides the CSR; other references get nothing
        offs, b0, b1 = pkg.amplicons_by_reference(bed, t, ["chrX", "MN908947.3", "chrY"])
        assert offs.tolist() == [0, 0, f0.size, f0.size] and np.array_equal(b0, f0) and np.array_equal(b1, f1)


# ---------------------------------------------------------------- ingest
REFS = [("seg1", 2341), ("seg2", 2341), ("seg3", 2233), ("seg4", 1778), ("seg5", 1565), ("seg6", 1413),
        ("seg7", 1027), ("seg8", 890)]


@pytest.fixture(scope="module")
def panel_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("panel")
    panel = ap.tiled_panel(REFS[:7], 25, size=300, step=150)        # seg8 has no amplicons
    path = d / "panel.bam"
    header, parsed, ref_lengths = ap.write_panel_bam(path, np.random.default_rng(3), REFS, panel, 4000)
    bed, tsv = d / "panel.bed", d / "panel.tsv"
    ap.write_panel_files(panel, bed, tsv)
    return path, header, parsed, ref_lengths, panel, bed, tsv


def test_filter_ingest_equals_the_restated_pairing(pkg, panel_file):
    path, _, parsed, ref_lengths, panel, bed, tsv = panel_file
    offs, a0, a1 = ap.panel_csr(panel, [n for n, _ in REFS])
    inside = ap.inside_by_reference(parsed, offs, a0, a1)
    for t, min_len, min_q in ((tsv, 0, 0), (None, 0, 0), (tsv, 120, 20)):
        got = pkg.read_bam(path, bed=bed, tsv=t, amplicon_mode=1, min_length=min_len, min_mapq=min_q,
                           per_reference=True, amplicons_by_reference=True)
        reads, filtered = bam_py.pair_like_the_reference(parsed, min_len=min_len, min_mapq=min_q, inside=inside)
        ids = [parsed[r["bam_id"]]["ref_id"] for r in reads]
        assert got["bam_ids"].tolist() == [r["bam_id"] for r in reads]
        assert got["contig_ids"].tolist() == ids
        assert got["starts"].tolist() == [r["start"] for r in reads]
        assert got["ends"].tolist() == [r["end"] for r in reads]
        assert got["filtered_out"].tolist() == filtered
        assert got["contig_lengths"].tolist() == ref_lengths
        # every survivor pair lies on one reference with amplicons; mates across references and unmapped mates are gone
        assert all(i == j and i < 7 for i, j in zip(ids[0::2], ids[1::2]))
        all_pairs = len(bam_py.pair_like_the_reference(parsed)[0]) // 2
        assert (0.5 if min_len == 0 else 0.1) * all_pairs < len(reads) // 2 < all_pairs


def test_grade_ingest_grades_by_the_per_reference_predicate(pkg, panel_file):
    path, _, parsed, _, panel, bed, tsv = panel_file
    offs, a0, a1 = ap.panel_csr(panel, [n for n, _ in REFS])
    inside = ap.inside_by_reference(parsed, offs, a0, a1)
    got = pkg.read_bam(path, bed=bed, tsv=tsv, amplicon_mode=2, per_reference=True, amplicons_by_reference=True)
    reads, filtered = bam_py.pair_like_the_reference(parsed)         # GRADE filters nothing
    assert got["bam_ids"].tolist() == [r["bam_id"] for r in reads] and got["filtered_out"].tolist() == filtered
    q = np.array([r["q"] for r in reads], dtype=np.int64)
    lo, hi = int(q.min()), int(q.max())
    single = np.repeat([inside(reads[i], reads[i + 1]) for i in range(0, len(reads), 2)], 2)
    want = q - lo + np.where(single, hi - lo, 0)
    assert got["qualities"].tolist() == want.tolist()
    assert single.any() and not single.all()
    # IGNORE with the flag == per-reference ingest without a BED
    ign = pkg.read_bam(path, bed=bed, tsv=tsv, amplicon_mode=0, per_reference=True, amplicons_by_reference=True)
    plain = pkg.read_bam(path, per_reference=True)
    for k in ("bam_ids", "starts", "ends", "qualities", "contig_ids", "filtered_out", "contig_lengths"):
        assert np.array_equal(ign[k], plain[k]), k


def test_refusals_old_and_new(pkg, panel_file, tmp_path):
    path, _, _, _, _, bed, tsv = panel_file
    with pytest.raises(ValueError, match="per_reference"):          # the flag alone is refused
        pkg.read_bam(path, bed=bed, tsv=tsv, amplicon_mode=1, amplicons_by_reference=True)
    with pytest.raises(ValueError, match="amplicons are not matched to references by name"):   # unchanged
        pkg.read_bam(path, bed=bed, per_reference=True)
    with pytest.raises(ValueError, match="amplicons_by_reference"):
        pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "o.bam", 10, per_reference=True, bed=bed)
    bad = tmp_path / "bad.bed"
    write_bed(bad, [("seg1", 0, 25, "a_LEFT"), ("seg9", 300, 325, "a_RIGHT")])
    with pytest.raises(ValueError, match='"seg9"'):
        pkg.read_bam(path, bed=bad, amplicon_mode=1, per_reference=True, amplicons_by_reference=True)
    assert pkg.reference_names(path) == [n for n, _ in REFS]
