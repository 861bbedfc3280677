"""downsample_bam(primer_clip=, per_amplicon=, amplicon_report=): the file-to-file flow of the amplicon-aware entry on a
panel BAM with 25-base primers -- the written records are the model's kept set (tests/amplicon_clip_model.py on
read_bam's columns with the inserts from the BED), the TSV is write_amplicon_report of the model's rows, and without the
new keywords the written file is byte for byte the plain flow's."""
import numpy as np
import pytest

import amplicon_clip_model as am
import amplicon_panels as ap
import bam_py

pytestmark = pytest.mark.gpu

REFS = [("seg1", 2300), ("seg2", 1700), ("bare", 900)]
M = 8


@pytest.fixture(scope="module")
def panel(tmp_path_factory):
    """2 000 pairs on a tiled panel over two references (a third has no amplicons), mates within 25 bases of the
    amplicon's ends: every read starts or ends inside a primer"""
    d = tmp_path_factory.mktemp("amplicon_clip")
    tiled = ap.tiled_panel(REFS[:2], 8)
    path, bed, tsv = d / "panel.bam", d / "panel.bed", d / "panel.tsv"
    header, parsed, _ = ap.write_panel_bam(path, np.random.default_rng(61), REFS, tiled, 2000)
    ap.write_panel_files(tiled, bed, tsv)
    return dict(path=path, bed=bed, tsv=tsv, tiled=tiled, header=header, parsed=parsed)


def tables(pkg, panel):
    names = pkg.reference_names(panel["path"])
    offs, a0, a1 = pkg.amplicons_by_reference(panel["bed"], panel["tsv"], names)
    i0, i1, left = pkg.amplicon_inserts_by_reference(panel["bed"], panel["tsv"], names)
    want = ap.panel_csr(panel["tiled"], names)
    assert all(np.array_equal(x, y) for x, y in zip((offs, a0, a1), want))
    # write_panel_files' primers are [lo, lo + 24) and [hi - 24, hi): the insert is [lo + 24, hi - 25]
    assert np.array_equal(i0, a0 + 24) and np.array_equal(i1, a1 - 25) and left[0] == "seg1_amp0_LEFT"
    chroms = [names[c] for c in np.repeat(np.arange(len(names)), np.diff(offs.astype(np.int64)))]
    return offs, a0, a1, i0, i1, left, chroms


@pytest.mark.parametrize("per_amplicon", [False, True])
def test_the_written_records_and_the_report_are_the_models(pkg, oracle, panel, tmp_path, per_amplicon):
    offs, a0, a1, i0, i1, left, chroms = tables(pkg, panel)
    cols = pkg.read_bam(panel["path"], per_reference=True)
    n = cols["starts"].size
    keep, lab, rows, st = am.solve(oracle, cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"], M, offs,
                                   a0, a1, i0, i1, per_amplicon=per_amplicon, complete_pairs=True)
    assert st["units_no_amplicon"] > 0 and st["reads_shortened"] > n // 2 and 0 < keep.sum() < n // 2
    out, tsv = tmp_path / "out.bam", tmp_path / "amplicons.tsv"
    written = pkg.downsample_bam("quasi-mcp-hip", panel["path"], out, M, per_reference=True, bed=panel["bed"],
                                 tsv=panel["tsv"], amplicons_by_reference=True, primer_clip=True,
                                 per_amplicon=per_amplicon, amplicon_report=tsv)
    kept_ids = np.sort(cols["bam_ids"][keep].astype(np.int64))
    oh, orecs, _ = bam_py.parse(out)
    assert oh == panel["header"] and written == kept_ids.size == len(orecs)
    # the ORIGINAL records: clipping decides what counts as depth, not what is written
    assert [r["raw"] for r in orecs] == [panel["parsed"][i]["raw"] for i in kept_ids.tolist()]
    assigned = lab != am.NO_AMPLICON
    units = np.bincount(lab[assigned].astype(np.int64), minlength=a0.size)
    read_lab = np.repeat(lab, 2)
    reads_kept = np.bincount(read_lab[keep].astype(np.int64), minlength=a0.size)
    want = tmp_path / "want.tsv"
    pkg.write_amplicon_report(want, chroms, a0, a1, left, units, reads_kept, rows)
    assert open(tsv).read() == open(want).read()
    assert len(open(tsv).read().splitlines()) == 1 + a0.size


def test_clipping_changes_the_selection_and_the_report_alone_does_not(pkg, panel, tmp_path):
    """without the new keywords the file is the plain flow's, byte for byte (this holds before the feature too); the
    report alone runs the entry with clipping off and pooled, which selects the same reads"""
    kw = dict(per_reference=True, bed=panel["bed"], tsv=panel["tsv"], amplicons_by_reference=True)
    plain, again, reported, clipped = (tmp_path / f"{k}.bam" for k in ("plain", "again", "reported", "clipped"))
    w0 = pkg.downsample_bam("quasi-mcp-hip", panel["path"], plain, M, **kw)
    w1 = pkg.downsample_bam("quasi-mcp-hip", panel["path"], again, M, primer_clip=False, per_amplicon=False,
                            amplicon_report=None, **kw)
    assert w0 == w1 > 0 and open(plain, "rb").read() == open(again, "rb").read()
    w2 = pkg.downsample_bam("quasi-mcp-hip", panel["path"], reported, M, amplicon_report=tmp_path / "r.tsv", **kw)
    assert w2 == w0 and open(plain, "rb").read() == open(reported, "rb").read()
    lines = [l.split("\t") for l in open(tmp_path / "r.tsv").read().splitlines()[1:]]
    assert all(l[1] == l[3] and l[2] == l[4] for l in lines)       # clipping off: the insert is the amplicon
    pkg.downsample_bam("quasi-mcp-hip", panel["path"], clipped, M, primer_clip=True, **kw)
    assert open(plain, "rb").read() != open(clipped, "rb").read()


def test_the_plain_flow_is_unchanged(pkg, panel, tmp_path):
    """guards "no existing behaviour changes": passes before the feature as well"""
    kw = dict(per_reference=True, bed=panel["bed"], tsv=panel["tsv"], amplicons_by_reference=True)
    a, b = tmp_path / "a.bam", tmp_path / "b.bam"
    assert pkg.downsample_bam("quasi-mcp-hip", panel["path"], a, M, **kw) == \
        pkg.downsample_bam("quasi-mcp-hip", panel["path"], b, M, filtered_path=tmp_path / "f.bam", **kw)
    assert open(a, "rb").read() == open(b, "rb").read()
    recs = bam_py.parse(a)[1]
    assert 0 < len(recs) < len(panel["parsed"])
