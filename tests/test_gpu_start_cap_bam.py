"""downsample_bam(start_cap=): the file-to-file flow of the start cap on a two-reference BAM with both strands and MAPQ
0 .. 60 -- the written records are the model's kept set (tests/start_cap_model.py on read_bam's columns, group = strand,
priority = MAPQ) completed by the oracle's find_pairs, the report holds the model's numbers, and a cap larger than any
pile writes the plain flow's file record for record."""
import numpy as np
import pytest

import bam_py
import start_cap_model as sm

pytestmark = pytest.mark.gpu

REFS = [("chrA", 3000), ("chrB", 2000)]
REPORT_KEYS = ("cap",) + sm.STAT_KEYS + ("records_written",)


@pytest.fixture(scope="module")
def piled_bam(tmp_path_factory):
    """300 pairs whose mates start on a few dozen sites of two references: piles of several reads on one start, on both
    strands, with three read lengths and every MAPQ"""
    rng = np.random.default_rng(51)
    path = tmp_path_factory.mktemp("start_cap") / "piles.bam"
    sites = [np.sort(rng.integers(0, length - 600, size=25)) for _, length in REFS]
    recs = []
    for q in range(300):
        ref = int(rng.integers(0, 2))
        site = int(rng.choice(sites[ref]))
        reverse = bool(rng.random() < 0.5)
        for first in (True, False):
            flag = (0x41 if first else 0x81) | (0x10 if reverse == first else 0)
            pos = site if first else site + int(rng.choice([120, 200, 310]))
            match = int(rng.choice([60, 100, 150]))
            mapq = q % 61 if first else int(rng.integers(0, 61))
            recs.append(bam_py.pack_record(f"p{q}", flag, pos, mapq, [(match, "M")], match, ref_id=ref))
    recs = [recs[i] for i in rng.permutation(len(recs))]
    bam_py.write_bam(path, REFS, recs)
    return path


def test_the_written_records_and_the_report_are_the_models(pkg, oracle, piled_bam, tmp_path):
    header, parsed, _ = bam_py.parse(piled_bam)
    cols = pkg.read_bam(piled_bam, per_reference=True, stratify="strand")
    n = cols["starts"].size
    assert n == 600 and set(cols["strata"].tolist()) == {0, 1} and set(cols["contig_ids"].tolist()) == {0, 1}
    assert cols["qualities"].min() == 0 and cols["qualities"].max() == 60
    M, K = 3, 2
    keep, capped, st, hist = sm.start_cap(oracle, cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"],
                                          M, K, groups=cols["strata"], priorities=cols["qualities"], shortfall=True,
                                          hist_bins=pkg.START_CAP_REPORT_BINS)
    assert st["cells_over_cap"] > 20 and st["reads_capped"] > 100 and 0 < keep.sum() < st["reads_survived"]
    out, tsv = tmp_path / "out.bam", tmp_path / "cap.tsv"
    written = pkg.downsample_bam("quasi-mcp-hip", piled_bam, out, M, per_reference=True, start_cap=K,
                                 start_cap_by_strand=True, start_cap_report=tsv)
    completed = pkg.mask_to_indices(oracle.find_pairs(sm.pack(keep), n), n).astype(np.int64)
    kept_ids = np.sort(cols["bam_ids"][completed].astype(np.int64))
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == kept_ids.size == len(orecs)
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]
    lines = [l.split("\t") for l in open(tsv).read().splitlines()]
    assert lines[0] == ["#stat", "value"]
    rows = {l[0]: int(l[1]) for l in lines[1:1 + len(REPORT_KEYS)]}
    assert tuple(l[0] for l in lines[1:1 + len(REPORT_KEYS)]) == REPORT_KEYS
    assert rows == dict(st, cap=K, records_written=written)
    assert lines[1 + len(REPORT_KEYS)] == ["#size", "cells"]
    bins = [(int(a), int(b)) for a, b in lines[2 + len(REPORT_KEYS):]]
    assert bins == [(k + 1, int(hist[k])) for k in range(pkg.START_CAP_REPORT_BINS)]
    # without the strand the sites are (reference, start): fewer, larger cells
    tsv2 = tmp_path / "cap2.tsv"
    written2 = pkg.downsample_bam("quasi-mcp-hip", piled_bam, tmp_path / "out2.bam", M, per_reference=True, start_cap=K,
                                  start_cap_report=tsv2)
    keep2, _, st2, _ = sm.start_cap(oracle, cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"], M, K,
                                    priorities=cols["qualities"], shortfall=True)
    rows2 = dict(l.split("\t") for l in open(tsv2).read().splitlines()[1:1 + len(REPORT_KEYS)])
    assert {k: int(v) for k, v in rows2.items()} == dict(st2, cap=K, records_written=written2)
    assert st2["cells"] < st["cells"]
    ids2 = np.sort(cols["bam_ids"][pkg.mask_to_indices(oracle.find_pairs(sm.pack(keep2), n), n).astype(np.int64)].astype(np.int64))
    assert [r["raw"] for r in bam_py.parse(tmp_path / "out2.bam")[1]] == [parsed[i]["raw"] for i in ids2.tolist()]


def test_a_cap_above_every_pile_writes_the_plain_flows_file(pkg, piled_bam, tmp_path):
    plain, capped, tsv = tmp_path / "plain.bam", tmp_path / "capped.bam", tmp_path / "cap.tsv"
    w0 = pkg.downsample_bam("quasi-mcp-hip", piled_bam, plain, 3, per_reference=True)
    w1 = pkg.downsample_bam("quasi-mcp-hip", piled_bam, capped, 3, per_reference=True, start_cap=1000,
                            start_cap_by_strand=True, start_cap_report=tsv)
    h0, r0, _ = bam_py.parse(plain)
    h1, r1, _ = bam_py.parse(capped)
    assert w0 == w1 == len(r0) and h0 == h1 and [r["raw"] for r in r0] == [r["raw"] for r in r1]
    rows = dict(l.split("\t") for l in open(tsv).read().splitlines()[1:1 + len(REPORT_KEYS)])
    assert int(rows["reads_capped"]) == int(rows["cells_over_cap"]) == int(rows["short_positions"]) == 0
