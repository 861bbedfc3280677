"""downsample_bam(proportion=...): the file flow of proportional downsampling on a small synthetic BAM with two
references -- the written records are the model's kept set completed by the oracle's find_pairs, and the report's lines
are the solve's statistics."""
import numpy as np
import pytest

import bam_py
import multi_reference as mr
import profile_model as pm
import proportional_model as qm

pytestmark = pytest.mark.gpu

NO_CONTIG = 0xFFFFFFFF
COUNTS = ["reads_placed", "bases_in", "bases_kept", "demand", "whole_positions", "floor_positions", "capped_positions",
          "max_depth", "max_need", "num", "den", "floor", "plain_route"]


@pytest.mark.parametrize("proportion,floor,M", [(0.25, 0, qm.NO_LIMIT), ((2, 3), 2, 6)])
def test_downsample_bam_writes_the_models_reads_and_reports_the_stats(pkg, solver, oracle, tmp_path, proportion, floor, M):
    path = tmp_path / "in.bam"
    refs = [("chrA", 3000), ("chrB", 1200)]
    header, parsed, _ = mr.write_multi_reference_bam(path, np.random.default_rng(23), refs, 600)
    cols = pkg.read_bam(path, per_reference=True)
    s, e, ids, lengths = cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"]
    n = s.size
    num, den = pkg.as_ratio(proportion)
    want = qm.expected_mask(s, e, ids, lengths, num, den, floor, M, fast=True)
    kept = pm.unpack(want, n)
    assert 0 < kept.sum() < (ids != NO_CONTIG).sum()                              # the fraction bites
    restated = qm.stats(s, e, ids, lengths, num, den, floor, M, want)
    mask = oracle.find_pairs(want, n)
    kept_ids = np.sort(np.asarray(cols["bam_ids"], np.int64)[pkg.mask_to_indices(mask, n).astype(np.int64)])
    assert np.unique(kept_ids).size == kept_ids.size
    out, report = tmp_path / "out.bam", tmp_path / "proportional.tsv"
    written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, proportion=proportion,
                                 proportion_floor=floor, proportional_report=report)
    oh, orecs, _ = bam_py.parse(out)
    assert oh == header and written == kept_ids.size == len(orecs)
    assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]
    text = report.read_text().splitlines()
    assert text[0] == "#stat\tvalue"
    rows = dict(line.split("\t") for line in text[1:])
    assert list(rows) == COUNTS + ["records_written"]
    assert {k: int(rows[k]) for k in COUNTS} == restated and int(rows["records_written"]) == written
    solver.solve_proportional(s, e, ids, lengths, proportion, floor, M)           # the entry itself, on the file's reads
    direct = solver.last_proportional_stats.as_dict()
    assert {k: int(direct[k]) for k in COUNTS} == restated
