"""The characterisation grid of downsample_bam: every subset of at most two of SWITCHES on top of per_reference=True,
then each of LATER_SWITCHES alone and with each of LATER_PARTNERS (an explicit list: squaring the grid again would not
pay), on one tiny two-reference BAM, through the public downsample_bam alone.  `outcome` runs one case and returns what
it did -- the exception's type and message, or the returned counts with a hash of the DECODED records of every BAM
written (tests/bam_py.py reads them back; the compressed bytes depend on the zlib at hand) and the text of every report.
Run as a script on a GPU it records the cases the file does not hold yet (all of them into a new file) and leaves the
recorded ones as they are:

    python tests/downsample_grid.py tests/golden/downsample_grid.json

tests/test_downsample_grid_cpu.py and tests/test_gpu_downsample_grid.py replay the record.

The input comes from the writer in tests/bam_py.py: genome-downsampler_amd's write_synthetic_bam writes one reference
only, and the grid needs two so that per-reference grouping and mates on the other reference do something.  The lines
of a report that begin with ms_ are timings and are left out of the recorded text."""
import hashlib
import itertools
import json
import os
import sys

import numpy as np

import bam_py
import multi_reference as mr

REFERENCES = [("chrA", 3000), ("chrB", 2000)]
N_PAIRS = 200
MAX_COVERAGE = 3
MIN_MAPQ = 10
SWITCHES = ("single_reference", "bed", "targets", "report", "track", "ladder", "stratify", "dedup", "profile",
            "pair_aware", "template_aware", "template_targets", "ceiling", "budget_reads", "budget_fraction",
            "replicates", "quality")
CASES = [combo for k in range(3) for combo in itertools.combinations(SWITCHES, k)]
# the modes that came after the grid: alone, and with the three switches every one of them refuses
LATER_SWITCHES = ("proportion", "mean_depth", "budget_bases", "thresholds", "start_cap", "fragment_depth")
LATER_PARTNERS = ("report", "track", "quality")
CASES += [(name,) for name in LATER_SWITCHES]
CASES += [(name, partner) for partner in LATER_PARTNERS for name in LATER_SWITCHES]


def key_of(combo):
    return "+".join(combo) if combo else "plain"


def make_inputs(directory):
    """the BAM (pairs on two references at about 8 x, some mates on the other one, MAPQ 0 .. 60 so that min_mapq drops
    some pairs), a primer BED (one amplicon over most of each reference) and a three-line target BED and bedGraph that
    match it"""
    bam = os.path.join(directory, "in.bam")
    mr.write_multi_reference_bam(bam, np.random.default_rng(20), REFERENCES, N_PAIRS, other_ref=0.1, unmapped=0.0)
    primers = os.path.join(directory, "primers.bed")
    with open(primers, "w") as f:
        f.write("chrA\t100\t120\ta_LEFT\nchrA\t2880\t2900\ta_RIGHT\nchrB\t50\t70\tb_LEFT\nchrB\t1900\t1950\tb_RIGHT\n")
    bed = os.path.join(directory, "regions.bed")
    with open(bed, "w") as f:
        f.write("chrA\t200\t1200\nchrA\t1500\t2900\nchrB\t100\t1700\n")
    graph = os.path.join(directory, "caps.bedgraph")
    with open(graph, "w") as f:
        f.write("chrA\t200\t1200\t1\nchrA\t1500\t2900\t5\nchrB\t100\t1700\t2\n")
    return dict(bam=bam, primers=primers, bed=bed, graph=graph)


def arguments(combo, inputs, out_dir):
    """-> (solver name, keyword arguments of downsample_bam) for one case"""
    out = lambda name: os.path.join(out_dir, name)
    by_switch = {
        "single_reference": dict(per_reference=False),
        "bed": dict(bed=inputs["primers"], amplicons_by_reference=True),
        "targets": dict(targets=inputs["bed"], target_padding=20),
        "report": dict(report=out("depth.tsv"), report_bins=4),
        "track": dict(track=out("depth.bedgraph"), track_channel="both"),
        "ladder": dict(ladder=[2, 1], ladder_out=out("ladder_{M}.bam")),
        "stratify": dict(stratify="strand", strata_report=out("strata.tsv")),
        "dedup": dict(dedup=True, dedup_report=out("dedup.tsv")),
        "profile": dict(profile=inputs["graph"]),
        "pair_aware": dict(pair_aware=True),
        "template_aware": dict(template_aware=True, template_report=out("templates.tsv")),
        "template_targets": dict(template_targets=inputs["bed"]),
        "ceiling": dict(ceiling=True, ceiling_report=out("ceiling.tsv")),
        "budget_reads": dict(budget_reads=150, budget_report=out("budget.tsv")),
        "budget_fraction": dict(budget_fraction=0.5),
        "replicates": dict(replicates=3, replicates_out=out("replicate_{R}.bam"), replicates_report=out("replicates.tsv")),
        "quality": {},
        "proportion": dict(proportion=(1, 4), proportion_floor=1, proportional_report=out("proportional.tsv")),
        "mean_depth": dict(mean_depth=2.5, mean_depth_report=out("mean_depth.tsv")),
        "budget_bases": dict(budget_bases=20000, mean_depth_report=out("budget_bases.tsv")),
        "thresholds": dict(thresholds=(1, 4), thresholds_report=out("thresholds.tsv")),
        "start_cap": dict(start_cap=1, start_cap_by_strand=True, start_cap_report=out("start_cap.tsv")),
        "fragment_depth": dict(template_aware=True, fragment_depth=True, fragment_report=out("fragments.tsv"),
                               template_report=out("templates.tsv")),
    }
    kwargs = dict(per_reference=True, filtered_path=out("filtered.bam"), min_mapq=MIN_MAPQ)
    for name in combo:
        kwargs.update(by_switch[name])
    return ("quasi-mcp-hip-quality" if "quality" in combo else "quasi-mcp-hip"), kwargs


def _records_hash(path):
    _, records, _ = bam_py.parse(path)
    h = hashlib.sha256()
    for r in records:
        h.update(r["raw"])
    return f"{len(records)}:{h.hexdigest()[:16]}"


def outcome(pkg, combo, inputs, out_dir):
    """run one case in the empty directory out_dir -> its outcome as JSON-ready data"""
    solver_name, kwargs = arguments(combo, inputs, out_dir)
    try:
        got = pkg.downsample_bam(solver_name, inputs["bam"], os.path.join(out_dir, "out.bam"), MAX_COVERAGE, **kwargs)
    except Exception as e:  # noqa: BLE001 -- whatever it raises IS the outcome
        return dict(error=type(e).__name__, message=str(e).replace(os.path.dirname(inputs["bam"]), "<in>")
                    .replace(out_dir, "<out>"), files=sorted(os.listdir(out_dir)))
    bams, reports = {}, {}
    for name in sorted(os.listdir(out_dir)):
        path = os.path.join(out_dir, name)
        if name.endswith(".bam"):
            bams[name] = _records_hash(path)
        else:
            with open(path) as f:
                reports[name] = "".join(line for line in f if not line.startswith("ms_"))
    return dict(returned=got, bams=bams, reports=reports)


def main(argv):
    import importlib
    import tempfile

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    pkg = importlib.import_module("genome-downsampler_amd")
    record = json.load(open(argv[1])) if os.path.exists(argv[1]) else {}
    with tempfile.TemporaryDirectory() as tmp:
        inputs = make_inputs(tmp)
        for i, combo in enumerate(CASES):
            if key_of(combo) in record:
                continue
            out_dir = os.path.join(tmp, f"case{i}")
            os.mkdir(out_dir)
            record[key_of(combo)] = outcome(pkg, combo, inputs, out_dir)
            print(key_of(combo), record[key_of(combo)].get("error", "ran"), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(argv[1])), exist_ok=True)
    with open(argv[1], "w") as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv)
