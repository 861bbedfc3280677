"""The sweep planner (genome-downsampler_amd/csrc/sweep_plan.h) on the CPU: the header compiled with g++ alone into a
small driver (tests/cpp/sweep_plan_driver.cpp), asked for the plans of shapes whose decision a commit or a comment
records, for every option that overrides the data-driven choice, and -- on a seeded grid -- whether the multi-device
cost model's predicate agrees with its Python mirror in sharding.py."""
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNKNOWN = 0xFFFFFFFF
SWEEP_FAST, SWEEP_GENERAL, SWEEP_EVENTS = 1, 2, 3   # QMCP_SWEEP_*


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sweep_plan") / "sweep_plan_driver"
    out = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                          "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "sweep_plan_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def run(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    plans = []
    for row in out.stdout.splitlines():
        d = dict(kv.split("=", 1) for kv in row.split())
        plans.append({k: (v if k == "form" else int(v)) for k, v in d.items()})
    assert len(plans) == len(lines)
    return plans


def line(route, **fields):
    return route + " " + " ".join(f"{k}={v}" for k, v in fields.items())


def poisson_empty(n, ltot):
    """start positions without a read where n reads start uniformly on ltot positions"""
    return round(ltot * math.exp(-n / ltot))


def reads_at(depth, ltot, M, span):
    return round(depth * ltot * M / span)


def uniform(driver, n, span, ltot, contigs, M, empty=None, **opt):
    empty = poisson_empty(n, ltot) if empty is None else empty
    return run(driver, [line("uniform", n=n, span=span, ltot=ltot, contigs=contigs, M=M, empty=empty, **opt)])[0]


def near(driver, n, ell, ltot, contigs, longest, M, min_span=None, may_rank=1, **opt):
    min_span = ell - 40 if min_span is None else min_span
    return run(driver, [line("near", n=n, ell=ell, min_span=min_span, ltot=ltot, contigs=contigs, longest=longest, M=M,
                             may_rank=may_rank, **opt)])[0]


def mixed(driver, n, span, ltot, contigs, M, share=None, longest=None, in_regs=1, hopeless=0, **opt):
    fields = dict(n=n, span=span, ltot=ltot, contigs=contigs, M=M, in_regs=in_regs, hopeless=hopeless, **opt)
    if share is not None:
        fields.update(s0=share[0], s1=share[1], s2=share[2], longest=ltot if longest is None else longest)
    return run(driver, [line("mixed", **fields)])[0]


# ------------------------------------------------------------------ the one-span route
def test_cfg4_sweeps_whole_contigs_event_driven(driver):
    """cfg4 (10^8 reads on 8 contigs of 10^6 positions, reads of 150, M = 100: 18.75 x M): the event-driven chain,
    no cut-point windows"""
    p = uniform(driver, 100_000_000, 150, 8_000_000, 8, 100)
    assert p["form"] == "events" and p["windows"] == 0 and not p["speculate"]


def test_sparse_deep_contig_takes_speculative_stretches_with_three_run_ins(driver):
    """168cb02: one contig of 82.6 M positions, 66 M reads of 150, M = 10 -- 12 x M, yet 0.8 reads a position: the general
    pipeline in speculative stretches, with three times the table's run-in (3 x 1 536 = 4 608 blocks)"""
    p = uniform(driver, 66_000_000, 150, 82_600_000, 1, 10)
    assert p["form"] == "spec_general" and p["speculate"] and p["windows"] > 0
    assert p["burn_blocks"] == 3 * 1536
    assert (p["unit"], p["round_to"], p["run_ins_apart"], p["min_run_ins"]) == (150, 150, 4, 8)


def test_large_M_upper_bound_by_sigma_depth(driver):
    """6009694: on one contig of 20 M positions, M = 400 at 3 x M and M = 200 at 4 x M (sigma depths 12.6 and 10.9) are not
    speculated on; M = 400 at 2 x M (5.8) is"""
    L = 20_000_000
    for M, depth, want in ((400, 3, False), (200, 4, False), (400, 2, True)):
        p = uniform(driver, reads_at(depth, L, M, 150), 150, L, 1, M)
        assert p["form"] == ("spec_general" if want else "general"), (M, depth, p)
        assert bool(p["speculate"]) == want and p["windows"] > 0


def test_large_M_lower_bound_by_sigma_depth(driver):
    """4a3a7f2: M = 400 at 1.2 x M is below kSpecMinDepth by its raw depth, above it by its sigma depth (1.67): speculated
    on, where the contig holds eight run-ins (11.9 M reads on 3.7 M positions)"""
    p = uniform(driver, 11_900_000, 150, 3_700_000, 1, 400)
    assert p["form"] == "spec_general" and p["speculate"]
    assert 3_700_000 >= 8 * p["burn_blocks"] * 150


def test_uniform_overrides(driver):
    n, L = 100_000_000, 8_000_000
    shallow = reads_at(2, 20_000_000, 50, 150)
    # sweep: general on deep data -- overridden before the windows are computed, so the contigs are cut too
    p = uniform(driver, n, 150, L, 8, 100, sweep=SWEEP_GENERAL)
    assert p["form"] == "general" and p["windows"] > 0 and not p["speculate"]
    # ... and speculation forced on, on top of it
    p = uniform(driver, n, 150, L, 8, 100, sweep=SWEEP_GENERAL, spec=1)
    assert p["form"] == "spec_general" and p["speculate"]
    # speculation forced on alone does not leave the event-driven form on deep data
    assert uniform(driver, n, 150, L, 8, 100, spec=1)["form"] == "events"
    # sweep: fast on shallow data -- no windows either (they follow the form)
    p = uniform(driver, shallow, 150, 20_000_000, 1, 50, sweep=SWEEP_FAST)
    assert p["form"] == "fast" and p["windows"] == 0 and not p["speculate"]
    # sweep: events on shallow data -- the windows stay
    p = uniform(driver, shallow, 150, 20_000_000, 1, 50, sweep=SWEEP_EVENTS)
    assert p["form"] == "events" and p["windows"] > 0
    # the default there, and speculation forced off
    assert uniform(driver, shallow, 150, 20_000_000, 1, 50)["form"] == "spec_general"
    p = uniform(driver, shallow, 150, 20_000_000, 1, 50, spec=-1)
    assert p["form"] == "general" and p["windows"] > 0 and not p["speculate"]
    # cut points: never (no windows, so no stretches), always (deep data is cut too, and stays event-driven)
    p = uniform(driver, shallow, 150, 20_000_000, 1, 50, cuts=-1)
    assert p["form"] == "general" and p["windows"] == 0
    p = uniform(driver, n, 150, L, 8, 100, cuts=1)
    assert p["form"] == "events" and p["windows"] > 0
    # the first tier's run-in: as given, never tripled on sparse deep data
    assert uniform(driver, 66_000_000, 150, 82_600_000, 1, 10, run_in=500)["burn_blocks"] == 500
    assert uniform(driver, shallow, 150, 20_000_000, 1, 50, run_in=500)["burn_blocks"] == 500


def test_uniform_shape_limits(driver):
    # spans beyond the seven-wave pipelines: the single-wave kernel; empty positions unknown: never event-driven
    assert uniform(driver, 20_000_000, 400, 8_000_000, 8, 20)["form"] == "single_wave"
    assert uniform(driver, 100_000_000, 150, 8_000_000, 8, 100, empty=UNKNOWN)["form"] == "fast"
    # spans below ev_min_span() and M beyond the packed field keep the block scan
    assert uniform(driver, 1_000_000_000, 20, 8_000_000, 8, 100)["form"] == "fast"
    assert uniform(driver, 60_000_000, 250, 8_000_000, 8, 100)["form"] == "fast"


# ------------------------------------------------------------------ the near-uniform route
def test_near_uniform_M_beyond_the_packed_field_takes_the_block_scan(driver):
    """d96b09c: M = 200, reads of 250 at 12 x M on 24 contigs of at most 2 M positions: M does not fit a packed field of
    the event-driven form, so the rounds run the block-scan pipeline (stretches), without speculation"""
    L = 11_730_000
    p = near(driver, reads_at(12, L, 200, 250), 250, L, 24, 500_000, 200)
    assert p["tried"] and p["stretches"] and not p["speculate"]


def test_near_uniform_depths(driver):
    """1.5 x M, reads of 150, M = 100: tried, in stretches.  At 6 x M on a 10^6-position contig the comment's rule (up to
    2 M positions keep the chain) holds where the data is not sparse -- M = 200, 8 reads a position --; with M = 100 the
    reads are sparse (4 a position < ln(150 / 0.693)) and 8a39558 sends them to stretches too."""
    p = near(driver, reads_at(1.5, 1_000_000, 100, 150), 150, 1_000_000, 1, 1_000_000, 100)
    assert p["tried"] and p["stretches"] and p["windows"] > 0
    p = near(driver, reads_at(6, 1_000_000, 200, 150), 150, 1_000_000, 1, 1_000_000, 200)
    assert p["tried"] and not p["stretches"] and p["windows"] == 0 and not p["speculate"]
    p = near(driver, reads_at(6, 1_000_000, 100, 150), 150, 1_000_000, 1, 1_000_000, 100)
    assert p["tried"] and p["stretches"]


def test_near_uniform_not_tried(driver):
    n = reads_at(3, 1_000_000, 100, 150)
    assert near(driver, n, 150, 1_000_000, 1, 1_000_000, 100)["tried"]
    assert not near(driver, n, 150, 1_000_000, 1, 1_000_000, 100, may_rank=0)["tried"]
    assert not near(driver, n, 150, 1_000_000, 1, 1_000_000, 100, min_span=0)["tried"]
    # below a sigma depth of 1.5 (M = 20 at 1.4 x M: 1.24), unless the option lowers the gate
    n = reads_at(1.4, 1_000_000, 20, 150)
    assert not near(driver, n, 150, 1_000_000, 1, 1_000_000, 20)["tried"]
    assert near(driver, n, 150, 1_000_000, 1, 1_000_000, 20, nu_min_depth=1.2)["tried"]
    # long deep contigs the pipeline would sweep as one chain: the event-driven chain only, and not where M does not fit
    L = 11_730_000
    assert not near(driver, reads_at(12, L, 200, 250), 250, L, 1, L, 200)["tried"]


def test_near_uniform_overrides(driver):
    shallow = reads_at(1.5, 1_000_000, 100, 150)
    deep = reads_at(6, 1_000_000, 200, 150)
    p = near(driver, shallow, 150, 1_000_000, 1, 1_000_000, 100, sweep=SWEEP_EVENTS)
    assert p["tried"] and not p["stretches"] and p["windows"] == 0
    p = near(driver, deep, 150, 1_000_000, 1, 1_000_000, 200, sweep=SWEEP_GENERAL)
    assert p["tried"] and p["stretches"] and p["windows"] > 0
    assert not near(driver, shallow, 150, 1_000_000, 1, 1_000_000, 100, spec=-1)["speculate"]
    longer = reads_at(6, 4_000_000, 200, 150)   # (eight run-ins of 1 536 blocks)
    assert not near(driver, longer, 150, 4_000_000, 1, 4_000_000, 200, sweep=SWEEP_GENERAL)["speculate"]
    assert near(driver, longer, 150, 4_000_000, 1, 4_000_000, 200, sweep=SWEEP_GENERAL, spec=1)["speculate"]
    assert near(driver, shallow, 150, 1_000_000, 1, 1_000_000, 100, cuts=-1)["windows"] == 0
    assert near(driver, shallow, 150, 1_000_000, 1, 1_000_000, 100, run_in=700)["burn_blocks"] == 700


# ------------------------------------------------------------------ the mixed-span route
ONE_LENGTH = (4096, 4000, 150)   # a sample of the spans: 98 % of one length
BROAD = (4096, 1000, 150)


def test_mixed_one_dominant_length_on_a_short_contig(driver):
    """7.5 x M, M = 50, one dominant length on a 2 M-position contig: shorter than a dozen run-ins -- no speculation"""
    p = mixed(driver, reads_at(7.5, 2_000_000, 50, 150), 150, 2_000_000, 1, 50, share=ONE_LENGTH)
    assert p["sample"] and p["windows"] > 0 and not p["speculate"]


def test_mixed_one_dominant_length_by_sigma_depth(driver):
    """5c23bbc: the same sample at 3 x M with M = 100 on 60 M positions (sigma depth 4.4): speculated on, with the
    table's whole run-in at that depth"""
    p = mixed(driver, reads_at(3, 60_000_000, 100, 150), 150, 60_000_000, 1, 100, share=ONE_LENGTH)
    assert p["sample"] and p["speculate"] and p["burn_blocks"] == 1536
    assert (p["round_to"], p["run_ins_apart"], p["min_run_ins"]) == (64, 2, 4)


def test_mixed_broad_mix(driver):
    """a broad mix of lengths at 5 x M forgets fast: speculated on, with three fifths of the table's run-in"""
    p = mixed(driver, reads_at(5, 10_000_000, 50, 150), 150, 10_000_000, 1, 50, share=BROAD)
    assert p["sample"] and p["speculate"] and p["burn_blocks"] == 1536 * 3 // 5


def test_mixed_cfg5_share(driver):
    """one GPU's share of configs[4] with longer reads (117.7 M positions, 2 x M, M = 50): speculated on with the full
    run-in (320 blocks, not three fifths of it)"""
    p = mixed(driver, reads_at(2, 117_700_000, 50, 160), 160, 117_700_000, 1, 50, share=ONE_LENGTH)
    assert p["sample"] and p["speculate"] and p["burn_blocks"] == 320


def test_mixed_gates_and_overrides(driver):
    L = 20_000_000
    n = reads_at(2, L, 50, 150)
    # below 2^20 reads no sample is taken: three fifths of the run-in
    p = mixed(driver, 1_000_000, 150, 1_500_000, 1, 50)
    assert not p["sample"] and p["speculate"] and p["burn_blocks"] == 320 * 3 // 5
    # outside the registers (LDS-cached walk) nothing is sampled or speculated on
    p = mixed(driver, n, 150, L, 1, 50, in_regs=0)
    assert not p["sample"] and not p["speculate"]
    # a shape remembered as hopeless: no sample, no speculation -- unless speculation or its run-in is forced
    p = mixed(driver, n, 150, L, 1, 50, hopeless=1)
    assert not p["sample"] and not p["speculate"]
    assert mixed(driver, n, 150, L, 1, 50, hopeless=1, spec=1)["speculate"]
    p = mixed(driver, n, 150, L, 1, 50, hopeless=1, run_in=400)
    assert p["speculate"] and p["burn_blocks"] == 400
    # forced off; cut points forced off (no stretches to speculate on) and on for deep data
    assert not mixed(driver, n, 150, L, 1, 50, share=BROAD, spec=-1)["speculate"]
    p = mixed(driver, n, 150, L, 1, 50, cuts=-1)
    assert p["windows"] == 0 and not p["sample"] and not p["speculate"]
    deep = reads_at(18.75, 8_000_000, 100, 160)
    assert mixed(driver, deep, 160, 8_000_000, 8, 100)["windows"] == 0
    assert mixed(driver, deep, 160, 8_000_000, 8, 100, cuts=1)["windows"] > 0


# ------------------------------------------------------------------ the sweeps' tables and scratch
def sizes(driver, **fields):
    return run(driver, [line("sizes", **fields)])[0]


def test_stretch_table_layout(driver):
    """seg_words is the windows' cuts and then three tables of 1 + 5 (contigs + windows) words: 3 contigs and 128
    windows give 128 + 3 x 656 words, tier t's table begins 128 + 656 t words in; a table of one contig without windows
    is 6 words"""
    assert sizes(driver, contigs=3, windows=128)["words"] == 2096
    assert [sizes(driver, contigs=3, windows=128, tier=t)["offset"] for t in (0, 1, 2)] == [128, 784, 1440]
    assert sizes(driver, contigs=1, windows=0, tier=1)["offset"] == 6
    # the words are where a fourth table would begin; the arena's largest (255 contigs, 3 840 windows)
    assert sizes(driver, contigs=3, windows=128, tier=3)["offset"] == 2096
    assert sizes(driver, contigs=255, windows=3840)["words"] == 3840 + 3 * (1 + 5 * 4095)


def test_event_sweep_scratch(driver):
    """320 000 positions, reads of 150, 771 workgroups: 320 000 / 600 + 771 + 1 pieces of 1 KiB, a checkpoint of 512
    words per 16 pieces and two per workgroup (+ 4), four words per piece (+ 64) of last changed blocks"""
    s = sizes(driver, ltot=320000, ell=150, wg=771)
    assert (s["pieces"], s["pack_bytes"], s["ckpt_bytes"], s["last_bytes"]) == (1305, 1336320, 3332096, 21136)
    # the bound the scratch is sized with: a stretch per contig and per window of the one-span routes (768)
    assert sizes(driver, contigs=3)["ev_wg_max"] == 771
    assert sizes(driver, cand=4096)["snap_bytes"] == 4096 * 512 * 4


# ------------------------------------------------------------------ the multi-device cost model
def test_share_predicate_agrees_with_sharding_py(driver):
    """ADVICE round 4, finding 3: share_sweeps_as_stretches compiled from the header == sharding.py's mirror, on a seeded
    grid of shapes across every regime (below the cut depth, speculated, too deep, too short, too many contigs)"""
    sh = importlib.import_module("genome-downsampler_amd.sharding")
    rng = np.random.default_rng(20261015)
    shapes = []
    for _ in range(3000):
        span = int(rng.choice([0, 1, 31, 100, 150, 151, 250, 256, 400, 512]))
        M = int(rng.choice([0, 1, 10, 20, 50, 100, 200, 400, 1000]))
        positions = int(10 ** rng.uniform(3, 9.3))
        contigs = int(rng.integers(1, 300))
        depth = 10 ** rng.uniform(-0.5, 1.7)
        reads = int(depth * positions * max(M, 1) / max(span, 1))
        shapes.append((reads, positions, contigs, span, M))
    got = run(driver, [line("share", reads=r, positions=p, contigs=c, span=s, M=m) for r, p, c, s, m in shapes])
    want = [sh.share_sweeps_as_stretches(r, p, c, s, m) for r, p, c, s, m in shapes]
    assert sum(want) > 300 and len(want) - sum(want) > 300   # both answers well represented
    bad = [(shape, g["stretches"], w) for shape, g, w in zip(shapes, got, want) if bool(g["stretches"]) != w]
    assert not bad, bad[:10]
