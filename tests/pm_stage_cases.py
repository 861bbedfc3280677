"""The cases of the pass-major stage tests (tests/test_gpu_pm_stages.py; three of them again, on the model alone, in
tests/test_pm_stage_compare_cpu.py).  Each is built from a fixed seed; spans are 30, clipped to the contig, unless said
otherwise.  CASES maps a case's name to a function that builds it (pm_stage_compare.make_case)."""
import zlib

import numpy as np

import pass_major_model as pm
from pm_stage_compare import make_case

PASS = pm.PASS
RAGGED = [70_001, 33_333, 250_000, 1_000]
RAGGED_READS = [9_000, 11_011, 30_000, 5]


def _seed(name):
    return zlib.crc32(name.encode()) & 0xFFFF


def _spans(starts, lengths, contig, span):
    """ends of reads of one span, clipped to the contig"""
    last = np.maximum(np.asarray(lengths, np.int64) - 1, 0)
    return np.minimum(np.asarray(starts, np.int64) + span - 1, last[contig])


def _uniform(name, lengths, counts, wish=-1, span=30, expect_aligned=None):
    def build():
        rng = np.random.default_rng(_seed(name))
        contig = np.repeat(np.arange(len(lengths)), counts)
        starts = np.concatenate([rng.integers(0, max(int(L), 1), size=int(k)) for L, k in zip(lengths, counts)])
        return make_case(name, lengths, counts, starts, _spans(starts, lengths, contig, span), wish=wish,
                         expect_aligned=expect_aligned, seed=_seed(name))
    return build


def _distribution(name, kind, lengths, counts, wish, expect_aligned):
    def build():
        rng = np.random.default_rng(_seed(name))
        lens = np.asarray(lengths, np.int64)
        poff = np.concatenate([[0], np.cumsum(lens)])
        shift = pm.range_shift_for(int(poff[-1]))
        width = 1 << shift
        contig = np.repeat(np.arange(len(lengths)), counts)
        parts = []
        for c, (L, k) in enumerate(zip(lengths, counts)):
            L, k = int(L), int(k)
            if kind == "sorted":        # a pass falls into one or two ranges, slices thousands of records long
                s = np.sort(rng.integers(0, L, size=k))
            elif kind == "one_position":
                s = np.full(k, L // 3)
            elif kind == "five_positions":   # 70 % of the reads on five positions
                hot = rng.integers(0, L, size=5)
                s = np.where(rng.random(k) < 0.7, hot[rng.integers(0, 5, size=k)], rng.integers(0, L, size=k))
            elif kind == "range_edges":      # keys 0 and 2^shift - 1 of every range of the genome's own axis
                g = np.arange(poff[c], poff[c] + L)
                edge = g[((g & (width - 1)) == 0) | ((g & (width - 1)) == width - 1)] - poff[c]
                s = edge[rng.integers(0, edge.size, size=k)]
            elif kind == "last_start":       # each contig's last valid start
                s = np.full(k, L - 1)
            else:
                raise ValueError(kind)
            parts.append(s)
        starts = np.concatenate(parts)
        span = 150 if kind == "sorted" else (100 if kind == "five_positions" else 30)
        return make_case(name, lengths, counts, starts, _spans(starts, lengths, contig, span), wish=wish,
                         expect_aligned=expect_aligned, seed=_seed(name))
    return build


INVALID_N = 3 * PASS + 77
INVALID_READS = [9_000, 8_000, INVALID_N - 17_005, 5]        # pass 1 holds contigs 0 and 1; the last pass is partial
INVALID_AT = {"first_pass": 100, "last_pass": 3 * PASS + 10, "two_contig_pass": 9_500}


def _invalid(name, variant, place, wish):
    def build():
        rng = np.random.default_rng(_seed(name))
        contig = np.repeat(np.arange(4), INVALID_READS)
        lens = np.asarray(RAGGED, np.int64)
        starts = np.concatenate([rng.integers(0, L - 30, size=k) for L, k in zip(RAGGED, INVALID_READS)])
        ends = starts + 29
        i = INVALID_AT[place]
        L = int(lens[contig[i]])
        if variant == "start_beyond":        # taken as the contig's last position
            starts[i], ends[i] = 4_000_000_000, 4_000_000_029
        elif variant == "start_after_end":
            starts[i], ends[i] = ends[i], starts[i]
        elif variant == "end_at_length":
            starts[i], ends[i] = L - 30, L
        else:
            raise ValueError(variant)
        return make_case(name, RAGGED, INVALID_READS, starts, ends, wish=wish, stop_after="C", expect_bad=1,
                         expect_aligned=1 if wish > 0 else 0, seed=_seed(name))
    return build


FILTER_N = 5 * PASS + 1


def _filter(name, kind):
    def build():
        rng = np.random.default_rng(_seed(name))
        L, n = 60_000, FILTER_N
        starts = rng.integers(0, L - 150, size=n)
        ends = starts + 149
        if kind == "one_percent":            # clipped at the front or at the back
            pick = rng.random(n) < 0.01
            clip = rng.integers(1, 40, size=n)
            front = rng.random(n) < 0.5
            starts = np.where(pick & front, starts + clip, starts)
            ends = np.where(pick & ~front, ends - clip, ends)
        elif kind == "run":                  # 3 000 neighbours: three waves overflow their 128 slots
            ends[10_000:13_000] -= rng.integers(1, 40, size=3_000)
        elif kind == "all":                  # the only span is not ell_reg: empty slices and tables
            ends = starts + 99
        elif kind != "none":
            raise ValueError(kind)
        return make_case(name, [L], [n], starts, ends, ell_reg=150, seed=_seed(name))
    return build


def _cases():
    cases = {}
    for n in (1, 63, 64, 65, 1023, 1024, 1025, PASS - 1, PASS, PASS + 1, 4 * PASS, 4 * PASS + 1, 9 * PASS + 5, 19 * PASS + 5):
        name = "size_%d" % n
        cases[name] = _uniform(name, [100_000], [n])
    for tag, lengths, counts in (("one_position", [1], [20_000]), ("g255", [255], [20_000]), ("g256", [256], [20_000]), ("g300", [300], [20_000]),
                                 ("sparse_2e21", [(1 << 21) - 5], [40_000]), ("widest_2e23", [(1 << 23) - 1], [20_000])):
        cases["genome_" + tag] = _uniform("genome_" + tag, lengths, counts)
    for wish, grid in ((-1, "global"), (1, "aligned")):
        al = 1 if wish > 0 else 0
        for tag, lengths, counts, fits in (("whole_ranges", [4096, 8192, 2048], [9_000, 20_011, 5_000], True),
                                           ("ragged", RAGGED, [9_000, 20_011, 30_000, 5], True),
                                           ("empty_contigs", [5_000, 0, 50_000, 5_000], [0, 0, 25_000, 0], True),
                                           ("sixty_contigs", [1090] * 60, [400] * 60, False)):   # 300 aligned ranges: the plan keeps the global grid
            name = "genome_%s_%s" % (tag, grid)
            cases[name] = _uniform(name, lengths, counts, wish=wish, expect_aligned=al if fits else 0)
        for kind in ("sorted", "one_position", "five_positions", "range_edges", "last_start"):
            name = "dist_%s_ragged_%s" % (kind, grid)
            cases[name] = _distribution(name, kind, RAGGED, RAGGED_READS, wish, al)
        for variant in ("start_beyond", "start_after_end", "end_at_length"):
            for place in INVALID_AT:
                name = "invalid_%s_%s_%s" % (variant, place, grid)
                cases[name] = _invalid(name, variant, place, wish)
    for kind in ("sorted", "one_position", "five_positions", "range_edges", "last_start"):
        name = "dist_%s_single" % kind
        cases[name] = _distribution(name, kind, [40_000], [50_000], -1, 0)
    for kind in ("none", "one_percent", "run", "all"):
        cases["filter_" + kind] = _filter("filter_" + kind, kind)
    return cases


CASES = _cases()
