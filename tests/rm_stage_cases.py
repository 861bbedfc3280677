"""The cases of the range-major stage tests (tests/test_gpu_rm_stages.py; every one below 2 M positions again, on the
model alone, in tests/test_range_major_model.py).  Each is built from a fixed seed; spans are 30, clipped to the contig,
unless said otherwise.  CASES maps a case's name to a function that builds it (rm_stage_compare.make_case)."""
import zlib

import numpy as np

import pm_stage_cases as pmc
import range_major_model as rm
from rm_stage_compare import adopt, make_case

TILE, PASS = rm.TILE, rm.PASS
ONE_CONTIG = 300_000                 # shift 11: 147 ranges of 2 048 positions


def _seed(name):
    return zlib.crc32(name.encode()) & 0xFFFF


def _ends(starts, lengths, contig, span=30):
    last = np.maximum(np.asarray(lengths, np.int64) - 1, 0)
    return np.minimum(np.asarray(starts, np.int64) + span - 1, last[contig])


def _uniform(name, lengths, counts, reads_of=None, **kw):
    """reads spread evenly over every contig that has positions (reads_of: the name whose seed draws them)"""
    def build():
        rng = np.random.default_rng(_seed(reads_of or name))
        contig = np.repeat(np.arange(len(lengths)), counts)
        starts = np.concatenate([rng.integers(0, max(int(L), 1), size=int(k)) for L, k in zip(lengths, counts)])
        return make_case(name, lengths, counts, starts, _ends(starts, lengths, contig), seed=_seed(name), **kw)
    return build


def _one_range(name, n):
    """every read inside range 3 of the one contig: the ranking's chunks of 1 024 records fill, and wrap, its ring of eight"""
    def build():
        rng = np.random.default_rng(_seed(name))
        starts = rng.integers(3 * 2048, 4 * 2048, size=n)
        return make_case(name, [ONE_CONTIG], [n], starts, starts + 29, seed=_seed(name))
    return build


def _spread(n, k):
    counts = np.full(k, n // k, np.int64)
    counts[:n % k] += 1
    return counts


def _contigs(name, k):
    def build():
        rng = np.random.default_rng(_seed(name))
        lengths = rng.integers(500, 3001, size=k)
        return _uniform(name, lengths, _spread(20_000, k))()
    return build


def _digit_span(name, k):
    """contig 1's reads are one whole pass, and its positions begin in range 10 and end in range 10 + k - 1 of 256-wide
    ranges: the pass's digits span k ranges"""
    a = 10 * 256
    b = a + (k - 1) * 256 + 128
    return _uniform(name, [a, b - a, 65_535 - b], [PASS, PASS, 20_000 - 2 * PASS])


def _heavy(name, records, below):
    """range 5 of the one contig holds `records` reads, the range below it `below` (the heavy range's first record is
    then record `below` of the stream), range 9 the rest of ten"""
    def build():
        rng = np.random.default_rng(_seed(name))
        starts = np.concatenate([rng.integers(5 * 2048, 6 * 2048, size=records), rng.integers(4 * 2048, 5 * 2048, size=below),
                                 rng.integers(9 * 2048, 10 * 2048, size=10 - below)])
        starts = starts[rng.permutation(starts.size)]
        return make_case(name, [ONE_CONTIG], [starts.size], starts, starts + 29, seed=_seed(name))
    return build


DIST_READS = [9_000, 11_011, 4_637, 5]           # 3 x 8 192 + 77 over the ragged contigs of the pass-major cases


def _distribution(name, kind):
    def build():
        return adopt(pmc._distribution(name, kind, pmc.RAGGED, DIST_READS, -1, None)(), stop_after="E")
    return build


def _invalid(name, variant, place):
    def build():
        return adopt(pmc._invalid(name, variant, place, -1)(), stop_after="D")
    return build


FILTER_READS = [TILE + 2_000, 2 * TILE - 1_000]   # tile 0 whole in contig 0, tile 1 in both, tile 2 whole in contig 1, tile 3 partial
FILTER_N = sum(FILTER_READS)


def _wave_reads(tile, wave, n):
    """the reads of a tile one wave of k_prepare takes: j = 256 k + 64 wave + lane"""
    j = (np.arange(16)[:, None] * 256 + 64 * wave + np.arange(64)[None, :]).reshape(-1)
    i = tile * TILE + j
    return i[i < n]


def _filter(name, kind, two_level):
    def build():
        rng = np.random.default_rng(_seed(name))
        lengths = [9_000_000 if two_level else 200_000, 100_000]
        counts = [5_000, 8_192 + 5 - 5_000] if kind == "all" else FILTER_READS
        n = sum(counts)
        contig = np.repeat(np.arange(2), counts)
        starts = np.concatenate([rng.integers(0, L - 64, size=k) for L, k in zip(lengths, counts)])
        other = np.zeros(n, bool)
        if kind == "three":
            other[[5, TILE + 2_500, n - 1]] = True
        elif kind == "run":
            other[5_000:8_000] = True
        elif kind == "all":
            other[:] = True
        elif kind != "none":
            where, count = kind.split("_")
            tile = {"lean": 2, "partial": 3, "twocontig": 1}[where]
            reads = _wave_reads(tile, 1, n)
            other[rng.choice(reads, size=int(count), replace=False)] = True
        span = np.where(other, rng.choice([17, 29, 31, 45], size=n), 30)
        return make_case(name, lengths, counts, starts, starts + span - 1, ell_reg=30, seed=_seed(name),
                         n_quota=3 if two_level else 6)
    return build


def _two_level_clustered(name):
    """40 M positions, all but 200 of 20 000 reads inside one stretch of 400 000: most super-ranges hold nothing"""
    def build():
        rng = np.random.default_rng(_seed(name))
        L = 40_000_000
        starts = np.concatenate([rng.integers(17_000_000, 17_400_000, size=19_800), rng.integers(0, L - 30, size=200)])
        starts = starts[rng.permutation(starts.size)]
        return make_case(name, [L], [starts.size], starts, starts + 29, seed=_seed(name), n_quota=3)
    return build


def _cases():
    cases = {}
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 9 * 1024 + 5, 16 * 1024 + 3, 3 * PASS + 77, 4 * PASS):
        cases["size_%d" % n] = _uniform("size_%d" % n, [ONE_CONTIG], [n])
    for n in (8 * 1024 - 1, 8 * 1024 + 1, 9 * 1024 + 5):
        cases["size_%d_one_range" % n] = _one_range("size_%d_one_range" % n, n)
    for n in (8 * TILE + 5, 16 * TILE):
        for tpb in (0, 2, 4, 6, 8):
            name = "tiles_per_block_%d_n%d" % (tpb, n)
            # (one input per n: every width must leave what the library's own choice, "0", leaves -- all are held
            #  against one model)
            cases[name] = _uniform(name, [ONE_CONTIG], [n], reads_of="tiles_per_block_n%d" % n, tiles_per_block=tpb, stop_after="A")
    cases["tiles_per_block_8_n%d" % (9 * TILE)] = _uniform("tiles_per_block_8_n%d" % (9 * TILE), [ONE_CONTIG], [9 * TILE],
                                                            tiles_per_block=8, stop_after="A")
    for tag, length in (("1", 1), ("255", 255), ("256", 256), ("300", 300), ("511x256", 511 * 256), ("1023x256", 1023 * 256), ("1024x256", 1024 * 256),
                        ("2e21m5", (1 << 21) - 5), ("2e23m1", (1 << 23) - 1)):
        cases["genome_" + tag] = _uniform("genome_" + tag, [length], [5_000])
    # a genome whose positions are as many as its reads: the ranking's list fits its buffer by positions and by records
    cases["genome_4095_both_lists"] = _uniform("genome_4095_both_lists", [4095], [4096])
    cases["two_level_2e23"] = _uniform("two_level_2e23", [1 << 23], [20_000], n_quota=3)
    cases["two_level_2e23p5"] = _uniform("two_level_2e23p5", [(1 << 23) + 5], [20_000], n_quota=3)
    cases["two_level_four_contigs"] = _uniform("two_level_four_contigs", [9_000_001, 5_000_000, 8_388_608 + 5, 123],
                                               [9_000, 4_800, 8_500, 0], n_quota=3)
    cases["two_level_clustered_40m"] = _two_level_clustered("two_level_clustered_40m")
    cases["two_level_one_read"] = _uniform("two_level_one_read", [(1 << 23) + 5], [1], n_quota=3)
    for k in (1, 2, 63, 64, 65, 200):
        cases["contigs_%d" % k] = _contigs("contigs_%d" % k, k)
    cases["contigs_whole_ranges"] = _uniform("contigs_whole_ranges", [4096, 8192, 2048], [6_000, 10_000, 4_000])
    cases["contigs_no_positions_between"] = _uniform("contigs_no_positions_between", [5_000, 0, 7_000], [10_000, 0, 10_000])
    cases["contigs_no_reads"] = _uniform("contigs_no_reads", [3_000, 4_000, 2_500, 5_000, 1_500], [0, 8_000, 0, 12_000, 0])
    cases["contigs_five_in_a_pass"] = _uniform("contigs_five_in_a_pass", [3_000, 700, 900, 800, 2_000, 2_500],
                                               [7_000, 300, 300, 300, 300, 11_800])
    for k in (1, 2, 3, 5, 9, 17, 33, 65, 129):
        cases["digit_span_%d" % k] = _digit_span("digit_span_%d" % k, k)
    for kind in ("sorted", "one_position", "five_positions", "range_edges", "last_start"):
        cases["dist_" + kind] = _distribution("dist_" + kind, kind)
    for below in range(4):
        cases["heavy_first_record_%d" % below] = _heavy("heavy_first_record_%d" % below, 3 * PASS + 77 - 10, below)
    for records in (32_767, 32_768, 32_769, 4 * 32_768 + 2):
        cases["heavy_%d" % records] = _heavy("heavy_%d" % records, records, 1)
    for variant in ("start_beyond", "start_after_end", "end_at_length"):
        for place in pmc.INVALID_AT:
            cases["invalid_%s_%s" % (variant, place)] = _invalid("invalid_%s_%s" % (variant, place), variant, place)
    for two_level in (False, True):
        for kind in ("none", "three", "lean_128", "lean_129", "partial_128", "partial_129", "twocontig_128", "twocontig_129", "run", "all"):
            name = "filter_%s_%s" % (kind, "two_level" if two_level else "one_level")
            cases[name] = _filter(name, kind, two_level)
    return cases


CASES = _cases()
