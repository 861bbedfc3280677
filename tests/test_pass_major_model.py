"""CPU model of the pass-major layout (tests/pass_major_model.py, round 4 form: slices padded to whole groups of 64
slots, one descriptor word per wave-slot): the producer's slots and tables, the scanned table,
the descriptors, the three consumers -- every index in bounds, every range's records recovered in
read-index order, and the keep mask of walk + settle equal to "the S(p) lowest read indices of every start
position p" for random quotas -- on ragged inputs (last pass partial, ranges straddling contig borders, empty ranges
and empty slices, one range holding everything, slices of a few records)."""
import numpy as np
import pytest

import pass_major_model as pm


def _case(rng, lengths, counts, shift, skew=None):
    lengths = np.asarray(lengths, np.int64)
    counts = np.asarray(counts, np.int64)
    poff = np.concatenate([[0], np.cumsum(lengths)])
    roff = np.concatenate([[0], np.cumsum(counts)])
    gs = []
    for c, (L, k) in enumerate(zip(lengths, counts)):
        if skew is not None:
            s = skew(rng, int(k), int(L))
        else:
            s = rng.integers(0, max(int(L), 1), size=int(k))
        gs.append(poff[c] + np.minimum(s, max(int(L) - 1, 0)))
    return np.concatenate(gs).astype(np.uint32), roff, poff, int(poff[-1])


CASES = [
    # lengths, counts, shift
    ([100_000], [3 * 8192 + 77], 9),                                   # one contig, last pass partial
    ([70_001, 33_333, 250_000, 1_000], [9_000, 20_011, 30_000, 5], 11),  # ranges straddle contig borders
    ([5_000, 5_000, 5_000], [0, 25_000, 0], 6),                         # contigs without reads
    ([300], [20_000], 3),                                               # tiny genome, 38 ranges
    ([40_000], [17_000], 15),                                           # ONE range holds everything
    ([(1 << 21) - 5], [40_000], 13),                                    # 256 ranges, sparse: slices of a few records
]


_expected_mask = pm.expected_mask     # (shared with the stage tests: tests/pm_stage_compare.py)


@pytest.mark.parametrize("lengths,counts,shift", CASES)
def test_layout_round_trip_bounds_and_mask(lengths, counts, shift):
    rng = np.random.default_rng(len(lengths) * 1000 + shift)
    gs, roff, poff, ltot = _case(rng, lengths, counts, shift)
    n = gs.size
    n_ranges = (ltot >> shift) + 1
    assert n_ranges <= 256
    keys16, idx16, cntp, lstw = pm.producer(gs, shift, n_ranges)
    pitch = pm.pitch_for(n)
    stride = pm.stride_for(n_ranges)
    Tp = pm.scan_table(cntp)
    assert Tp.size == 256 * pitch + 1 and int(Tp[-1]) % 64 == 0 and int(Tp[-1]) >= n
    desc, range_start = pm.descriptors(Tp, lstw, n, n_ranges)
    assert int(range_start[-1]) == n
    # random quotas: 0, 1, a few, everything
    width = 1 << shift
    quota = rng.choice([0, 0, 1, 1, 2, 5, 1 << 20], size=ltot + width)
    seen = np.zeros(n, bool)
    mask = np.zeros(n, bool)
    kept_total = 0
    amb_all = {}
    for d in range(n_ranges):
        g0, n_ws = pm.range_wave_slots(Tp, pitch, d)
        true_count = int(range_start[d + 1]) - int(range_start[d])
        if n_ws == 0:
            assert true_count == 0
            continue
        # every record of the range, in read-index order, through the descriptors
        reads = []
        for ws in range(n_ws):
            slot0, nv, P = pm.unpack(desc[g0 + ws], stride)
            assert slot0 + nv <= pitch * stride and slot0 // stride == P
            r = P * pm.PASS + idx16[slot0:slot0 + nv].astype(np.int64)
            assert idx16[slot0:slot0 + nv].max() < pm.PASS
            reads.append(r)
        reads = np.concatenate(reads)
        assert reads.size == true_count and reads.max() < n and np.all(np.diff(reads) > 0)
        assert np.all((gs[reads] >> shift) == d)
        assert not seen[reads].any()
        seen[reads] = True
        # bucket counts
        hist = pm.offsets(keys16, desc, Tp, pitch, d, shift, stride)
        assert np.array_equal(hist, np.bincount((gs[reads] & (width - 1)).astype(np.int64), minlength=width))
        # walk (settled below)
        amb, kept = pm.walk(keys16, idx16, desc, Tp, pitch, d, quota[d * width:(d + 1) * width], stride, n, mask, rng)
        kept_total += kept
        amb_all[d] = amb
    assert seen.all()
    for d, amb in amb_all.items():
        kept_total += pm.settle(amb, keys16, idx16, desc, Tp, pitch, d, n, stride, mask)
    want = _expected_mask(gs, lambda p: quota[p])
    assert np.array_equal(mask, want) and kept_total == int(want.sum())


def test_skewed_passes_with_long_and_empty_slices():
    """reads sorted by position inside the contig: a pass's records fall into one or two ranges (slices of
    thousands of records, most slices empty); quotas that run out inside chunks"""
    rng = np.random.default_rng(2)
    gs, roff, poff, ltot = _case(rng, [200_000], [5 * 8192 + 1], 10,
                                 skew=lambda r, k, L: np.sort(r.integers(0, L // 50, size=k) * 50))
    n = gs.size
    n_ranges = (ltot >> 10) + 1
    keys16, idx16, cntp, lstw = pm.producer(gs, 10, n_ranges)
    pitch = pm.pitch_for(n)
    Tp = pm.scan_table(cntp)
    desc, range_start = pm.descriptors(Tp, lstw, n, n_ranges)
    stride = pm.stride_for(n_ranges)
    quota = rng.integers(0, 12, size=ltot + 1024)
    mask = np.zeros(n, bool)
    ambs = {}
    for d in range(n_ranges):
        g0, n_ws = pm.range_wave_slots(Tp, pitch, d)
        if n_ws == 0:
            continue
        ambs[d], _ = pm.walk(keys16, idx16, desc, Tp, pitch, d, quota[d * 1024:(d + 1) * 1024], stride, n, mask, rng)
    assert sum(len(a) for a in ambs.values()) > 0        # the case is meant to produce quota-crossing groups
    for d, amb in ambs.items():
        pm.settle(amb, keys16, idx16, desc, Tp, pitch, d, n, stride, mask)
    assert np.array_equal(mask, _expected_mask(gs, lambda p: quota[p]))


# ---- what the kernels write besides the layout: the model's functions against brute-force loops
def _ragged_reads(rng, ell):
    lengths = np.array([3_000, 0, 700, 9_000], np.int64)
    counts = np.array([2 * 8192 + 300, 0, 1_500, 8192 - 11], np.int64)
    contig = np.repeat(np.arange(4), counts)
    starts = np.concatenate([rng.integers(0, max(int(L) - ell, 1), size=int(k)) for L, k in zip(lengths, counts)])
    return lengths, counts, contig, starts, starts + ell - 1


def test_exception_lists_against_a_loop():
    """every (pass, wave of 1 024 reads) lists its first 128 exceptions in read-index order; the rest overflow"""
    rng = np.random.default_rng(11)
    ell = 50
    lengths, counts, contig, starts, ends = _ragged_reads(rng, ell)
    n = starts.size
    ends = ends.copy()
    clipped = rng.random(n) < 0.03
    clipped[5_000:5_700] = True                      # a run: waves 4 and 5 overflow their slots
    ends[clipped] -= rng.integers(1, 20, size=int(clipped.sum()))
    starts[17] = 4_000_000_000                       # an invalid read is an exception like any other, clamped
    ends[17] = 4_000_000_020
    ends[18] = lengths[0] + 5
    poff = np.concatenate([[0], np.cumsum(lengths)])
    gs = poff[contig] + pm.clamped(starts, contig, lengths)
    ge = poff[contig] + pm.clamped(ends, contig, lengths)
    regular = pm.regular_reads(starts, ends, ell)
    cnt, groups, overflow = pm.exception_lists(gs, ge, regular)
    want_cnt = [0] * (pm.pitch_for(n) * 8)
    want_groups, want_over = {}, []
    for i in range(n):
        span = (int(ends[i]) - int(starts[i]) + 1) % (1 << 32)
        assert bool(regular[i]) == (span == ell)
        if span == ell:
            continue
        last = max(int(lengths[contig[i]]) - 1, 0)
        ent = (int(poff[contig[i]]) + min(int(starts[i]), last), int(poff[contig[i]]) + min(int(ends[i]), last), i)
        g = 8 * (i // pm.PASS) + (i % pm.PASS) // 1024
        if want_cnt[g] < 128:
            want_groups.setdefault(g, []).append(ent)
            want_cnt[g] += 1
        else:
            want_over.append(ent)
    assert not regular[17] and not regular[18] and len(want_over) > 0 and max(want_cnt) == 128
    assert cnt.tolist() == want_cnt and sorted(groups) == sorted(want_groups)
    for g, ent in want_groups.items():
        assert groups[g].tolist() == [list(e) for e in ent]
    assert sorted(map(tuple, overflow.tolist())) == sorted(want_over)
    # the filtered producer: only the regular reads enter the slices, under their index inside the pass
    keys16, idx16, cntp, lstw = pm.producer(gs.astype(np.uint32), 6, (int(poff[-1]) >> 6) + 1, regular)
    assert int((lstw >> 16).sum()) == int(regular.sum())
    stride = pm.stride_for((int(poff[-1]) >> 6) + 1)
    seen = []
    for d, P in zip(*np.nonzero(lstw >> 16)):
        at = int(P) * stride + int(lstw[d, P] & 0xFFFF) * 64
        seen.append(int(P) * pm.PASS + idx16[at:at + int(lstw[d, P] >> 16)].astype(np.int64))
    assert np.array_equal(np.sort(np.concatenate(seen)), np.nonzero(regular)[0])


def test_statistics_and_plain_references_against_loops():
    rng = np.random.default_rng(12)
    lengths, counts, contig, starts, ends = _ragged_reads(rng, 30)
    n = starts.size
    for variant in range(4):
        s, e = starts.copy(), ends.copy()
        if variant == 1:
            s[n - 3], e[n - 3] = 4_000_000_000, 4_000_000_029      # a start beyond its contig
        elif variant == 2:
            s[9_000], e[9_000] = e[9_000], s[9_000]                  # start > end: the span wraps, as in the kernel
        elif variant == 3:
            e[40] = lengths[contig[40]]                              # an end at the contig's length
            s[40] = e[40] - 29
        mn, mx, bad = 1 << 32, 0, 0
        for i in range(n):
            span = (int(e[i]) - int(s[i]) + 1) % (1 << 32)
            mn, mx = min(mn, span), max(mx, span)
            bad |= int(s[i] > e[i] or e[i] >= lengths[contig[i]])
        assert pm.statistics(s, e, contig, lengths) == (mn, mx, bad) and bad == (variant != 0)
        assert np.array_equal(pm.clamped(s, contig, lengths),
                              [min(int(v), max(int(lengths[c]) - 1, 0)) for v, c in zip(s, contig)])
    # bucket offsets, empty positions, loads
    poff = np.concatenate([[0], np.cumsum(lengths)])
    ltot = int(poff[-1])
    gs = (poff[contig] + starts).astype(np.int64)
    count = [0] * ltot
    for v in gs:
        count[int(v)] += 1
    boff = [0]
    for p in range(ltot):
        boff.append(boff[-1] + count[p])
    assert pm.bucket_offsets(gs, ltot).tolist() == boff
    assert pm.empty_positions(gs, ltot) == sum(1 for c in count if c == 0)
    n_ranges = (ltot >> 6) + 1
    _, _, cntp, lstw = pm.producer(gs.astype(np.uint32), 6, n_ranges)
    rows_true = [0] * 256
    rows_slots = [0] * 256
    for P in range((n + pm.PASS - 1) // pm.PASS):
        per = [0] * 256
        for v in gs[P * pm.PASS:(P + 1) * pm.PASS]:
            per[int(v) >> 6] += 1
        for d in range(256):
            rows_true[d] += per[d]
            rows_slots[d] += (per[d] + 63) // 64
    assert pm.loads(cntp, lstw) == (max(rows_true), max(rows_slots))
    assert [pm.range_shift_for(v) for v in (1, 255, 256, 300, 14_336, 100_000, (1 << 21) - 5, (1 << 23) - 1)] == [0, 0, 1, 1, 6, 9, 13, 15]
