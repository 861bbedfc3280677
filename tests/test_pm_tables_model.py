"""The pass-major table stage in two launches (csrc/kernels/pass_major.inc.hip: k_pm_row_sums, k_pm_tables), restated in
numpy the way the kernels partition it -- a row of the [range][pass] tables cut into Y parts, one workgroup per (range,
part): partial sums of the padded and the true counts, then every workgroup's own prefix over all 256 x Y partial pairs,
the scan of its part in absolute padded flat coordinates, the descriptors of its entries, and from workgroup (0, 0) the
ranges' true flat starts, the heaviest load and the grand total -- and asserted EQUAL to what tests/pass_major_model.py
computes for the same tables with one scan over the flattened table (scan_table) and one pass over its entries
(descriptors).  32-bit arithmetic throughout, as on the device."""
import numpy as np
import pytest

import pass_major_model as pm

Y = 8  # kPmDescrY


def row_part(pitch, y):
    per = (pitch + Y - 1) // Y
    return min(pitch, y * per), min(pitch, (y + 1) * per)


def row_sums(cntp, lstw):
    """k_pm_row_sums: work[d][y] = (padded records, true records) of part y of row d"""
    pitch = cntp.shape[1]
    work = np.zeros((256, Y, 2), np.uint32)
    for y in range(Y):
        a, b = row_part(pitch, y)
        work[:, y, 0] = cntp[:, a:b].sum(axis=1, dtype=np.uint32)
        work[:, y, 1] = (lstw[:, a:b] >> 16).sum(axis=1, dtype=np.uint32)
    return work


def tables(cntp, lstw, work, n_groups):
    """k_pm_tables, workgroup by workgroup -> Tp [256 pitch + 1], desc [n_groups], range_start [257], max_load"""
    pitch = cntp.shape[1]
    Tp = np.full(256 * pitch + 1, 0xFFFFFFFF, np.uint32)
    desc = np.full(n_groups, 0xFFFFFFFF, np.uint32)
    range_start = max_load = None
    for d in range(256):
        for y in range(Y):
            # thread t: row t's totals and the padded total of its parts before y
            rp = work[:, :, 0].sum(axis=1, dtype=np.uint32)
            rt = work[:, :, 1].sum(axis=1, dtype=np.uint32)
            before = work[:, :y, 0].sum(axis=1, dtype=np.uint32)
            excl = (np.cumsum(rp, dtype=np.uint32) - rp).astype(np.uint32)
            carry = np.uint32(excl[d] + before[d])
            if d == 0 and y == 0:
                Tp[256 * pitch] = np.uint32(excl[255] + rp[255])
                range_start = np.concatenate([[0], np.cumsum(rt, dtype=np.uint32)]).astype(np.uint32)
                max_load = int(rt.max())
            a, b = row_part(pitch, y)
            for P0 in range(a, b, 1024):           # a round: four tiles of 256 entries
                for u in range(4):
                    lo, hi = min(b, P0 + 256 * u), min(b, P0 + 256 * (u + 1))
                    c = cntp[d, lo:hi]
                    t = (carry + np.cumsum(c, dtype=np.uint32) - c).astype(np.uint32)
                    assert (Tp[d * pitch + lo:d * pitch + hi] == 0xFFFFFFFF).all()   # written once
                    Tp[d * pitch + lo:d * pitch + hi] = t
                    carry = np.uint32(carry + c.sum(dtype=np.uint32))
                    if not (lstw[d, lo:hi] >> 16).any():
                        continue
                    for P, tt, w in zip(range(lo, hi), t, lstw[d, lo:hi]):
                        cnt, lst64 = int(w) >> 16, int(w) & 0xFFFF
                        g = int(tt) >> 6
                        for j in range((cnt + 63) >> 6):
                            assert g + j < n_groups and desc[g + j] == 0xFFFFFFFF
                            desc[g + j] = (P << 15) | ((lst64 + j) << 6) | (min(64, cnt - 64 * j) - 1)
    return Tp, desc, range_start, max_load


def make_tables(counts):
    """true counts [256][pitch] -> cntp, lstw as the producer writes them (a pass's slices follow each other padded)"""
    counts = np.asarray(counts, np.int64)
    assert counts.shape[0] == 256 and counts.shape[1] % 4 == 0 and counts.sum(axis=0).max() <= pm.PASS
    pad = (counts + 63) // 64 * 64
    first = np.cumsum(pad, axis=0) - pad
    return pad.astype(np.uint32), ((first // 64) | (counts << 16)).astype(np.uint32)


def check(counts, empty_tail_passes=0):
    cntp, lstw = make_tables(counts)
    pitch = cntp.shape[1]
    n = (pitch - empty_tail_passes) * pm.PASS
    assert pm.pitch_for(n) == pitch
    want_Tp = pm.scan_table(cntp)
    n_ranges = 256
    want_desc, want_rs = pm.descriptors(want_Tp, lstw, n, n_ranges)
    n_groups = pitch * (pm.stride_for(n_ranges) // 64)    # the buffer's bound, as the launcher passes it
    Tp, desc, rs, max_load = tables(cntp, lstw, row_sums(cntp, lstw), n_groups)
    assert np.array_equal(Tp, want_Tp)
    G = int(want_Tp[-1]) // 64
    assert G <= n_groups and np.array_equal(desc[:G], want_desc) and (desc[G:] == 0xFFFFFFFF).all()
    assert np.array_equal(rs, want_rs)
    assert max_load == int(np.diff(want_rs.astype(np.int64)).max())


def _ragged(rng, pitch, rows, per_entry):
    counts = np.zeros((256, pitch), np.int64)
    for P in range(pitch):
        left = pm.PASS
        for d in rng.permutation(rows):
            c = min(int(per_entry(rng)), left)
            counts[d, P] = c
            left -= c
    return counts


@pytest.mark.parametrize("pitch", [4, 16, 20])   # Y = 8: parts of 1, 2 and 3 entries -- at 4 and 20 some parts are empty
def test_ragged_tables(pitch):
    rng = np.random.default_rng(pitch)
    # rows of zeros between the others; counts of 1, multiples of 64, and anything else
    rows = np.array([0, 1, 2, 7, 63, 64, 100, 200, 254, 255])
    pick = lambda r: r.choice([0, 1, 1, 63, 64, 65, 128, 640, int(r.integers(0, 900))])
    check(_ragged(rng, pitch, rows, pick))
    # the last passes beyond the reads: zero entries the scan still runs over
    counts = _ragged(rng, pitch, rows, pick)
    counts[:, pitch - 3:] = 0
    check(counts, empty_tail_passes=3)


def test_single_non_empty_row():
    for row in (0, 129, 255):
        counts = np.zeros((256, 16), np.int64)
        counts[row, :] = [pm.PASS, 1, 64, 0, 8191, 65, 0, 0, 4096, 63, 1, 1, 0, 128, 8192, 5]
        check(counts)


def test_all_256_rows():
    rng = np.random.default_rng(256)
    check(_ragged(rng, 20, np.arange(256), lambda r: r.choice([0, 1, 31, 32, 64])))
    counts = np.full((256, 4), 32, np.int64)     # every slice half a group: the padding doubles the flat space
    check(counts)
    counts = np.ones((256, 16), np.int64)        # entries of 1
    check(counts)


def test_more_than_one_round_per_part():
    """a part longer than a round of 1 024 entries (and than one tile of 256): the carry between tiles and rounds"""
    pitch = 8 * 1300
    rng = np.random.default_rng(5)
    counts = np.zeros((256, pitch), np.int64)
    counts[3, :] = rng.choice([0, 1, 64, 100], size=pitch)
    counts[200, :] = rng.choice([0, 0, 0, 7], size=pitch)
    cntp, lstw = make_tables(counts)
    want_Tp = pm.scan_table(cntp)
    n_groups = pitch * (pm.stride_for(256) // 64)
    # (the descriptors of this size through the model's python loop are slow: the scan, the true starts and the load only)
    lstw_no_desc = lstw & np.uint32(0xFFFF)
    Tp, _, _, _ = tables(cntp, lstw_no_desc, row_sums(cntp, lstw), n_groups)
    assert np.array_equal(Tp, want_Tp)
    work = row_sums(cntp, lstw)
    assert np.array_equal(work[:, :, 1].sum(axis=1), counts.sum(axis=1))
