"""Host restatement of the pass-major producer's flat write-out (k_pm_prepare_sort, csrc/kernels/pass_major.inc.hip):
where a pass's digits span at most 32 ranges, the pass is staged in LDS in the padded layout it has in memory -- a
record's stage slot is its slice's padded base inside the pass plus its stable rank inside the slice -- and the stage's
words [0, ptot) leave as one run to the slots [P stride, P stride + ptot), low halves to keys16, high halves to idx16.

stage_pass() builds the stage of one pass, producer_flat() the buffers of a whole call, with the slots it wrote;
tests/test_pm_flat_writeout_model.py holds them against tests/pass_major_model.py."""
import numpy as np

import pass_major_model as pm

PASS = pm.PASS
FLAT_DIGITS = 32          # digit interval the form serves
STAGE_WORDS = 10240       # the stage in LDS: 8 192 records and up to 63 words of padding for each of 32 slices
STALE = 0xDEAD            # what the model's stage holds where the pass put no record (the device: whatever was there)


def takes_flat_form(d_lo, d_hi):
    """the producer's choice, per pass: the digit interval of the pass's contigs, not the digits that occur"""
    return d_lo <= d_hi and d_hi - d_lo + 1 <= FLAT_DIGITS


def stage_pass(digits, low):
    """digits, low: range and position inside the range of every read of one pass, in read order.
    -> stage (STAGE_WORDS words: low | index in pass << 16), ptot, the slices' padded bases, their record counts"""
    digits = np.asarray(digits, np.int64)
    low = np.asarray(low, np.int64)
    assert 1 <= digits.size <= PASS and low.max() < (1 << 16)
    c = np.bincount(digits, minlength=256).astype(np.int64)
    pad = (c + 63) // 64 * 64
    pbase = np.concatenate([[0], np.cumsum(pad)[:-1]])
    ptot = int(pad.sum())
    assert ptot <= STAGE_WORDS, "the padded pass does not fit the stage"
    stage = np.full(STAGE_WORDS, STALE | (STALE << 16), np.int64)
    # the stable rank inside the slice: the earlier reads of the pass with the same digit
    order = np.argsort(digits, kind="stable")
    compact = np.concatenate([[0], np.cumsum(c)[:-1]])
    rank = np.empty(digits.size, np.int64)
    rank[order] = np.arange(digits.size) - compact[digits[order]]
    slot = pbase[digits] + rank
    assert np.unique(slot).size == slot.size and slot.max() < ptot
    stage[slot] = low | (np.arange(digits.size) << 16)
    return stage, ptot, pbase, c


def producer_flat(gstart, shift, n_ranges, digit_interval):
    """digit_interval(P) -> (d_lo, d_hi) of pass P.  -> keys16, idx16 (0xFFFF where nothing was written), written (bool
    per slot), ptots (per pass; -1 where the pass keeps the slice-by-slice write-out, which the model leaves unwritten)"""
    gstart = np.asarray(gstart, np.int64)
    n = gstart.size
    pitch, stride = pm.pitch_for(n), pm.stride_for(n_ranges)
    keys16 = np.full(pitch * stride, 0xFFFF, np.uint16)
    idx16 = np.full(pitch * stride, 0xFFFF, np.uint16)
    written = np.zeros(pitch * stride, bool)
    ptots = []
    for P in range((n + PASS - 1) // PASS):
        g = gstart[P * PASS:min(n, (P + 1) * PASS)]
        d_lo, d_hi = digit_interval(P)
        if not takes_flat_form(d_lo, d_hi):
            ptots.append(-1)
            continue
        digits = g >> shift
        assert digits.min() >= d_lo and digits.max() <= d_hi
        stage, ptot, _, _ = stage_pass(digits, g & ((1 << shift) - 1))
        assert ptot % 64 == 0 and ptot <= stride
        at = P * stride                                   # a multiple of 64: every 16-byte store is aligned
        keys16[at:at + ptot] = (stage[:ptot] & 0xFFFF).astype(np.uint16)
        idx16[at:at + ptot] = (stage[:ptot] >> 16).astype(np.uint16)
        written[at:at + ptot] = True
        ptots.append(ptot)
    return keys16, idx16, written, np.asarray(ptots, np.int64)
