"""Host restatement of the pass-major producer's ranking by per-lane counts (csrc/kernels/pm_lane_rank.inc.hip), word
for word: the [digit pair][lane] words with two 16-bit counters each, the returning add that hands back the in-lane
running counts, the scan over the lanes stored one lane up with the wave's totals in slot 0, and the cross-wave step of
k_pm_prepare_sort.  Lane l of wave w owns the reads [1024 w + 16 l, 1024 w + 16 l + 16) of the pass.

rank_pass(digits, d_lo, n_pairs) -> the position of every read inside the pass sorted stably by digit, which is what a
stable argsort gives (tests/test_pm_lane_rank_model.py holds the two against each other)."""
import numpy as np

PASS = 8192
WAVES = 8
LANES = 64
PER_LANE = 16
FIELD = 0xFFFF


def wave_words(rel, valid):
    """one wave: rel, valid per read (1 024 entries, in read order) -> (old, words, totals): the word the returning add
    handed back per read, the wave's [16][64] words after the scan (lane l's slot: the exclusive prefix over the lanes,
    slot 0 cleared), and the wave's record count per digit (32 entries)"""
    words = np.zeros((16, LANES), np.int64)
    old = np.zeros(LANES * PER_LANE, np.int64)
    for lane in range(LANES):
        for j in range(PER_LANE):
            i = lane * PER_LANE + j
            pair, field = (int(rel[i]) >> 1) & 15, (int(rel[i]) & 1) << 4
            old[i] = words[pair, lane]
            words[pair, lane] += (1 << field) if valid[i] else 0
    inclusive = np.cumsum(words, axis=1)            # one 32-bit scan serves both fields: no field exceeds 1 024
    assert ((inclusive & FIELD) <= LANES * PER_LANE).all() and ((inclusive >> 16) <= LANES * PER_LANE).all()
    stored = np.roll(inclusive, 1, axis=1)          # lane l writes slot (l + 1) & 63
    totals = np.zeros(32, np.int64)
    totals[0::2], totals[1::2] = stored[:, 0] & FIELD, stored[:, 0] >> 16
    stored[:, 0] = 0                                # lane 0's exclusive prefix
    return old, stored, totals


def rank_pass(digits, d_lo, n_pairs):
    """digits: the digit of every read of one pass (<= 8 192 reads, all inside [d_lo, d_lo + 2 n_pairs))"""
    digits = np.asarray(digits, np.int64)
    count = digits.size
    assert 1 <= count <= PASS and 1 <= n_pairs <= 16
    assert digits.min() >= d_lo and digits.max() < d_lo + 2 * n_pairs
    rel = np.zeros(PASS, np.int64)
    rel[:count] = digits - d_lo
    valid = np.arange(PASS) < count
    s_cnt = np.zeros((WAVES, 32), np.int64)
    in_wave = np.zeros(PASS, np.int64)
    for w in range(WAVES):
        sl = slice(w * 1024, (w + 1) * 1024)
        old, words, s_cnt[w] = wave_words(rel[sl], valid[sl])
        lane = np.arange(1024) // PER_LANE
        pair, field = (rel[sl] >> 1) & 15, (rel[sl] & 1) << 4
        in_wave[sl] = ((old + words[pair, lane]) >> field) & FIELD
    # the cross-wave step (unchanged in the kernel): a digit's records begin behind the lower digits' totals, a wave's
    # behind the lower waves'
    tot = s_cnt.sum(axis=0)
    digit_base = np.concatenate([[0], np.cumsum(tot)[:-1]])
    wave_base = np.cumsum(s_cnt, axis=0) - s_cnt
    w_of = np.arange(PASS) // 1024
    pos = digit_base[rel] + wave_base[w_of, rel] + in_wave
    return pos[:count]
