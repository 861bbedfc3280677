"""Host-side model of the PASS-MAJOR layout of the range-ranked route (csrc/kernels/pass_major.inc.hip), round 4 form
-- every index its producer writes and its consumers read, with bounds asserted -- so that the layout's arithmetic is
checked on the CPU before (and beside) any GPU run.  (Round 2's abandoned 16-bit-index experiment ended in a GPU
memory-access fault whose code was not kept; since then a layout is modelled first.)

Layout.  The reads of a call are cut into PASSES of 8 192 consecutive reads.  k_pm_prepare_sort sorts every pass by
position range (digit = clamped global start >> shift, <= 256 ranges), stably, and writes the pass's records of range
d -- its SLICE (d, P) -- at a slot that is a multiple of 64: pass P owns the slots [P * stride, (P + 1) * stride),
stride = 8192 + 64 * n_ranges, and the slices follow each other padded to whole groups of 64 slots.  Two 16-bit
streams: keys16[slot] = global start & (2^shift - 1), idx16[slot] = read index - P * 8192.  Two tables laid out
[range][pass] (row pitch a multiple of 4):
    cntp[d][P] = records of the slice rounded up to a multiple of 64      lstw[d][P] = (first slot - P * stride) / 64
                                                                                       | true record count << 16
An exclusive scan over the flattened cntp table gives Tp[d][P]: the PADDED FLAT position of the slice -- range d's
records in read-index order are its slices in pass order, each padded to whole groups.  A group of 64 padded flat
positions (a WAVE-SLOT, g = position / 64) therefore lies in exactly one slice, and a one-word descriptor per
wave-slot says where: desc[g] = pass << 15 | slot group inside the pass << 6 | (records in the group - 1).  The
consumers never search:
    k_pm_offsets  walks a range's wave-slots in any order (LDS histogram of the positions);
    k_pm_walk     walks them in order, sixteen (one chunk) per step, against the per-position quotas, and marks the kept
                  records' read indices (pass * 8192 + idx16);
    k_pm_settle   decides the (chunk, position) groups whose quota ran out inside a chunk.
"""
import numpy as np

PASS = 8192
CHUNK_WS = 16          # wave-slots per chunk (one per wave of the walking workgroup)
WAVE_READS = 1024      # reads of a pass one producer wave owns (eight waves a pass)
EXC_PER_WAVE = 128     # exception-list slots per (pass, wave)
MAX_RANGE_SHIFT = 15


def pitch_for(n):
    n_pass = (n + PASS - 1) // PASS
    return (n_pass + 3) & ~3


def stride_for(n_ranges):
    return PASS + 64 * n_ranges


def producer(gstart, shift, n_ranges, regular=None):
    """-> keys16, idx16 (pitch * stride slots, 0xFFFF where nothing was written), cntp, lstw ([256][pitch] uint32).
    regular (bool per read, or None: every read): the reads that enter the slices -- the near-uniform route's filter
    leaves the others out; idx16 stays the read's index inside its pass"""
    n = gstart.size
    pitch = pitch_for(n)
    stride = stride_for(n_ranges)
    keys16 = np.full(pitch * stride, 0xFFFF, np.uint16)
    idx16 = np.full(pitch * stride, 0xFFFF, np.uint16)
    cntp = np.zeros((256, pitch), np.uint32)
    lstw = np.zeros((256, pitch), np.uint32)
    for P in range((n + PASS - 1) // PASS):
        lo, hi = P * PASS, min(n, (P + 1) * PASS)
        sel = np.arange(hi - lo) if regular is None else np.nonzero(regular[lo:hi])[0]
        d = (gstart[lo:hi][sel] >> shift).astype(np.int64)
        assert d.size == 0 or d.max() < n_ranges <= 256
        order = np.argsort(d, kind="stable")
        c = np.bincount(d, minlength=256).astype(np.int64)
        pad = (c + 63) // 64 * 64
        first = np.concatenate([[0], np.cumsum(pad)[:-1]])
        assert first[-1] + pad[-1] <= stride
        compact = np.concatenate([[0], np.cumsum(c)[:-1]])
        for dd in np.nonzero(c)[0]:
            src = sel[order[compact[dd]:compact[dd] + c[dd]]]
            at = P * stride + first[dd]
            keys16[at:at + c[dd]] = (gstart[lo:hi][src] & ((1 << shift) - 1)).astype(np.uint16)
            idx16[at:at + c[dd]] = src.astype(np.uint16)
        cntp[:, P] = pad.astype(np.uint32)
        assert (first // 64).max() < (1 << 16) and c.max() < (1 << 16)
        lstw[:, P] = ((first // 64) | (c << 16)).astype(np.uint32)
    return keys16, idx16, cntp, lstw


def scan_table(cntp):
    """exclusive scan over the flattened [range][pass] table, total appended (launch_exclusive_scan, write_total)"""
    flat = cntp.reshape(-1).astype(np.uint64)
    return np.concatenate([[0], np.cumsum(flat)]).astype(np.uint32)


def unpack(dsc, stride):
    """-> first slot, records, pass of a wave-slot's descriptor"""
    dsc = int(dsc)
    P = dsc >> 15
    return P * stride + ((dsc >> 6) & 511) * 64, (dsc & 63) + 1, P


def descriptors(Tp, lstw, n, n_ranges):
    """k_pm_descr + k_pm_range_table: one thread per (range, pass) table entry -> the slice's wave-slot descriptors, and
    (row sums of the true counts, scanned) the ranges' TRUE flat starts.  -> desc [G], range_start [257] (true)"""
    pitch = pitch_for(n)
    G = int(Tp[-1]) // 64
    desc = np.full(G, 0xFFFFFFFF, np.uint32)
    true_rows = np.zeros(256, np.int64)
    for d in range(256):
        for P in range(pitch):
            w = int(lstw[d, P])
            cnt, lst64 = w >> 16, w & 0xFFFF
            if cnt == 0:
                continue
            true_rows[d] += cnt
            t = int(Tp[d * pitch + P])
            assert t % 64 == 0
            g = t // 64
            n_ws = (cnt + 63) // 64
            for j in range(n_ws):
                assert P < (1 << 17) and lst64 + j < 512 and g + j < G and desc[g + j] == 0xFFFFFFFF
                desc[g + j] = (P << 15) | ((lst64 + j) << 6) | (min(64, cnt - 64 * j) - 1)
    assert not (desc == 0xFFFFFFFF).any()      # every wave-slot of the padded flat space belongs to a slice
    range_start = np.concatenate([[0], np.cumsum(true_rows)]).astype(np.uint32)
    assert int(range_start[-1]) <= n
    return desc, range_start


def range_wave_slots(Tp, pitch, d):
    lo, hi = int(Tp[d * pitch]), int(Tp[(d + 1) * pitch])
    assert lo % 64 == 0 and hi % 64 == 0
    return lo // 64, (hi - lo) // 64


def offsets(keys16, desc, Tp, pitch, d, shift, stride):
    """k_pm_offsets: the range's positions, histogrammed (order-free)"""
    g0, n_ws = range_wave_slots(Tp, pitch, d)
    hist = np.zeros(1 << shift, np.int64)
    for ws in range(n_ws):
        slot0, nv, _ = unpack(desc[g0 + ws], stride)
        k = keys16[slot0:slot0 + nv]
        assert k.max() < (1 << shift)
        np.add.at(hist, k.astype(np.int64), 1)
    return hist


def walk(keys16, idx16, desc, Tp, pitch, d, quota, stride, n, mask, rng):
    """k_pm_walk for one range.  quota: int array [1 << shift] = S(p).  Chunks of 16 wave-slots in order; inside a chunk
    the draws happen in an arbitrary order (rng permutation: the device's LDS arbitration).  Sets mask[read index] of the
    kept records; -> amb [(chunk, position key, skip)], kept"""
    g0, n_ws = range_wave_slots(Tp, pitch, d)
    q = quota.astype(np.int64).copy()
    amb = []
    kept = 0
    n_chunks = (n_ws + CHUNK_WS - 1) // CHUNK_WS
    for c in range(n_chunks):
        recs = []          # (key, read index)
        for w in range(CHUNK_WS):
            ws = c * CHUNK_WS + w
            if ws >= n_ws:
                continue
            slot0, nv, P = unpack(desc[g0 + ws], stride)
            for lane in range(nv):
                i = int(idx16[slot0 + lane])
                assert i < PASS
                recs.append((int(keys16[slot0 + lane]), P * PASS + i))
        order = rng.permutation(len(recs))
        old = [0] * len(recs)
        for i in order:
            old[i] = q[recs[i][0]]
            q[recs[i][0]] -= 1
        for i, (key, read) in enumerate(recs):
            aft = q[key]
            if old[i] > 0 and aft >= 0:
                assert read < n and not mask[read]
                mask[read] = True
                kept += 1
            if old[i] == 1 and aft < 0:
                amb.append((c, key, int(-aft)))
    return amb, kept


def settle(amb, keys16, idx16, desc, Tp, pitch, d, n, stride, mask):
    """k_pm_settle: a listed (chunk, position) group keeps all of the chunk's records at that position but the last
    `skip` in read-index order"""
    g0, n_ws = range_wave_slots(Tp, pitch, d)
    kept = 0
    for (c, key, skip) in amb:
        members = []
        for w in range(CHUNK_WS):
            ws = c * CHUNK_WS + w
            if ws >= n_ws:
                continue
            slot0, nv, P = unpack(desc[g0 + ws], stride)
            for lane in range(nv):
                if int(keys16[slot0 + lane]) == key:
                    members.append(P * PASS + int(idx16[slot0 + lane]))
        assert len(members) > skip
        for i in members[:len(members) - skip]:
            assert i < n and not mask[i]
            mask[i] = True
            kept += 1
    return kept


# ---- what the kernels write besides the layout (tests/pm_stage_compare.py holds the device's buffers against these)
def range_shift_for(ltot):
    """the smallest shift whose ranges of positions 0..ltot fit one partition level (one-level genomes only)"""
    shift = 0
    while shift < MAX_RANGE_SHIFT and (ltot >> shift) >= 256:
        shift += 1
    assert (ltot >> shift) < 256, "two partition levels: not the pass-major form"
    return shift


def contig_of_reads(roff):
    roff = np.asarray(roff, np.int64)
    return np.repeat(np.arange(roff.size - 1), np.diff(roff))


def clamped(local, contig, lengths):
    """k_pm_prepare_sort: a coordinate beyond its contig -- the call fails -- is taken as the contig's last position
    (min(s, len - 1); position 0 of a contig without positions)"""
    last = np.maximum(np.asarray(lengths, np.int64) - 1, 0)
    return np.minimum(np.asarray(local, np.int64), last[contig])


def statistics(starts, ends, contig, lengths):
    """stats[0..2]: minimum and maximum span over all reads (e - s + 1 in 32-bit arithmetic, as the kernel has it) and
    the bad flag (start > end, or end at or beyond the contig's length)"""
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    span = (e - s + 1) & 0xFFFFFFFF
    bad = (s > e) | (e >= np.asarray(lengths, np.int64)[contig])
    return int(span.min()), int(span.max()), int(bad.any())


def regular_reads(starts, ends, ell_reg):
    """the reads that enter the slices: all of them, or with a filter those of span ell_reg"""
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    if ell_reg == 0:
        return np.ones(s.size, bool)
    return ((e - s + 1) & 0xFFFFFFFF) == ell_reg


def exception_lists(gs, ge, regular):
    """the filtered producer's lists.  gs / ge: clamped global starts and ends of every read.  Each (pass, wave of 1 024
    reads) lists its first 128 exceptions in read-index order at slots (8 P + w) 128 ...; the rest go to the overflow
    region in any order.  -> cnt [pitch * 8], groups {group: int64 [k][3] = (start, end, index)}, overflow int64 [m][3]
    (in read-index order here)"""
    n = gs.size
    cnt = np.zeros(pitch_for(n) * (PASS // WAVE_READS), np.int64)
    groups, over = {}, []
    exc = np.nonzero(~regular)[0]
    grp = exc // WAVE_READS     # = 8 P + w: passes are eight waves
    for g in np.unique(grp):
        idx = exc[grp == g]
        ent = np.stack([gs[idx], ge[idx], idx], axis=1).astype(np.int64)
        cnt[g] = min(idx.size, EXC_PER_WAVE)
        groups[int(g)] = ent[:EXC_PER_WAVE]
        over.append(ent[EXC_PER_WAVE:])
    overflow = np.concatenate(over) if over else np.zeros((0, 3), np.int64)
    return cnt, groups, overflow


def loads(cntp, lstw):
    """max_load[0], [1]: the heaviest range's records (largest true row sum) and wave-slots (largest padded row sum / 64)"""
    return int((lstw >> 16).astype(np.int64).sum(axis=1).max()), int(cntp.astype(np.int64).sum(axis=1).max()) // 64


def bucket_offsets(gs_regular, ltot):
    """boff[p], p = 0 .. ltot: the regular reads that start below p (plain reference, not through the layout)"""
    return np.searchsorted(np.sort(np.asarray(gs_regular, np.int64)), np.arange(ltot + 1), side="left").astype(np.uint32)


def empty_positions(gs_regular, ltot):
    """stats[3]: positions of [0, ltot) at which no regular read starts"""
    return int(ltot - np.unique(np.asarray(gs_regular, np.int64)).size)


def expected_mask(gs, quota, regular=None):
    """the quota[p] lowest read indices of every global start p (plain reference, not through the layout); quota: an
    array per global position, or a callable.  Only the regular reads take part."""
    n = gs.size
    quota_of = quota if callable(quota) else (lambda p: quota[p])
    reads = np.arange(n) if regular is None else np.nonzero(regular)[0]
    mask = np.zeros(n, bool)
    if reads.size == 0:
        return mask
    order = reads[np.argsort(gs[reads], kind="stable")]
    sorted_g = gs[order]
    starts = np.concatenate([[0], np.nonzero(np.diff(sorted_g.astype(np.int64)))[0] + 1, [order.size]])
    for a, b in zip(starts[:-1], starts[1:]):
        k = min(int(quota_of(int(sorted_g[a]))), b - a)
        mask[order[a:a + k]] = True
    return mask
