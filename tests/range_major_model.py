"""Host-side model of the RANGE-MAJOR form of the range-ranked route (csrc/kernels/prepare_scan.inc.hip: k_prepare, the
scan; csrc/kernels/ranked_route.inc.hip: k_range_partition, k_seg_tables, k_seg_hist, k_seg_range_table, k_range_offsets,
k_rank_mark): what every launch leaves in every buffer, in plain numpy with Python loops over tiles, passes and ranges
only, every index asserted in bounds.  tests/rm_stage_compare.py holds the device's buffers against it,
tests/test_range_major_model.py holds it against direct numpy (a stable argsort by range, bincount, searchsorted).

Geometry (restated from kernels/launchers.inc.hip; the stage driver reports the library's own values and the
comparison requires them to agree).  Reads are cut into TILES of 4 096 and partition PASSES of 8 192 (two tiles).
k_prepare counts, per (digit, pass), the regular reads whose clamped global start has that digit (digit = (gstart >>
part_shift) & 255) into a [256][pitch] table; its exclusive scan gives, for a fixed digit, the passes' runs one behind
the other, so a pass's records of a digit go to table[digit][pass] + their rank inside the pass.  One level: digit =
range.  Two levels (genomes from 2^23 positions): the first level's digit is the SUPER-RANGE (shift + 8), its output
{global start, index} records; every super-range is then cut into tiles and passes of its own and partitioned by its
second digit through a [super-range][digit][tile] histogram, scanned over its whole extent."""
import numpy as np

TILE = 4096
PASS = 8192
PART_WAVE = 1024       # records of a pass one partition wave owns
EXC_PER_GROUP = 128    # exception-list slots per (tile, wave)
NU_OVERFLOW = 1 << 20  # kNuOverflow: the list's last slots, for what a group's 128 do not hold
MAX_RANGE_SHIFT = 15
RANGES_WORDS = 65537 + 7 + 771 + 5
MAX_LOAD_AT, SEG_TABLES_AT = 65540, 65544


# ------------------------------------------------------------------------------------------------------------ geometry
def sort_tiles(n):
    return (n + TILE - 1) // TILE


def part_pass_pitch(n):
    return (((sort_tiles(n) + 1) >> 1) + 3) & ~3


def range_path_two_level(ltot):
    return (ltot >> MAX_RANGE_SHIFT) >= 256


def range_shift_for(ltot):
    shift = 0
    while shift < MAX_RANGE_SHIFT and (ltot >> shift) >= 256:
        shift += 1
    if range_path_two_level(ltot):
        lowest = 0
        while (ltot >> lowest) >= 65536:
            lowest += 1
        shift = max(lowest, MAX_RANGE_SHIFT)
    return shift


def n_ranges_for(ltot, shift):
    """ranges the per-range kernels are launched over: positions 0 .. ltot inclusive"""
    return (ltot >> shift) + 1


def seg_tile_bound(n):
    return sort_tiles(n) + 256


def scan_spine_entries(n):
    return (n + 4095) // 4096 + 1


def spine_bytes(n, ltot):
    """api/solve_head.inc.hip: the larger of the level-2 histogram's spine and a scan over the positions"""
    return max(scan_spine_entries(256 * seg_tile_bound(n)) * 4 + 16, (scan_spine_entries(ltot + 1) + 1) * 4 + 16)


def rank_by_pos_slots(shift, ltot):
    return n_ranges_for(ltot, shift) << shift


def rank_scratch_by_records(shift, ltot, n):
    return n < rank_by_pos_slots(shift, ltot)


def rank_scratch_bytes(shift, ltot, n):
    return min(rank_by_pos_slots(shift, ltot), n) * 8 + 64


def prepare_exc_slots(n):
    return sort_tiles(n) * 4 * EXC_PER_GROUP + NU_OVERFLOW


# --------------------------------------------------------------------------------------------------------------- reads
def contig_of_reads(roff):
    roff = np.asarray(roff, np.int64)
    return np.repeat(np.arange(roff.size - 1), np.diff(roff))


def clamped(local, contig, lengths):
    """a coordinate at or beyond its contig's length -- the call fails -- is taken as the contig's last position"""
    last = np.maximum(np.asarray(lengths, np.int64) - 1, 0)
    return np.minimum(np.asarray(local, np.int64), last[contig])


def spans32(starts, ends):
    return (np.asarray(ends, np.int64) - np.asarray(starts, np.int64) + 1) & 0xFFFFFFFF


def regular_reads(starts, ends, ell_reg):
    if ell_reg == 0:
        return np.ones(np.asarray(starts).size, bool)
    return spans32(starts, ends) == ell_reg


def lean_tiles(roff, n):
    """k_prepare's lean path: whole tiles inside one contig"""
    contig = contig_of_reads(roff)
    lean = np.zeros(sort_tiles(n), bool)
    for t in range(sort_tiles(n)):
        lo, hi = t * TILE, min(n, (t + 1) * TILE)
        lean[t] = hi - lo == TILE and contig[lo] == contig[hi - 1]
    return lean


# -------------------------------------------------------------------------------------------------------------- stages
def prepare(starts, ends, roff, lengths, ell_reg, part_shift):
    """k_prepare (+ k_nu_count_groups): -> dict with
    stats012  span minimum and maximum over the valid reads and the error flag (a lean tile -- whole, one contig --
              does not branch per read: there an invalid read's span, in 32-bit arithmetic, enters the range too)
    table     [256][pitch] regular reads per (digit, pass), the digit of the clamped global start; padding passes zero
    gs, ge    clamped global starts and ends; regular: the reads that enter the partition
    with a filter: exc_total [groups] exceptions per (tile, wave) group -- the wave's reads of a tile are j = 256 k + 64 w
    + lane --, exc_of {group: int64 [m][3] (start, end, index) in read-index order}, lean [tiles]"""
    starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    lengths = np.asarray(lengths, np.int64)
    n = starts.size
    poff = np.concatenate([[0], np.cumsum(lengths)])
    contig = contig_of_reads(roff)
    assert contig.size == n and n >= 1
    gs = poff[contig] + clamped(starts, contig, lengths)
    ge = poff[contig] + clamped(ends, contig, lengths)
    assert gs.max() < max(int(poff[-1]), 1)
    span = spans32(starts, ends)
    bad = (starts > ends) | (ends >= lengths[contig])
    regular = regular_reads(starts, ends, ell_reg)
    assert not (ell_reg != 0 and bad.any()), "the model does not follow invalid reads through the filter"
    lean = lean_tiles(roff, n)
    counted = ~bad | np.repeat(lean, TILE)[:n]          # reads whose span enters the statistics
    mn = int(span[counted].min()) if counted.any() else 0xFFFFFFFF
    mx = int(span[counted].max()) if counted.any() else 0
    pitch = part_pass_pitch(n)
    table = np.zeros((256, pitch), np.uint32)
    digit = (gs >> part_shift) & 255
    for P in range((n + PASS - 1) // PASS):
        lo, hi = P * PASS, min(n, (P + 1) * PASS)
        assert P < pitch
        table[:, P] = np.bincount(digit[lo:hi][regular[lo:hi]], minlength=256)
    out = {"n": n, "pitch": pitch, "stats012": (mn, mx, int(bad.any())), "table": table, "gs": gs, "ge": ge, "regular": regular,
           "contig": contig, "poff": poff, "lean": lean}
    if ell_reg != 0:
        groups = sort_tiles(n) * 4
        exc_total = np.zeros(groups, np.int64)
        exc_of = {}
        idx = np.nonzero(~regular)[0]
        grp = (idx // TILE) * 4 + ((idx % TILE) % 256) // 64
        for g in np.unique(grp):
            i = idx[grp == g]
            assert 0 <= g < groups
            exc_total[g] = i.size
            exc_of[int(g)] = np.stack([gs[i], ge[i], i], axis=1).astype(np.int64)
        out.update({"exc_total": exc_total, "exc_of": exc_of})
    return out


def scan_table(table):
    """launch_exclusive_scan over the flattened table with the total behind it; -> scanned [256 pitch + 1], spine (tile
    sums of 4 096 entries scanned, the total behind them)"""
    flat = table.reshape(-1).astype(np.int64)
    scanned = np.concatenate([[0], np.cumsum(flat)])
    assert scanned[-1] < (1 << 32)
    tiles = (flat.size + 4095) // 4096
    sums = np.array([flat[t * 4096:(t + 1) * 4096].sum() for t in range(tiles)], np.int64)
    spine = np.concatenate([[0], np.cumsum(sums)])
    return scanned.astype(np.uint32), spine.astype(np.uint32)


def _partition_passes(key, val, bounds, shift, dest_of, total):
    """the stable scatter every partition launch does: records [lo, hi) of every pass in `bounds` go, digit by digit in
    input order, to dest_of(pass number, digit) + their rank inside the pass.  -> destination per record (-1: none)"""
    dst = np.full(key.size, -1, np.int64)
    for P, (lo, hi) in enumerate(bounds):
        if hi <= lo:
            continue
        d = (key[lo:hi] >> shift) & 255
        order = np.argsort(d, kind="stable")
        c = np.bincount(d, minlength=256)
        first = np.concatenate([[0], np.cumsum(c)[:-1]])
        for dd in np.nonzero(c)[0]:
            at = int(dest_of(P, int(dd)))
            assert 0 <= at and at + c[dd] <= total, "a pass's run leaves the stream"
            dst[lo + order[first[dd]:first[dd] + c[dd]]] = at + np.arange(c[dd])
    return dst


def partition_one_level(prep, scanned, shift):
    """k_range_partition<1, false>.  -> keys16 [total], idx [total], range_start [257], max_load"""
    n, pitch = prep["n"], prep["pitch"]
    reg = np.nonzero(prep["regular"])[0]
    total = int(scanned[256 * pitch])
    assert total == reg.size
    key = prep["gs"][reg]
    # the regular reads of pass P: a slice of `reg`
    cut = np.searchsorted(reg, np.arange(0, n + PASS, PASS))
    bounds = list(zip(cut[:-1], cut[1:]))
    dst = _partition_passes(key, reg, bounds, shift, lambda P, d: scanned[d * pitch + P], total)
    assert (dst >= 0).all() and np.unique(dst).size == total
    keys16 = np.zeros(total, np.uint16)
    idx = np.zeros(total, np.uint32)
    keys16[dst] = key & ((1 << shift) - 1)
    idx[dst] = reg
    range_start = np.concatenate([scanned[np.arange(256) * pitch], [total]]).astype(np.uint32)
    return keys16, idx, range_start, int(np.diff(range_start.astype(np.int64)).max())


def partition_two_levels(prep, scanned, shift, seg_bound):
    """k_range_partition<1, true>, k_seg_tables, k_seg_hist, the scan, k_range_partition<2, false>, k_seg_range_table.
    -> dict: recs [total][2] {global start, index}, super_start / tile_base / pass_base [257], hist [256 seg_bound] (the
    level-2 histogram [super-range][digit][tile] over the extent tile_base[256] gives, zeros behind it), hist_scanned (its
    exclusive scan, as the device leaves the buffer), keys16, idx, range_start [65537], max_load"""
    n, pitch = prep["n"], prep["pitch"]
    reg = np.nonzero(prep["regular"])[0]
    total = int(scanned[256 * pitch])
    assert total == reg.size
    key = prep["gs"][reg]
    cut = np.searchsorted(reg, np.arange(0, n + PASS, PASS))
    dst = _partition_passes(key, reg, list(zip(cut[:-1], cut[1:])), shift + 8, lambda P, d: scanned[d * pitch + P], total)
    assert (dst >= 0).all() and np.unique(dst).size == total
    recs = np.zeros((total, 2), np.uint32)
    recs[dst, 0] = key
    recs[dst, 1] = reg
    super_start = np.concatenate([scanned[np.arange(256) * pitch], [total]]).astype(np.int64)
    n_h = np.diff(super_start)
    t_h = (n_h + TILE - 1) // TILE
    p_h = (t_h + 1) // 2
    tile_base = np.concatenate([[0], np.cumsum(t_h)])
    pass_base = np.concatenate([[0], np.cumsum(p_h)])
    assert tile_base[256] <= seg_bound
    hist = np.zeros(256 * seg_bound, np.int64)
    rkey = recs[:, 0].astype(np.int64)
    for h in np.nonzero(t_h)[0]:
        for t in range(int(t_h[h])):
            lo, hi = super_start[h] + t * TILE, min(super_start[h] + (t + 1) * TILE, super_start[h + 1])
            at = tile_base[h] * 256 + np.arange(256) * t_h[h] + t
            assert at.max() < 256 * tile_base[256]
            hist[at] = np.bincount((rkey[lo:hi] >> shift) & 255, minlength=256)
    hscan = np.concatenate([[0], np.cumsum(hist)[:-1]])
    keys16 = np.zeros(total, np.uint16)
    idx = np.zeros(total, np.uint32)
    written = np.zeros(total, bool)
    for h in np.nonzero(t_h)[0]:
        lo0, hi0 = int(super_start[h]), int(super_start[h + 1])
        bounds = [(lo0 + p * PASS, min(lo0 + (p + 1) * PASS, hi0)) for p in range(int(p_h[h]))]
        row, th = int(tile_base[h]) * 256, int(t_h[h])
        d2 = _partition_passes(rkey, None, bounds, shift, lambda P, d: hscan[row + 2 * P + d * th], total)
        sel = np.nonzero(d2 >= 0)[0]
        assert sel.size == hi0 - lo0 and not written[d2[sel]].any()
        written[d2[sel]] = True
        keys16[d2[sel]] = rkey[sel] & ((1 << shift) - 1)
        idx[d2[sel]] = recs[sel, 1]
    assert written.all()
    range_start = np.zeros(65537, np.int64)
    for h in range(256):
        row, th = int(tile_base[h]) * 256, int(t_h[h])
        range_start[h * 256:(h + 1) * 256] = hscan[row + np.arange(256) * th] if th else super_start[h]
    range_start[65536] = super_start[256]
    his = np.concatenate([range_start[1:65536], [0]])
    his[255::256] = super_start[1:]                     # a super-range's last range ends where the next super-range begins
    return {"recs": recs, "super_start": super_start.astype(np.uint32), "tile_base": tile_base.astype(np.uint32),
            "pass_base": pass_base.astype(np.uint32), "hist": hist.astype(np.uint32), "hist_scanned": hscan.astype(np.uint32),
            "keys16": keys16, "idx": idx, "range_start": range_start.astype(np.uint32),
            "max_load": int((his - range_start[:65536]).max())}


def offsets(keys16, range_start, shift, ltot):
    """k_range_offsets, range by range: the range's keys histogrammed, scanned from the range's first record on.
    -> boff [ltot + 1], the empty-position count (positions below ltot that start no read)"""
    width = 1 << shift
    boff = np.zeros(ltot + 1, np.uint32)
    empties = 0
    for r in range(n_ranges_for(ltot, shift)):
        lo, hi = int(range_start[r]), int(range_start[r + 1])
        assert lo <= hi <= keys16.size
        k = keys16[lo:hi].astype(np.int64)
        assert k.size == 0 or k.max() < width
        c = np.bincount(k, minlength=width)
        pos0 = r << shift
        live = min(width, ltot + 1 - pos0)               # positions pos0 .. ltot get an offset
        assert live >= 1 and not c[min(width, max(ltot - pos0, 0)):].any(), "a record at or beyond the genome's end"
        boff[pos0:pos0 + live] = lo + np.concatenate([[0], np.cumsum(c)[:-1]])[:live]
        empties += int((c[:max(min(width, ltot - pos0), 0)] == 0).sum())
    return boff, empties


def rank_mask(keys16, idx, range_start, shift, ltot, boff, selend, n):
    """k_rank_mark: walking a range's records in order, a record is kept while its position's quota selend - boff lasts.
    -> bool per read, the kept total"""
    total = int(range_start[n_ranges_for(ltot, shift)])
    mask = np.zeros(n, bool)
    kept = 0
    for r in range(n_ranges_for(ltot, shift)):
        lo, hi = int(range_start[r]), int(range_start[r + 1])
        if hi <= lo:
            continue
        assert hi <= total
        pos0 = r << shift
        live = min(1 << shift, ltot - pos0)
        k = keys16[lo:hi].astype(np.int64)
        assert live > 0 and k.max() < live
        q = selend[pos0:pos0 + live].astype(np.int64) - boff[pos0:pos0 + live].astype(np.int64)
        order = np.argsort(k, kind="stable")
        ks = k[order]
        first = np.searchsorted(ks, ks, side="left")     # a record's rank among its position's = its place - the first's
        keep = np.zeros(hi - lo, bool)
        keep[order] = (np.arange(hi - lo) - first) < q[ks]
        reads = idx[lo:hi][keep].astype(np.int64)
        assert reads.size == 0 or (reads.max() < n and not mask[reads].any())
        mask[reads] = True
        kept += reads.size
    return mask, kept
