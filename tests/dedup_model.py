"""The contract of qmcp_hip_solve_dedup_* (include/qmcp_hip.h) stated literally with numpy: families by np.lexsort, the
representative the first of every family in (score descending, index ascending) order, the keep mask the oracle's
by-contig selection (tests/multi_reference.py) of the representatives' reads in input order, mapped back."""
import numpy as np

import multi_reference as mr

NO_CONTIG = mr.NO_CONTIG


def pack(bits):
    n = bits.size
    out = np.zeros(((n + 63) // 64) * 64, dtype=np.uint8)
    out[:n] = bits
    return np.packbits(out, bitorder="little").view(np.uint64)[:(n + 63) // 64].copy()


def unpack(mask, n):
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[:n].astype(bool)


def _families(order, keys):
    """order: the units sorted so that equal keys are adjacent; keys: per unit, the columns that name its family ->
    (representative units, duplicate units, sizes)"""
    if order.size == 0:
        return order, order, np.zeros(0, np.int64)
    k = np.stack([np.asarray(c)[order] for c in keys], axis=1)
    head = np.ones(order.size, dtype=bool)
    head[1:] = (k[1:] != k[:-1]).any(axis=1)
    at = np.flatnonzero(head)
    sizes = np.diff(np.concatenate([at, [order.size]]))
    return order[head], order[~head], sizes


def dedup(oracle, starts, ends, contig_ids, contig_lengths, M, tags=None, qualities=None, pairs=False,
          complete_pairs=False, hist_bins=0, by_contig=None):
    """-> (keep bits, duplicate bits, stats dict, hist): bool arrays in input order.  by_contig(starts, ends, ids,
    lengths, M) -> packed mask replaces the oracle's by-contig selection where the oracle cannot go (contigs of 2^27
    positions): the by-contig entry itself, which has its own tests against the oracle"""
    s = np.asarray(starts, dtype=np.int64)
    e = np.asarray(ends, dtype=np.int64)
    ids = np.asarray(contig_ids, dtype=np.int64)
    n = s.size
    t = np.zeros(n, np.int64) if tags is None else np.asarray(tags, dtype=np.int64)
    q = np.zeros(n, np.int64) if qualities is None else np.asarray(qualities, dtype=np.int64)
    placed = ids != NO_CONTIG
    survive = np.zeros(n, dtype=bool)
    dup = np.zeros(n, dtype=bool)
    if not pairs:
        units = np.flatnonzero(placed)
        order = units[np.lexsort((units, -q[units], t[units], e[units], s[units], ids[units]))]
        reps, dups, sizes = _families(order, (ids, s, e, t))
        survive[reps] = True
        dup[dups] = True
    else:
        assert n % 2 == 0
        # cell ids: one per distinct (contig, start, end, tag) of the placed reads, one more (the largest) for cell U
        cell = np.full(n, -1, dtype=np.int64)
        if placed.any():
            rows = np.stack([ids[placed], s[placed], e[placed], t[placed]], axis=1)
            _, inv = np.unique(rows, axis=0, return_inverse=True)
            cell[placed] = inv.reshape(-1)
        cell[~placed] = cell.max() + 1 if n else 0
        a, b = cell[0::2], cell[1::2]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        score = np.where(placed[0::2], q[0::2], 0) + np.where(placed[1::2], q[1::2], 0)
        units = np.flatnonzero(placed[0::2] | placed[1::2])
        order = units[np.lexsort((units, -score[units], hi[units], lo[units]))]
        reps, dups, sizes = _families(order, (lo, hi))
        survive[2 * reps] = True
        survive[2 * reps + 1] = True
        dup[2 * dups] = True
        dup[2 * dups + 1] = True
    keep = np.zeros(n, dtype=bool)
    on = np.flatnonzero(survive)
    if on.size:
        cols = (s[on].astype(np.uint32), e[on].astype(np.uint32), ids[on].astype(np.uint32))
        m = by_contig(*cols, contig_lengths, M) if by_contig else mr.oracle_by_contig(oracle, *cols, contig_lengths, M)
        keep[on[unpack(m, on.size)]] = True
    if complete_pairs:
        both = keep[0::2] | keep[1::2]
        keep[0::2] = both
        keep[1::2] = both
    hist = np.zeros(hist_bins, dtype=np.uint64)
    if hist_bins:
        np.add.at(hist, np.minimum(sizes, hist_bins) - 1, 1)
    stats = dict(units=int(units.size), families=int(sizes.size), duplicate_units=int(units.size - sizes.size),
                 largest_family=int(sizes.max()) if sizes.size else 0, reads_survived=int(survive.sum()))
    return keep, dup, stats, hist


def plan(field_bits):
    """dedup_plan.h's plan_dedup_sort restated: fields least significant first -> dict(key_bits, form, passes, rounds);
    a round is (mask of its fields, bits, passes, shifts of its fields)"""
    key_bits = sum(field_bits)
    if key_bits <= 64:
        shifts, at = [], 0
        for b in field_bits:
            shifts.append(at)
            at += b
        on = sum(1 << f for f, b in enumerate(field_bits) if b)
        passes = (key_bits + 7) // 8 if key_bits else 1
        return dict(key_bits=key_bits, form=0 if key_bits <= 32 else 1, passes=passes,
                    rounds=[(on, key_bits, passes, [shifts[f] for f, b in enumerate(field_bits) if b])])
    rounds = [(1 << f, b, (b + 7) // 8, [0]) for f, b in enumerate(field_bits) if b]
    return dict(key_bits=key_bits, form=2, passes=sum(r[2] for r in rounds), rounds=rounds)


def read_fields(total_length, min_span, max_span, tag_lo, tag_hi, q_lo, q_hi, with_quality=True):
    w = lambda lo, hi: int(hi - lo).bit_length() if lo <= hi else 0
    return [w(q_lo, q_hi) if with_quality else 0, w(tag_lo, tag_hi), w(min_span, max_span), int(total_length).bit_length()]


def pair_fields(n_placed, q_lo, q_hi):
    ib = int(n_placed).bit_length()
    return [int(2 * (q_hi - q_lo)).bit_length() if q_lo <= q_hi else 0, ib, ib]
