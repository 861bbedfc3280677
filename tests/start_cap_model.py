"""The contract of qmcp_hip_solve_start_cap_* (include/qmcp_hip.h) stated literally with numpy: the placed reads sorted
by np.lexsort on (contig, start, group, -priority, -span, index), the rank inside every (contig, start, group) cell, the
survivors the ranks below K, the keep mask the oracle's by-contig selection (tests/multi_reference.py) of the survivors
in input order, mapped back; the kept reads per cell and the shortfall against min(cov of ALL placed reads, M) counted
from that mask."""
import numpy as np

import multi_reference as mr
from dedup_model import pack, unpack  # noqa: F401  (the tests take both from here)

NO_CONTIG = mr.NO_CONTIG
STAT_KEYS = ("reads_placed", "cells", "cells_over_cap", "reads_capped", "largest_cell", "reads_survived", "cells_kept",
             "largest_kept_cell", "short_positions", "short_bases")


def cells_and_ranks(starts, ends, contig_ids, groups=None, priorities=None):
    """-> (order, cell, rank, sizes): the placed reads in the order of the contract, the dense cell number and the rank
    in its cell of each of them, and the cells' sizes"""
    s = np.asarray(starts, dtype=np.int64)
    e = np.asarray(ends, dtype=np.int64)
    ids = np.asarray(contig_ids, dtype=np.int64)
    n = s.size
    g = np.zeros(n, np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    q = np.zeros(n, np.int64) if priorities is None else np.asarray(priorities, dtype=np.int64)
    units = np.flatnonzero(ids != NO_CONTIG)
    order = units[np.lexsort((units, -(e - s)[units], -q[units], g[units], s[units], ids[units]))]
    if order.size == 0:
        z = np.zeros(0, np.int64)
        return order, z, z, z
    k = np.stack([ids[order], s[order], g[order]], axis=1)
    head = np.ones(order.size, dtype=bool)
    head[1:] = (k[1:] != k[:-1]).any(axis=1)
    at = np.flatnonzero(head)
    cell = np.cumsum(head) - 1
    rank = np.arange(order.size) - at[cell]
    sizes = np.diff(np.concatenate([at, [order.size]]))
    return order, cell, rank, sizes


def depth(starts, ends, contig_ids, contig_lengths, on):
    """per contig, the depth of the reads whose bit in `on` is set -> one int64 array over the concatenated contigs"""
    lengths = np.asarray(contig_lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lengths)])
    ids = np.asarray(contig_ids, dtype=np.int64)
    take = np.flatnonzero(on & (ids != NO_CONTIG))
    ev = np.zeros(off[-1] + 1, dtype=np.int64)
    np.add.at(ev, off[ids[take]] + np.asarray(starts, dtype=np.int64)[take], 1)
    np.add.at(ev, off[ids[take]] + np.asarray(ends, dtype=np.int64)[take] + 1, -1)
    return np.cumsum(ev)[:-1]


def start_cap(oracle, starts, ends, contig_ids, contig_lengths, M, cap, groups=None, priorities=None, shortfall=False,
              hist_bins=0, by_contig=None):
    """-> (keep bits, capped bits, stats dict, hist): bool arrays in input order.  by_contig(starts, ends, ids, lengths,
    M) -> packed mask replaces the oracle's by-contig selection where the oracle cannot go"""
    s = np.asarray(starts, dtype=np.int64)
    e = np.asarray(ends, dtype=np.int64)
    ids = np.asarray(contig_ids, dtype=np.int64)
    n = s.size
    assert cap >= 1
    order, cell, rank, sizes = cells_and_ranks(s, e, ids, groups, priorities)
    survive = np.zeros(n, dtype=bool)
    capped = np.zeros(n, dtype=bool)
    survive[order[rank < cap]] = True
    capped[order[rank >= cap]] = True
    keep = np.zeros(n, dtype=bool)
    on = np.flatnonzero(survive)
    if on.size:
        cols = (s[on].astype(np.uint32), e[on].astype(np.uint32), ids[on].astype(np.uint32))
        m = by_contig(*cols, contig_lengths, M) if by_contig else mr.oracle_by_contig(oracle, *cols, contig_lengths, M)
        keep[on[unpack(m, on.size)]] = True
    kept_per_cell = np.bincount(cell[keep[order]], minlength=sizes.size) if order.size else np.zeros(0, np.int64)
    hist = np.zeros(hist_bins, dtype=np.uint64)
    if hist_bins:
        np.add.at(hist, np.minimum(sizes, hist_bins) - 1, 1)
    short_positions = short_bases = 0
    if shortfall:
        want = np.minimum(depth(s, e, ids, contig_lengths, np.ones(n, bool)), M)
        lack = np.maximum(want - depth(s, e, ids, contig_lengths, keep), 0)
        short_positions, short_bases = int((lack > 0).sum()), int(lack.sum())
    stats = dict(reads_placed=int(order.size), cells=int(sizes.size), cells_over_cap=int((sizes > cap).sum()),
                 reads_capped=int(capped.sum()), largest_cell=int(sizes.max()) if sizes.size else 0,
                 reads_survived=int(survive.sum()), cells_kept=int((kept_per_cell > 0).sum()),
                 largest_kept_cell=int(kept_per_cell.max()) if kept_per_cell.size else 0,
                 short_positions=short_positions, short_bases=short_bases)
    return keep, capped, stats, hist


def key_bits(starts, ends, contig_ids, contig_lengths, groups=None, priorities=None):
    """the width of the sort key the entry builds from the call's own ranges: span, priority, group, gstart"""
    s = np.asarray(starts, dtype=np.int64)
    e = np.asarray(ends, dtype=np.int64)
    placed = np.asarray(contig_ids, dtype=np.int64) != NO_CONTIG
    w = lambda col: int(col[placed].max() - col[placed].min()).bit_length() if placed.any() else 0
    total = int(np.asarray(contig_lengths, dtype=np.int64).sum())
    return (w(e - s) + (0 if priorities is None else w(np.asarray(priorities, dtype=np.int64)))
            + (0 if groups is None else w(np.asarray(groups, dtype=np.int64))) + total.bit_length())
