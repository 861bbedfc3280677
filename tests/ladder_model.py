"""The coverage ladder (qmcp_hip_solve_ladder_*) restated on the oracle: level 0 is the per-contig canonical selection
of all reads (multi_reference.oracle_by_contig), level j + 1 the same selection of the reads level j kept, alone, in
input order with their contig ids.  The result is one byte per read: the number of levels that keep it."""
import numpy as np

import multi_reference as mr


def ladder_levels(oracle, starts, ends, contig_ids, contig_lengths, coverages):
    """-> uint8[n_reads]; K_j = {i : levels[i] > j}"""
    s, e = np.asarray(starts, dtype=np.uint32), np.asarray(ends, dtype=np.uint32)
    ids = np.asarray(contig_ids, dtype=np.uint32)
    levels = np.zeros(s.size, dtype=np.uint8)
    alive = np.arange(s.size)                      # input indices of the reads the level above kept
    for M in coverages:
        mask = mr.oracle_by_contig(oracle, s[alive], e[alive], ids[alive], contig_lengths, int(M))
        bits = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[:alive.size].astype(bool)
        alive = alive[bits]
        levels[alive] += 1
    return levels


def level_mask(levels, j):
    """the packed input-order mask of K_j"""
    levels = np.asarray(levels, dtype=np.uint8)
    bits = np.zeros(((levels.size + 63) // 64) * 64, dtype=np.uint8)
    bits[:levels.size] = levels > j
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def n_kept(levels, n_levels):
    return [int((np.asarray(levels) > j).sum()) for j in range(n_levels)]
