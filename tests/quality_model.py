"""The quality-aware selection of qmcp_hip_solve_quality_*, restated two ways (tests only):
  quality_choice  the contract: in every (contig, start, end) cell keep as many reads as the plain mask keeps there,
                  the first ones in the order (quality descending, read index ascending)
  greedy_quality  the canonical greedy of the oracle's selection (sweep positions, take the live read of largest end,
                  then largest start, ...) with its last key "smallest index" replaced by "highest quality, then
                  smallest index" -- written from the rule, for small inputs only"""
import heapq

import numpy as np

NO_CONTIG = 0xFFFFFFFF


def bits_of(mask, n):
    return np.unpackbits(np.ascontiguousarray(mask, dtype=np.uint64).view(np.uint8), bitorder="little")[:n].astype(bool)


def mask_of(bits):
    n = bits.size
    padded = np.zeros(((n + 63) // 64) * 64, np.uint8)
    padded[:n] = bits
    return np.packbits(padded, bitorder="little").view(np.uint64).copy()


def quality_choice(plain_mask, starts, ends, contig, q):
    """keep mask of the contract; contig may be None (one contig).  Reads with contig NO_CONTIG form a cell of their
    own (the plain mask never keeps them)"""
    s = np.asarray(starts, np.int64)
    n = s.size
    if n == 0:
        return mask_of(np.zeros(0, bool))
    e = np.asarray(ends, np.int64)
    c = np.zeros(n, np.int64) if contig is None else np.asarray(contig, np.int64)
    qq = np.asarray(q, np.int64)
    K = bits_of(plain_mask, n)
    unplaced = c == NO_CONTIG
    s = np.where(unplaced, 0, s)
    e = np.where(unplaced, 0, e)
    order = np.lexsort((np.arange(n), -qq, e, s, c))          # last key first: contig, start, end, -q, index
    cs, ss, es = c[order], s[order], e[order]
    head = np.ones(n, bool)
    head[1:] = (cs[1:] != cs[:-1]) | (ss[1:] != ss[:-1]) | (es[1:] != es[:-1])
    heads = np.flatnonzero(head)
    seg = np.cumsum(head) - 1
    rank = np.arange(n) - heads[seg]
    kept_in_cell = np.add.reduceat(K[order].astype(np.int64), heads)
    keep = np.zeros(n, bool)
    keep[order] = rank < kept_in_cell[seg]
    return mask_of(keep)


def greedy_quality(starts, ends, L, M, q):
    """one contig of length L: the canonical sweep with the four-key order; -> keep mask"""
    s = np.asarray(starts, np.int64)
    e = np.asarray(ends, np.int64)
    qq = np.asarray(q, np.int64)
    n = s.size
    diff = np.zeros(L + 1, np.int64)
    np.add.at(diff, s, 1)
    np.add.at(diff, e + 1, -1)
    need = np.minimum(np.cumsum(diff)[:L], M)
    by_start = [[] for _ in range(L)]
    for i in range(n):
        by_start[s[i]].append(i)
    expire = np.zeros(L + 1, np.int64)
    keep = np.zeros(n, bool)
    heap, cov = [], 0
    for p in range(L):
        for i in by_start[p]:
            heapq.heappush(heap, (-e[i], -s[i], -qq[i], i))
        deficit = need[p] - cov
        while deficit > 0:
            _, _, _, r = heapq.heappop(heap)
            if e[r] < p:
                continue
            keep[r] = True
            expire[e[r]] += 1
            cov += 1
            deficit -= 1
        cov -= expire[p]
    return keep


def greedy_quality_multi(starts, ends, lengths, offs, M, q):
    """contigs grouped by offs (n_contigs + 1 read offsets): each swept on its own"""
    n = len(starts)
    keep = np.zeros(n, bool)
    for k in range(len(lengths)):
        a, b = int(offs[k]), int(offs[k + 1])
        keep[a:b] = greedy_quality(starts[a:b], ends[a:b], int(lengths[k]), M, q[a:b])
    return mask_of(keep)


def contig_of(offs, n):
    """the contig of every read of a grouped call"""
    return np.repeat(np.arange(len(offs) - 1), np.diff(np.asarray(offs, np.int64)))
