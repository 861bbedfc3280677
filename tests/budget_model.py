"""Budget downsampling restated on the CPU oracle and numpy (qmcp_hip_solve_budget_*): count(M) is the popcount of the
by-contig oracle's mask at M (tests/multi_reference.py), after pair completion in numpy when asked; the answer to a
budget is a coverage M* in 0 .. top with count(M*) <= budget and (M* == top or count(M* + 1) > budget).  Nothing here
knows the library's planner: `answers` is brute force over every coverage, `largest` a plain bisection for the inputs
whose 0 .. top is too long for that (it leans on the monotonicity that test_budget_cpu.py checks)."""
import numpy as np

import multi_reference as mr

NO_CONTIG = mr.NO_CONTIG
CURVE_MAX = 8191


def unpack(mask, n):
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[:n].astype(bool)


def pack(bits):
    n = bits.size
    out = np.zeros(((n + 63) // 64) * 64, dtype=np.uint8)
    out[:n] = bits
    return np.packbits(out, bitorder="little").view(np.uint64)[:(n + 63) // 64].copy()


def depth(starts, ends, contig_ids, lengths):
    """the depth of the placed reads at every position of every contig, contigs one after the other"""
    lengths = np.atleast_1d(np.asarray(lengths, dtype=np.int64))
    ids = np.asarray(contig_ids, dtype=np.uint32)
    base = np.concatenate([[0], np.cumsum(lengths)])
    on = ids != NO_CONTIG
    diff = np.zeros(int(base[-1]) + 1, dtype=np.int64)
    g = base[ids[on].astype(np.int64)]
    np.add.at(diff, g + np.asarray(starts, dtype=np.int64)[on], 1)
    np.add.at(diff, g + np.asarray(ends, dtype=np.int64)[on] + 1, -1)
    return np.cumsum(diff)[:-1]


def complete_pairs(bits, contig_ids):
    """reads (2q, 2q + 1) are pair q: a placed read is also kept when its placed mate is"""
    placed = np.asarray(contig_ids, dtype=np.uint32) != NO_CONTIG
    pair = (bits[0::2] | bits[1::2]).repeat(2)
    return pair & placed


class Model:
    def __init__(self, oracle, starts, ends, contig_ids, lengths, max_coverage, whole_pairs=False):
        self.oracle, self.s, self.e = oracle, np.asarray(starts, np.uint32), np.asarray(ends, np.uint32)
        self.ids, self.lengths = np.asarray(contig_ids, np.uint32), np.atleast_1d(np.asarray(lengths, np.uint32))
        self.n, self.whole_pairs = self.s.size, whole_pairs
        assert not whole_pairs or self.n % 2 == 0
        self.cov = depth(self.s, self.e, self.ids, self.lengths)
        self.placed = int(np.count_nonzero(self.ids != NO_CONTIG))
        self.max_depth = int(self.cov.max()) if self.cov.size else 0
        self.total_bases = int(self.cov.sum())
        self.top = min(int(max_coverage), self.max_depth)
        self._bits = {}

    def bits(self, M):
        if M not in self._bits:
            if M == 0:
                b = np.zeros(self.n, bool)
            else:
                b = unpack(mr.oracle_by_contig(self.oracle, self.s, self.e, self.ids, self.lengths, M), self.n)
                if self.whole_pairs:
                    b = complete_pairs(b, self.ids)
            self._bits[M] = b
        return self._bits[M]

    def mask(self, M):
        return pack(self.bits(M))

    def count(self, M):
        return int(self.bits(M).sum())

    def curve(self, capacity=CURVE_MAX + 1):
        """S(M) = sum of min(cov, M) for M = 0 .. min(top, CURVE_MAX, capacity - 1), from the definition"""
        last = min(self.top, CURVE_MAX, capacity - 1)
        return np.array([int(np.minimum(self.cov, M).sum()) for M in range(last + 1)], dtype=np.uint64)

    def all_counts(self):
        return np.array([self.count(M) for M in range(self.top + 1)], dtype=np.int64)

    def answers(self, budget):
        """every coverage with properties (1) and (2), by brute force over 0 .. top"""
        c = self.all_counts()
        return [M for M in range(self.top + 1) if c[M] <= budget and (M == self.top or c[M + 1] > budget)]

    def largest(self, budget):
        """the largest coverage in 0 .. top with count <= budget, by bisection (count monotone: no flag)"""
        lo, hi = 0, self.top + 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if self.count(mid) <= budget:
                lo = mid
            else:
                hi = mid
        return lo


def probe_limit(top):
    """2 * ceil(log2(top + 1)) + 2"""
    return 2 * int(top).bit_length() + 2   # ceil(log2(x)) == (x - 1).bit_length()
