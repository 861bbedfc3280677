"""Mean-depth downsampling restated on the CPU oracle and numpy (qmcp_hip_solve_mean_depth_*), on top of
tests/budget_model.py: bases(M) is the depth of the oracle's mask at M (after pair completion when asked) summed over the
positions of R, and R is a membership array painted from the RAW regions one by one -- nothing here merges, sorts or
projects, and nothing knows the library's target table or planner.  `answers` is brute force over every coverage."""
import numpy as np

import budget_model as bm

NO_CONTIG = bm.NO_CONTIG
CURVE_MAX = bm.CURVE_MAX


def membership(lengths, region_offsets, region_starts, region_ends):
    """one bool per position, contigs one after the other: inside some region of its contig (inclusive bounds, clipped
    to the contig; a region that begins at or beyond the contig's length touches nothing).  No table: everything"""
    lengths = np.atleast_1d(np.asarray(lengths, dtype=np.int64))
    base = np.concatenate([[0], np.cumsum(lengths)])
    if region_offsets is None:
        return np.ones(int(base[-1]), bool)
    inside = np.zeros(int(base[-1]), bool)
    for c in range(lengths.size):
        for k in range(int(region_offsets[c]), int(region_offsets[c + 1])):
            s, e = int(region_starts[k]), int(region_ends[k])
            assert s <= e
            inside[base[c] + min(s, lengths[c]):base[c] + min(e + 1, lengths[c])] = True
    return inside


def random_regions(rng, lengths):
    """zero to four regions per contig: overlapping, nested, one reaching the contig's last position, one starting beyond
    the contig, and contigs without any -> (offsets, starts, ends), in no particular order within a contig"""
    offs, r0, r1 = [0], [], []
    for c, length in enumerate(np.asarray(lengths, dtype=np.int64).tolist()):
        regs = []
        if length > 0 and rng.random() < 0.8:
            for _ in range(int(rng.integers(1, 4))):
                s = int(rng.integers(0, length))
                regs.append((s, s + int(rng.integers(0, max(length // 3, 1)))))       # may run past the end: clipped
            s, e = regs[0]
            if e - s >= 2:
                regs.append((s + 1, e - 1))                                           # nested
            kind = int(rng.integers(0, 3))
            if kind == 0:
                regs.append((max(length - 1 - int(rng.integers(0, 50)), 0), length - 1))  # ends on the last position
            elif kind == 1:
                regs.append((length + int(rng.integers(0, 5)), length + 100))         # begins beyond the contig
            regs = [regs[i] for i in rng.permutation(len(regs))][:4]
        r0 += [s for s, _ in regs]
        r1 += [e for _, e in regs]
        offs.append(len(r0))
    return np.array(offs, np.uint32), np.array(r0, np.uint32), np.array(r1, np.uint32)


class Model(bm.Model):
    def __init__(self, oracle, starts, ends, contig_ids, lengths, max_coverage, regions=None, whole_pairs=False):
        super().__init__(oracle, starts, ends, contig_ids, lengths, max_coverage, whole_pairs=whole_pairs)
        offs, r0, r1 = regions if regions is not None else (None, None, None)
        self.inside = membership(self.lengths, offs, r0, r1)
        self.positions = int(self.inside.sum())
        self.total_bases = int(self.cov[self.inside].sum())      # over R (bm.Model's is over everything)
        self._bases = {}

    def bases(self, M):
        """the kept depth at M summed over the positions of R"""
        if M not in self._bases:
            b = self.bits(M)
            kept = bm.depth(self.s[b], self.e[b], self.ids[b], self.lengths)
            self._bases[M] = int(kept[self.inside].sum())
        return self._bases[M]

    def curve_R(self, capacity=CURVE_MAX + 1):
        """S_R(M) = sum over R of min(cov, M) for M = 0 .. min(top, CURVE_MAX, capacity - 1), from the definition"""
        last = min(self.top, CURVE_MAX, capacity - 1)
        cov = self.cov[self.inside]
        return np.array([int(np.minimum(cov, M).sum()) for M in range(last + 1)], dtype=np.uint64)

    def all_bases(self):
        return np.array([self.bases(M) for M in range(self.top + 1)], dtype=np.int64)

    def answers(self, budget):
        """every coverage with properties (1) and (2), by brute force over 0 .. top"""
        b = self.all_bases()
        return [M for M in range(self.top + 1) if b[M] <= budget and (M == self.top or b[M + 1] > budget)]

    def largest(self, budget):
        """the largest coverage in 0 .. top with bases <= budget by bisection (where bases is monotone)"""
        lo, hi = 0, self.top + 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if self.bases(mid) <= budget else (lo, mid)
        return lo
