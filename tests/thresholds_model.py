"""Coverage thresholds restated on the CPU oracle and numpy (qmcp_hip_solve_thresholds_*).  keep_M is budget_model's
Model.bits(M) WITHOUT pair completion: the by-contig oracle's mask at M.  Everything here is brute force from the
definitions in include/qmcp_hip.h: M ascends from lo, a read's threshold is the first M that keeps it, solving stops
after the first M at which every placed read has one (or at hi), a violation is a (read, M) pair in which a read with a
threshold is not kept, the pair minimum is taken among placed mates, the counts are the final thresholds' <= M."""
import numpy as np

import budget_model as bm

NO_CONTIG = bm.NO_CONTIG
NEVER = 0xFFFF


def pair_minimum(thresholds, contig_ids):
    """reads (2q, 2q + 1) are pair q: a placed read takes the smaller of its own and its placed mate's threshold; an
    unplaced read lends nothing and stays NEVER"""
    t = np.asarray(thresholds, np.uint16)
    placed = np.asarray(contig_ids, np.uint32) != NO_CONTIG
    lend = np.where(placed, t, NEVER).astype(np.uint16)          # what a read offers its mate
    mate = lend.reshape(-1, 2)[:, ::-1].reshape(-1)
    return np.where(placed, np.minimum(t, mate), NEVER).astype(np.uint16)


class Thresholds:
    """the answer of one call: thresholds (uint16), top, solves, saturated, violations, n_kept, counts(capacity)"""

    def __init__(self, oracle, starts, ends, contig_ids, lengths, lo, hi, whole_pairs=False):
        assert 1 <= lo <= hi <= NEVER - 1
        self.model = bm.Model(oracle, starts, ends, contig_ids, lengths, hi)
        m = self.model
        self.lo, self.hi, self.n = lo, hi, m.n
        placed = m.ids != NO_CONTIG
        t = np.full(m.n, NEVER, np.uint16)
        seen = np.zeros(m.n, bool)
        self.violations = 0
        M = lo
        while True:
            keep = m.bits(M)
            assert not keep[~placed].any()
            self.violations += int((seen & ~keep).sum())
            t[keep & ~seen] = M
            seen |= keep
            if seen[placed].all() or M == hi:
                break
            M += 1
        self.top, self.solves = M, M - lo + 1
        self.saturated = 1 if seen[placed].all() else 0
        self.own = t.copy()                                        # before the pair minimum
        self.thresholds = pair_minimum(t, m.ids) if whole_pairs else t
        self.n_kept = int((self.thresholds <= hi).sum())

    def counts(self, capacity=None):
        last = self.hi if capacity is None else min(self.hi, self.lo + capacity - 1)
        return np.array([int((self.thresholds <= M).sum()) for M in range(self.lo, last + 1)], dtype=np.uint64)

    def bits(self, M):
        """what thresholds <= M selects"""
        return self.thresholds <= M
