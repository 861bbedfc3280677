"""Coverage profile (qmcp_hip_solve_profile_*), restated for the tests: the canonical selection rule with a cap ARRAY.
  cap_arrays      per contig, cap(p): default_cap, overwritten inside each region (clipped; dropped beyond the contig)
  select          one contig, reads in input order: at the leftmost position with a deficit against
                  need(p) = min(cov(p), cap(p)), take the unselected covering reads with the furthest end, then the
                  furthest start, then the lowest index
  expected_mask   every contig's reads in input order through select, packed in input order
  brute_minimum   the fewest reads that satisfy cov_F >= need everywhere (all subsets at once; <= ~16 reads)
  demand_and_capped   the two counters k_profile_need reduces, over the contigs given"""
import numpy as np

NO_CONTIG = 0xFFFFFFFF


def cap_arrays(contig_lengths, default_cap, offs=None, r0=None, r1=None, caps=None):
    out = []
    for c, L in enumerate(np.atleast_1d(contig_lengths).tolist()):
        cap = np.full(L, int(default_cap), np.int64)
        if offs is not None:
            for k in range(int(offs[c]), int(offs[c + 1])):
                if int(r0[k]) < L:
                    cap[int(r0[k]):min(int(r1[k]), L - 1) + 1] = int(caps[k])
        out.append(cap)
    return out


def coverage(s, e, L):
    diff = np.zeros(L + 1, np.int64)
    np.add.at(diff, s, 1)
    np.add.at(diff, e + 1, -1)
    return np.cumsum(diff)[:L]


def select(starts, ends, cap):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    L = cap.size
    need = np.minimum(coverage(s, e, L), cap)
    kept = np.zeros(s.size, bool)
    have = np.zeros(L, np.int64)
    for p in np.flatnonzero(need > 0).tolist():
        d = int(need[p] - have[p])
        if d <= 0:
            continue
        cand = np.flatnonzero(~kept & (s <= p) & (e >= p))
        take = cand[np.lexsort((cand, -s[cand], -e[cand]))[:d]]
        kept[take] = True
        for i in take.tolist():
            have[s[i]:e[i] + 1] += 1
    return kept


def pack(bits):
    n = bits.size
    padded = np.zeros(((n + 63) // 64) * 64, np.uint8)
    padded[:n] = bits
    return np.packbits(padded, bitorder="little").view(np.uint64)[:(n + 63) // 64].copy()


def unpack(mask, n):
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[:n].astype(bool)


def expected_mask(starts, ends, contig_ids, contig_lengths, default_cap, offs=None, r0=None, r1=None, caps=None):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    bits = np.zeros(s.size, bool)
    for c, cap in enumerate(cap_arrays(contig_lengths, default_cap, offs, r0, r1, caps)):
        sel = np.flatnonzero(ids == c)
        if sel.size:
            bits[sel] = select(s[sel], e[sel], cap)
    return pack(bits)


def is_valid(starts, ends, cap, kept):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    need = np.minimum(coverage(s, e, cap.size), cap)
    return bool(np.all(coverage(s[kept], e[kept], cap.size) >= need))


def brute_minimum(starts, ends, cap):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    n, L = s.size, cap.size
    pos = np.arange(L)
    covers = ((s[:, None] <= pos[None, :]) & (e[:, None] >= pos[None, :])).astype(np.int64)   # reads x positions
    need = np.minimum(covers.sum(axis=0), cap)
    subsets = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.int64)     # subsets x reads
    ok = np.all(subsets @ covers >= need[None, :], axis=1)
    return int(subsets.sum(axis=1)[ok].min())


def demand_and_capped(starts, ends, contig_ids, contig_lengths, default_cap, offs, r0, r1, caps, contigs=None):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    demand = capped = 0
    for c, cap in enumerate(cap_arrays(contig_lengths, default_cap, offs, r0, r1, caps)):
        if contigs is not None and c not in contigs:
            continue
        sel = ids == c
        cov = coverage(s[sel], e[sel], cap.size)
        demand += int(np.minimum(cov, cap).sum())
        capped += int((cov > cap).sum())
    return demand, capped


def random_regions(rng, lengths, max_cap, max_regions=5, zero_run=0):
    """disjoint CSR regions per contig with caps 0..max_cap: edges at multiples of 64 and +-1 where the contig is long
    enough, some reaching beyond the contig (clipped), and -- zero_run > 0 -- one cap-0 run at least that long"""
    offs, r0, r1, caps = [0], [], [], []
    for L in np.atleast_1d(lengths).tolist():
        edges = set()
        for _ in range(int(rng.integers(0, 2 * max_regions + 1))):
            x = int(rng.integers(0, max(L, 1)))
            if rng.random() < 0.5 and L > 64:
                x = min(max(64 * int(rng.integers(0, L // 64 + 1)) + int(rng.integers(-1, 2)), 0), L - 1)
            edges.add(x)
        edges = sorted(edges)
        regs = []
        for a, b in zip(edges[0::2], edges[1::2]):
            regs.append([a, b - 1 if b - 1 >= a else a, int(rng.integers(0, max_cap + 1))])
        if regs and rng.random() < 0.3:
            regs[-1][1] = L + int(rng.integers(0, 40))                                   # clipped to the contig
        if zero_run and L > zero_run + 2:
            a = int(rng.integers(0, L - zero_run))
            regs = [r for r in regs if r[1] < a or r[0] > a + zero_run] + [[a, a + zero_run, 0]]
        order = rng.permutation(len(regs))                                               # the order is free
        for k in order.tolist():
            r0.append(regs[k][0]); r1.append(regs[k][1]); caps.append(regs[k][2])
        offs.append(len(r0))
    return (np.array(offs, np.uint32), np.array(r0, np.uint32), np.array(r1, np.uint32), np.array(caps, np.uint32))
