"""Coverage profile (qmcp_hip_solve_profile_*), restated for the tests: the canonical selection rule with a cap ARRAY.
  cap_arrays      per contig, cap(p): default_cap, overwritten inside each region (clipped; dropped beyond the contig)
  select          one contig, reads in input order: at the leftmost position with a deficit against
                  need(p) = min(cov(p), cap(p)), take the unselected covering reads with the furthest end, then the
                  furthest start, then the lowest index
  expected_mask   every contig's reads in input order through select, packed in input order
  brute_minimum   the fewest reads that satisfy cov_F >= need everywhere (all subsets at once; <= ~16 reads)
  demand_and_capped   the two counters k_profile_need reduces, over the contigs given
A second restatement of the same rule, for axes and tables `select` cannot walk (it is O(positions with need x reads)):
  fast_select         one contig from sorted events: need(p) only changes at a read's start, behind a read's end and at
                      a region's edges, the kept coverage only drops behind a kept read's end, so a deficit can only
                      appear at one of those positions; candidates wait in a heap ordered (end desc, start desc, index)
  fast_expected_mask  expected_mask through fast_select; no array per position anywhere
  compact             the translation helper: reads and regions in a few islands of long contigs, moved to short contigs
                      (the rule is translation-invariant and a stretch without reads decides nothing)
  stretch_windows, form_of   which kernel form the launchers pick for a call, restated from its statistics"""
import heapq

import numpy as np

NO_CONTIG = 0xFFFFFFFF
LDS_RING_LIMIT = 16383          # the longest span whose two rings still fit LDS
NEED_LDS_MAX = 4096             # the most regions k_profile_need stages in LDS


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


# ------------------------------------------------------------------------------------------ the rule from sorted events
def clipped_regions(L, r0, r1, caps):
    """one contig's regions as sorted (start, end, cap) rows, clipped to the contig and dropped beyond it"""
    return sorted((int(a), min(int(b), L - 1), int(c)) for a, b, c in zip(r0, r1, caps) if int(a) < L)


def fast_select(starts, ends, L, default_cap, regions=()):
    """`select` for one contig of L positions under default_cap and sorted disjoint (start, end, cap) rows.  need(p)
    is constant between breakpoints (read starts, read ends + 1, region starts, region ends + 1) and the kept coverage
    only drops at a kept read's end + 1, itself a breakpoint: deficits are looked for at breakpoints only"""
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    kept = np.zeros(s.size, bool)
    if s.size == 0:
        return kept
    regs = np.array(list(regions), np.int64).reshape(-1, 3)
    bp = np.unique(np.concatenate([s, e + 1, regs[:, 0], regs[:, 1] + 1]))
    bp = bp[bp < L]
    cov = np.searchsorted(np.sort(s), bp, side="right") - np.searchsorted(np.sort(e), bp, side="left")
    cap = np.full(bp.size, int(default_cap), np.int64)
    if regs.size:
        k = np.searchsorted(regs[:, 0], bp, side="right") - 1                    # the last region that starts at or before
        inside = (k >= 0) & (regs[np.maximum(k, 0), 1] >= bp)
        cap[inside] = regs[k[inside], 2]
    need = np.minimum(cov, cap).tolist()
    by_start = np.argsort(s, kind="stable").tolist()
    sl, el = s.tolist(), e.tolist()
    waiting, leaving = [], []                # (-end, -start, index) of unkept reads met so far; end + 1 of kept reads
    have = entered = 0
    for p, want in zip(bp.tolist(), need):
        while leaving and leaving[0] <= p:
            heapq.heappop(leaving)
            have -= 1
        while entered < len(by_start) and sl[by_start[entered]] <= p:
            i = by_start[entered]
            heapq.heappush(waiting, (-el[i], -sl[i], i))
            entered += 1
        while have < want:
            neg_end, _, i = heapq.heappop(waiting)                               # the furthest end, start, lowest index
            assert -neg_end >= p, "need <= cov: an unkept read covers p"         # (reads behind p sink below the live ones)
            kept[i] = True
            heapq.heappush(leaving, (-neg_end + 1))
            have += 1
    return kept


def fast_expected_mask(starts, ends, contig_ids, contig_lengths, default_cap, offs=None, r0=None, r1=None, caps=None):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    bits = np.zeros(s.size, bool)
    grouped = np.argsort(ids, kind="stable")
    first = np.searchsorted(ids[grouped], np.arange(len(np.atleast_1d(contig_lengths)) + 1))
    for c, L in enumerate(np.atleast_1d(contig_lengths).tolist()):
        sel = grouped[first[c]:first[c + 1]]                                      # ascending: input order
        if sel.size:
            a, b = (int(offs[c]), int(offs[c + 1])) if offs is not None else (0, 0)
            rows = clipped_regions(L, r0[a:b], r1[a:b], caps[a:b]) if b > a else ()
            bits[sel] = fast_select(s[sel], e[sel], L, default_cap, rows)
    return pack(bits)


def regions_of(cap):
    """a cap array as CSR regions of one contig, one region per run of equal caps"""
    cap = np.asarray(cap, np.int64)
    edges = np.concatenate([[0], np.flatnonzero(np.diff(cap)) + 1, [cap.size]])
    u = lambda x: np.asarray(x, np.uint32)
    return u([0, edges.size - 1]), u(edges[:-1]), u(edges[1:] - 1), u(cap[edges[:-1]])


# ------------------------------------------------------------------------------------------ translation
def compact(starts, ends, contig_ids, contig_lengths, offs=None, r0=None, r1=None, caps=None, gap=1):
    """the same instance on short contigs: per contig the reads' islands (maximal runs of positions under a read, runs
    that touch joined) moved next to one another with `gap` uncovered positions between them; regions are cut to the
    islands, what lies between islands is dropped (no read: need is 0 whatever the cap).  Reads keep their order and
    their contig; unplaced reads keep their coordinates.  Returns starts, ends, contig_ids, contig_lengths, offs, r0,
    r1, caps in the shape the models and the solver take"""
    s, e = np.asarray(starts, np.int64).copy(), np.asarray(ends, np.int64).copy()
    ids = np.asarray(contig_ids, np.int64)
    lengths = np.atleast_1d(contig_lengths).tolist()
    new_len, new_offs, n0, n1, ncap = [], [0], [], [], []
    for c, L in enumerate(lengths):
        sel = np.flatnonzero(ids == c)
        if sel.size == 0:
            new_len.append(min(L, 1))
            new_offs.append(len(n0))
            continue
        order = np.argsort(s[sel], kind="stable")
        ss, ee = s[sel][order], e[sel][order]
        reach = np.maximum.accumulate(ee)
        fresh = np.concatenate([[True], ss[1:] > reach[:-1] + 1])                 # a read that begins a new island
        isl_a = ss[fresh]
        isl_b = reach[np.concatenate([np.flatnonzero(fresh)[1:] - 1, [ss.size - 1]])]
        moved = np.concatenate([[0], np.cumsum(isl_b - isl_a + 1 + gap)[:-1]])    # the island's new first position
        k = np.searchsorted(isl_a, s[sel], side="right") - 1
        shift = moved[k] - isl_a[k]
        s[sel] += shift
        e[sel] += shift
        new_len.append(int(moved[-1] + isl_b[-1] - isl_a[-1] + 1))
        if offs is not None:
            a, b = int(offs[c]), int(offs[c + 1])
            for ra, rb, rc in clipped_regions(L, r0[a:b], r1[a:b], caps[a:b]):
                lo = int(np.searchsorted(isl_b, ra, side="left"))                 # the first island that ends at or behind ra
                hi = int(np.searchsorted(isl_a, rb, side="right"))                # islands before this one begin at or before rb
                for j in range(lo, hi):
                    n0.append(max(ra, int(isl_a[j])) - int(isl_a[j]) + int(moved[j]))
                    n1.append(min(rb, int(isl_b[j])) - int(isl_a[j]) + int(moved[j]))
                    ncap.append(rc)
        new_offs.append(len(n0))
    u = lambda x: np.asarray(x, np.uint32)
    out = (s.astype(np.uint32), e.astype(np.uint32), u(contig_ids), u(new_len))
    if offs is None:
        return out + (None, None, None, None)
    return out + (u(new_offs), u(n0), u(n1), u(ncap))


# ------------------------------------------------------------------------------------------ the form a call takes
def stretch_windows(ltot, max_span, n_contigs):
    """cut-point windows the mixed-span route asks for when cut points are forced on: at least 64 longest spans each,
    none for 256 contigs or more, at most 3 840"""
    if n_contigs >= 256 or max_span == 0:
        return 0
    w = int(ltot) // (64 * int(max_span))
    return 0 if w < 2 else min(w, 3840)


def need_form(n_regions):
    return "need_lds" if n_regions <= NEED_LDS_MAX else "need_global"


def form_of(stats, n_contigs, cut_points):
    """which capped sweep one batch took, from its statistics (sort_passes, max_span, total_length) and the cut_points
    setting it ran under (-1: one workgroup per contig; 1: per contig and window): ("k64" | "rec", "reg", B, K) for
    the register-resident walk with B blocks of 64 buckets per lane and K loader waves, or ("k64" | "rec", "plain",
    "lds" | "global") for the plain walk and where its rings live"""
    if cut_points not in (-1, 1):
        raise ValueError("the library's own choice of windows is not restated here")
    keys = "k64" if stats.sort_passes >= 5 else "rec"
    max_span = int(stats.max_span)
    b = {2: 2, 3: 3, 4: 4, 5: 6, 6: 6, 7: 8, 8: 8}.get(max((max_span + 127) // 64, 2))
    if b is None:
        return (keys, "plain", "global" if max_span > LDS_RING_LIMIT else "lds")
    n_wg = n_contigs + (stretch_windows(stats.total_length, max_span, n_contigs) if cut_points > 0 else 0)
    return (keys, "reg", b, 4 if n_wg <= 64 else 1)
