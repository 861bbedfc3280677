"""Ceiling downsampling (qmcp_hip_solve_ceiling_*), restated for the tests on top of profile_model.
kept(p) <= cap(p) everywhere is dropped(p) >= max(0, cov(p) - cap(p)), and keeping the most reads is dropping the fewest:
the dropped set D of a contig is profile_model's canonical selection under the cap array max(cov - cap, 0) (its need is
min(cov, that array), which is that array), and the answer is every placed read outside D.
  dual_caps       per contig (cov, cap, max(cov - cap, 0)) of its placed reads
  dual_regions    the dual cap arrays as one CSR table (profile_model.regions_of per contig): what solve_profile takes to
                  select D by its own route
  dropped_bits    D, one bool per read, through profile_model.select (fast=True: fast_select, from sorted events)
  expected_mask   placed and not in D, packed in input order; whole_pairs: a read whose mate (2q, 2q + 1) is in D joins D
  stats           every field of qmcp_hip_ceiling_stats but the time, in numpy
  brute_maximum   the most reads of one contig with cov_F <= cap everywhere (all subsets at once; <= ~16 reads)"""
import numpy as np

import profile_model as pm

NO_CONTIG = pm.NO_CONTIG


def dual_caps(starts, ends, contig_ids, contig_lengths, default_cap, offs=None, r0=None, r1=None, caps=None):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    out = []
    for c, cap in enumerate(pm.cap_arrays(contig_lengths, default_cap, offs, r0, r1, caps)):
        sel = ids == c
        cov = pm.coverage(s[sel], e[sel], cap.size)
        out.append((cov, cap, np.maximum(cov - cap, 0)))
    return out


def dual_regions(starts, ends, contig_ids, contig_lengths, default_cap, offs=None, r0=None, r1=None, caps=None):
    o, a, b, c = [0], [], [], []
    for _, _, dual in dual_caps(starts, ends, contig_ids, contig_lengths, default_cap, offs, r0, r1, caps):
        if dual.size:
            _, x, y, z = pm.regions_of(dual)
            a.append(x); b.append(y); c.append(z)
        o.append(o[-1] + (a[-1].size if dual.size else 0))
    u = lambda parts: np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
    return np.array(o, np.uint32), u(a), u(b), u(c)


def dropped_bits(starts, ends, contig_ids, contig_lengths, default_cap, offs=None, r0=None, r1=None, caps=None, fast=False):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    D = np.zeros(s.size, bool)
    for c, (_, _, dual) in enumerate(dual_caps(s, e, ids, contig_lengths, default_cap, offs, r0, r1, caps)):
        sel = np.flatnonzero(ids == c)
        if sel.size == 0:
            continue
        if fast:
            _, x, y, z = pm.regions_of(dual)
            D[sel] = pm.fast_select(s[sel], e[sel], dual.size, 0, list(zip(x.tolist(), y.tolist(), z.tolist())))
        else:
            D[sel] = pm.select(s[sel], e[sel], dual)
    return D


def with_mates(D):
    """D with the mate (reads 2q, 2q + 1) of each of its reads"""
    pairs = D.reshape(-1, 2)
    return np.repeat(pairs[:, 0] | pairs[:, 1], 2)


def expected_mask(starts, ends, contig_ids, contig_lengths, default_cap, offs=None, r0=None, r1=None, caps=None,
                  whole_pairs=False, fast=False):
    D = dropped_bits(starts, ends, contig_ids, contig_lengths, default_cap, offs, r0, r1, caps, fast)
    if whole_pairs:
        D = with_mates(D)
    placed = np.asarray(contig_ids, np.int64) != NO_CONTIG
    return pm.pack(placed & ~D)


def stats(starts, ends, contig_ids, contig_lengths, default_cap, offs=None, r0=None, r1=None, caps=None, whole_pairs=False,
          fast=False):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    lengths = np.atleast_1d(contig_lengths).tolist()
    D = dropped_bits(s, e, ids, lengths, default_cap, offs, r0, r1, caps, fast)
    final = with_mates(D) if whole_pairs else D
    placed = ids != NO_CONTIG
    out = {"reads_placed": int(placed.sum()), "reads_dropped": int((placed & final).sum()),
           "mates_dropped": int((placed & final & ~D).sum()), "over_positions": 0, "over_bases": 0, "short_positions": 0,
           "short_bases": 0, "excess_positions": 0, "max_kept_depth": 0}
    for c, (cov, cap, dual) in enumerate(dual_caps(s, e, ids, lengths, default_cap, offs, r0, r1, caps)):
        sel = (ids == c) & ~D                                                    # the solve's own mask: before the mates
        kept = pm.coverage(s[sel], e[sel], cap.size)
        floor = np.minimum(cov, cap)
        out["over_positions"] += int((dual > 0).sum())
        out["over_bases"] += int(dual.sum())
        out["short_positions"] += int((kept < floor).sum())
        out["short_bases"] += int(np.maximum(floor - kept, 0).sum())
        out["excess_positions"] += int((kept > cap).sum())
        out["max_kept_depth"] = max(out["max_kept_depth"], int(kept.max()) if kept.size else 0)
    out["regions_in"] = 0 if offs is None else int(np.asarray(offs)[-1])
    out["regions_used"] = 0 if offs is None else sum(
        int(r0[k]) < lengths[c] for c in range(len(lengths)) for k in range(int(offs[c]), int(offs[c + 1])))
    return out


def brute_maximum(starts, ends, cap):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    n, L = s.size, cap.size
    pos = np.arange(L)
    covers = ((s[:, None] <= pos[None, :]) & (e[:, None] >= pos[None, :])).astype(np.int64)   # reads x positions
    subsets = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.int64)     # subsets x reads
    ok = np.all(subsets @ covers <= np.asarray(cap, np.int64)[None, :], axis=1)
    return int(subsets.sum(axis=1)[ok].max())
