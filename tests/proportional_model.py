"""Proportional downsampling (qmcp_hip_solve_proportional_*), restated for the tests: the canonical selection rule of
tests/profile_model.py under a need that comes from the data's own depth, in Python integers throughout.
  quota           ceil(cov * num / den)
  need_of         min(cov, M, max(quota, floor)) for one depth
  need_array      one contig's need per position from its reads
  need_arrays     every contig's (cov, need)
  expected_mask   every contig's reads in input order through profile_model.select (or fast_select on the need's runs),
                  packed in input order
  region_table    the CSR region table (default cap 0) that spells the need out for qmcp_hip_solve_profile_*
  stats           every counter of qmcp_hip_proportional_stats for a mask"""
import numpy as np

import profile_model as pm

NO_CONTIG = 0xFFFFFFFF
NO_LIMIT = (1 << 31) - 1


def quota(cov, num, den):
    return -((-int(cov) * int(num)) // int(den))


def need_of(cov, num, den, floor, M):
    return min(int(cov), int(M), max(quota(cov, num, den), int(floor)))


def need_array(starts, ends, L, num, den, floor, M):
    cov = pm.coverage(np.asarray(starts, np.int64), np.asarray(ends, np.int64), L)
    return cov, np.array([need_of(c, num, den, floor, M) for c in cov.tolist()], np.int64).reshape(L)


def need_arrays(starts, ends, contig_ids, contig_lengths, num, den, floor, M):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    out = []
    for c, L in enumerate(np.atleast_1d(contig_lengths).tolist()):
        sel = ids == c
        out.append(need_array(s[sel], e[sel], L, num, den, floor, M))
    return out


def expected_mask(starts, ends, contig_ids, contig_lengths, num, den, floor=0, M=NO_LIMIT, fast=False):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    bits = np.zeros(s.size, bool)
    for c, (_, need) in enumerate(need_arrays(s, e, ids, contig_lengths, num, den, floor, M)):
        sel = np.flatnonzero(ids == c)
        if sel.size == 0:
            continue
        if fast:
            _, r0, r1, caps = pm.regions_of(need)
            bits[sel] = pm.fast_select(s[sel], e[sel], need.size, 0, sorted(zip(r0.tolist(), r1.tolist(), caps.tolist())))
        else:
            bits[sel] = pm.select(s[sel], e[sel], need)
    return pm.pack(bits)


def region_table(starts, ends, contig_ids, contig_lengths, num, den, floor=0, M=NO_LIMIT):
    """(offs, r0, r1, caps): one region per run of equal need on every contig; use with default_cap 0"""
    offs, r0, r1, caps = [0], [], [], []
    for _, need in need_arrays(starts, ends, contig_ids, contig_lengths, num, den, floor, M):
        count = offs[-1]
        if need.size:
            _, a, b, c = pm.regions_of(need)
            r0.append(a); r1.append(b); caps.append(c)
            count += a.size
        offs.append(count)
    cat = lambda xs: np.concatenate(xs).astype(np.uint32) if xs else np.zeros(0, np.uint32)
    return np.asarray(offs, np.uint32), cat(r0), cat(r1), cat(caps)


def stats(starts, ends, contig_ids, contig_lengths, num, den, floor, M, mask):
    """the counters of qmcp_hip_proportional_stats on the capped route (plain_route == 0)"""
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ids = np.asarray(contig_ids, np.int64)
    placed = ids != NO_CONTIG
    kept = pm.unpack(mask, s.size)
    out = dict(reads_placed=int(placed.sum()), bases_in=int((e - s + 1)[placed].sum()),
               bases_kept=int((e - s + 1)[kept].sum()), demand=0, whole_positions=0, floor_positions=0,
               capped_positions=0, max_depth=0, max_need=0, num=int(num), den=int(den), floor=int(floor), plain_route=0)
    for cov, need in need_arrays(s, e, ids, contig_lengths, num, den, floor, M):
        for cv, nd in zip(cov.tolist(), need.tolist()):
            q = quota(cv, num, den)
            out["demand"] += nd
            out["whole_positions"] += cv > 0 and nd == cv
            out["floor_positions"] += q < min(int(floor), cv, int(M))
            out["capped_positions"] += max(q, int(floor)) > int(M) and cv > int(M)
            out["max_depth"] = max(out["max_depth"], cv)
            out["max_need"] = max(out["max_need"], nd)
    return out
