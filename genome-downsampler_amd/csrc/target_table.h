// target_table.h -- the target regions of several contigs as qmcp_hip_solve_targets_* reads them, and the projection of
// one read onto the compressed axis of its contig's target positions.
//
// Plain C++17 (no HIP needed): api/targets.inc.hip includes it, kernels/targets.inc.hip includes it for project_read, and
// so can a host-only test.  The caller gives the regions of each contig in CSR form -- contig c owns
// [offs[c], offs[c + 1]) of starts / ends, inclusive bounds, in any order, overlapping and nested regions allowed.
// The table keeps, per contig, the regions
//   1. padded: [start - padding, end + padding], the start saturating at 0;
//   2. clipped to [0, length - 1]; a region that begins at or beyond length (after padding) is dropped, and a contig
//      of length 0 has none;
//   3. sorted, with overlapping and adjacent (end + 1 == next start) regions merged, so that the merged regions of a
//      contig are disjoint, ascending and separated by at least one position;
// and cum[k], the number of target positions of the contig before merged region k.  T_c is the union of contig c's
// merged regions, |T_c| = tlen[c], rank_c(p) = |{t in T_c : t < p}|.  A read [s, e] on c covers a contiguous run of T_c
// in rank order: it projects to [rank_c(s), rank_c(e + 1) - 1], and is OFF-TARGET when that interval is empty.
#ifndef QMCP_TARGET_TABLE_H
#define QMCP_TARGET_TABLE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define QMCP_HD __host__ __device__
#else
#define QMCP_HD
#endif

namespace qmcp {

// The projection of the read [s, e] (s <= e) onto the merged regions [lo, hi) of its contig: rs / re the regions'
// inclusive bounds, cum the target positions of the contig before each.  Two binary searches: k, the first region with
// end >= s, and j, the last with start <= e.  The read is on target iff k <= j; then
//   *cs = cum[k] + max(s, rs[k]) - rs[k]   (= rank(s):          positions before region k, plus those of k before s)
//   *ce = cum[j] + min(e, re[j]) - rs[j]   (= rank(e + 1) - 1:  the last target position at or before e)
// The kernel and the host (tests/cpp/target_table_driver.cpp) share this one definition.
QMCP_HD inline bool project_read(const uint32_t* rs, const uint32_t* re, const uint32_t* cum, uint32_t lo, uint32_t hi,
                                 uint32_t s, uint32_t e, uint32_t* cs, uint32_t* ce) {
    uint32_t a = lo, b = hi;  // the first region with end >= s lies in [a, b]
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (re[m] < s) a = m + 1;
        else b = m;
    }
    const uint32_t k = a;
    b = hi;  // the first region with start > e lies in [a, b]: it is not before k (rs[k'] <= re[k'] < s <= e below k)
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (rs[m] <= e) a = m + 1;
        else b = m;
    }
    if (a == k) return false;  // no region with end >= s and start <= e
    const uint32_t j = a - 1;
    const uint32_t rk = rs[k], rj = rs[j], ej = re[j];
    *cs = cum[k] + (s > rk ? s - rk : 0u);
    *ce = cum[j] + (e < ej ? e : ej) - rj;
    return true;
}

// bit i of the low 16 bits of x -> bit 4 i (the projection kernel interleaves four ballots into keep-mask words)
QMCP_HD inline uint64_t spread_bits_by_4(uint64_t x) {
    x &= 0xFFFFull;
    x = (x | (x << 24)) & 0x000000FF000000FFull;
    x = (x | (x << 12)) & 0x000F000F000F000Full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

}  // namespace qmcp

#include <algorithm>
#include <utility>
#include <vector>

#include "qmcp_hip.h"

namespace qmcp {

struct TargetTable {
    std::vector<uint32_t> offs;          // n_contigs + 1: contig c owns merged regions [offs[c], offs[c + 1])
    std::vector<uint32_t> rs, re, cum;   // per merged region: inclusive bounds, target positions of its contig before it
    std::vector<uint32_t> tlen;          // |T_c| per contig
    uint64_t positions = 0;              // sum of |T_c|
    uint32_t regions_in = 0, regions_merged = 0;
};

// offs has n_contigs + 1 entries: starts at 0 and never decreases.  QMCP_OK or QMCP_EINVAL.
inline int check_target_offsets(const uint32_t* offs, uint32_t n_contigs) {
    if (!offs || offs[0] != 0) return QMCP_EINVAL;
    for (uint32_t c = 0; c < n_contigs; ++c)
        if (offs[c + 1] < offs[c]) return QMCP_EINVAL;
    return QMCP_OK;
}

// QMCP_EINVAL: bad offsets, null tables with a non-zero count, null lengths, a region with start > end.
inline int build_target_table(const uint32_t* offs, const uint32_t* starts, const uint32_t* ends, uint32_t padding,
                              const uint32_t* lengths, uint32_t n_contigs, TargetTable& t) {
    if (!lengths || check_target_offsets(offs, n_contigs) != QMCP_OK) return QMCP_EINVAL;
    const uint32_t n = offs[n_contigs];
    if (n && (!starts || !ends)) return QMCP_EINVAL;
    for (uint32_t k = 0; k < n; ++k)
        if (starts[k] > ends[k]) return QMCP_EINVAL;
    t = TargetTable();
    t.regions_in = n;
    t.offs.assign((size_t)n_contigs + 1, 0);
    t.tlen.assign(n_contigs, 0);
    std::vector<std::pair<uint32_t, uint32_t>> reg;
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const uint32_t len = lengths[c];
        reg.clear();
        for (uint32_t k = offs[c]; k < offs[c + 1]; ++k) {
            const uint32_t s = starts[k] >= padding ? starts[k] - padding : 0u;
            if (s >= len) continue;  // beyond the contig (every region of a contig of length 0)
            const uint64_t e = std::min<uint64_t>((uint64_t)ends[k] + padding, (uint64_t)len - 1);
            reg.emplace_back(s, (uint32_t)e);
        }
        std::sort(reg.begin(), reg.end());
        uint32_t total = 0;
        for (size_t i = 0; i < reg.size();) {
            const uint32_t s = reg[i].first;
            uint32_t e = reg[i].second;
            size_t k = i + 1;
            while (k < reg.size() && (uint64_t)reg[k].first <= (uint64_t)e + 1) e = std::max(e, reg[k++].second);
            t.rs.push_back(s);
            t.re.push_back(e);
            t.cum.push_back(total);
            total += e - s + 1;
            i = k;
        }
        t.tlen[c] = total;
        t.positions += total;
        t.offs[c + 1] = (uint32_t)t.rs.size();
    }
    t.regions_merged = (uint32_t)t.rs.size();
    return QMCP_OK;
}

}  // namespace qmcp
#endif
