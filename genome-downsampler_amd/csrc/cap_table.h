// cap_table.h -- the cap regions of several contigs as qmcp_hip_solve_profile_* reads them: a piecewise-constant cap
// along every contig, cap_c(p) = the cap of the region of contig c that holds p, default_cap elsewhere.
//
// Plain C++17 (no HIP needed): api/profile.inc.hip includes it, and so can a host-only test
// (tests/cpp/cap_table_driver.cpp).  The caller gives the regions of each contig in CSR form -- contig c owns
// [offs[c], offs[c + 1]) of starts / ends / caps, inclusive bounds, in any order.  The table keeps, per contig, the regions
//   1. clipped to [0, length - 1]; a region that begins at or beyond length is dropped (every region of a contig of
//      length 0 is);
//   2. sorted by start;
//   3. checked to be disjoint AFTER clipping (two regions may share no position; adjacent ones are fine, and stay two
//      regions: their caps may differ).
// Unlike the target table nothing is merged.  solve_by_contig_on_device solves batches of consecutive contigs on one
// concatenated position axis, so batch_cap_table gives any run of contigs its regions in global positions of that run:
// sorted, disjoint, ready for k_profile_need's binary search.
#ifndef QMCP_CAP_TABLE_H
#define QMCP_CAP_TABLE_H
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "qmcp_hip.h"

namespace qmcp {

constexpr uint32_t kCapLimit = 1u << 31;  // a cap of 2^31 or more is QMCP_ERANGE: k_profile_need flags cut positions in the top bit of need

struct CapTable {
    std::vector<uint32_t> offs;         // n_contigs + 1: contig c owns kept regions [offs[c], offs[c + 1])
    std::vector<uint32_t> rs, re, cap;  // per kept region, ascending within a contig: inclusive bounds (clipped), cap
    uint64_t positions = 0;             // positions inside kept regions
    uint32_t regions_in = 0, regions_used = 0;
    uint32_t max_cap = 0;               // the largest cap of a kept region
};

// offs has n_contigs + 1 entries: starts at 0 and never decreases.  QMCP_OK or QMCP_EINVAL.
inline int check_cap_offsets(const uint32_t* offs, uint32_t n_contigs) {
    if (!offs || offs[0] != 0) return QMCP_EINVAL;
    for (uint32_t c = 0; c < n_contigs; ++c)
        if (offs[c + 1] < offs[c]) return QMCP_EINVAL;
    return QMCP_OK;
}

// QMCP_EINVAL: bad offsets, null tables with a non-zero count, null lengths, a region with start > end, two regions of
// one contig that overlap after clipping.  QMCP_ERANGE: a cap of 2^31 or more.  offs == NULL is the empty table.
inline int build_cap_table(const uint32_t* offs, const uint32_t* starts, const uint32_t* ends, const uint32_t* caps,
                           const uint32_t* lengths, uint32_t n_contigs, CapTable& t) {
    t = CapTable();
    t.offs.assign((size_t)n_contigs + 1, 0);
    if (!lengths) return QMCP_EINVAL;
    if (!offs) return QMCP_OK;
    if (check_cap_offsets(offs, n_contigs) != QMCP_OK) return QMCP_EINVAL;
    const uint32_t n = offs[n_contigs];
    if (n && (!starts || !ends || !caps)) return QMCP_EINVAL;
    for (uint32_t k = 0; k < n; ++k)
        if (starts[k] > ends[k]) return QMCP_EINVAL;
    for (uint32_t k = 0; k < n; ++k)
        if (caps[k] >= kCapLimit) return QMCP_ERANGE;
    t.regions_in = n;
    struct Reg { uint32_t s, e, cap; };
    std::vector<Reg> reg;
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const uint32_t len = lengths[c];
        reg.clear();
        for (uint32_t k = offs[c]; k < offs[c + 1]; ++k) {
            if (starts[k] >= len) continue;  // beyond the contig
            reg.push_back({starts[k], std::min(ends[k], len - 1), caps[k]});
        }
        std::sort(reg.begin(), reg.end(), [](const Reg& a, const Reg& b) { return a.s < b.s; });
        for (size_t i = 0; i < reg.size(); ++i) {
            if (i && reg[i].s <= reg[i - 1].e) return QMCP_EINVAL;
            t.rs.push_back(reg[i].s);
            t.re.push_back(reg[i].e);
            t.cap.push_back(reg[i].cap);
            t.positions += (uint64_t)(reg[i].e - reg[i].s) + 1;
            t.max_cap = std::max(t.max_cap, reg[i].cap);
        }
        t.offs[c + 1] = (uint32_t)t.rs.size();
    }
    t.regions_used = (uint32_t)t.rs.size();
    return QMCP_OK;
}

// The regions of contigs [first, first + count) on the concatenated position axis of that run (contig first + k begins
// at the sum of the lengths before it; a batch holds at most 2^31 - 2 positions): gs / ge / gcap, ascending and disjoint.
inline void batch_cap_table(const CapTable& t, const uint32_t* lengths, uint32_t first, uint32_t count,
                            std::vector<uint32_t>& gs, std::vector<uint32_t>& ge, std::vector<uint32_t>& gcap) {
    gs.clear(); ge.clear(); gcap.clear();
    uint64_t base = 0;
    for (uint32_t c = first; c < first + count; ++c) {
        for (uint32_t k = t.offs[c]; k < t.offs[c + 1]; ++k) {
            gs.push_back((uint32_t)(base + t.rs[k]));
            ge.push_back((uint32_t)(base + t.re[k]));
            gcap.push_back(t.cap[k]);
        }
        base += lengths[c];
    }
}

// A staged solve under a cap table (api/templates_profile.inc.hip) runs stage T of a schedule that ends at M under
// ceil(cap * T / M), in 64 bits: never above cap, cap itself at T == M, T where cap == M, and 0 only where cap is 0.
inline uint32_t scale_cap(uint32_t cap, uint32_t T, uint32_t M) {
    return (uint32_t)(((uint64_t)cap * T + M - 1) / M);
}

// before[k], per kept region: the positions below rs[k] of its contig whose cap is positive -- F(rs[k]) of the prefix
// count F(x) = |{ p < x : cap(p) > 0 }| that k_tpl_on_cap evaluates at a segment's two ends.  Between two region borders
// F is linear, so the values at the borders are all the kernel needs.  (A contig holds fewer than 2^31 positions.)
inline void cap_positive_before(const CapTable& t, uint32_t default_cap, std::vector<uint32_t>& before) {
    before.assign(t.rs.size(), 0);
    const size_t n_contigs = t.offs.size() - 1;
    for (size_t c = 0; c < n_contigs; ++c) {
        uint32_t f = 0, x = 0;  // f = F(x)
        for (uint32_t k = t.offs[c]; k < t.offs[c + 1]; ++k) {
            if (default_cap != 0) f += t.rs[k] - x;
            before[k] = f;
            if (t.cap[k] != 0) f += t.re[k] - t.rs[k] + 1;
            x = t.re[k] + 1;
        }
    }
}

}  // namespace qmcp
#endif
