// amplicon_table.h -- the amplicons of several contigs as the FILTER of qmcp_hip_filter_solve_by_contig_host reads them.
//
// Plain C++17 (no HIP): api/amplicon_by_contig.inc.hip includes it, and so can a host-only test.  The caller gives the
// amplicons of each contig in CSR form -- contig c owns [offs[c], offs[c + 1]) of starts / ends, in any order,
// duplicates and nesting allowed.  The table keeps, per contig, the amplicons sorted by start and the running maximum
// of their ends, pmax_end[k] = max(end[offs[c]..k]).  A pair of reads [s1, e1], [s2, e2] on contig c then lies inside
// one amplicon (both reads included, inclusive bounds: Amplicon::includes) iff the last amplicon k of c with
// start[k] <= min(s1, s2) exists and pmax_end[k] >= max(e1, e2):
//   an amplicon contains both reads  <=>  its start <= min(s1, s2) and its end >= max(e1, e2); the amplicons with
//   start <= min(s1, s2) are a prefix of the sorted contig, and the largest end in that prefix is pmax_end[k].
// One binary search instead of the linear scan over every amplicon (AmpliconSet::member_includes_both).
#ifndef QMCP_AMPLICON_TABLE_H
#define QMCP_AMPLICON_TABLE_H
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "qmcp_hip.h"

namespace qmcp {

// offs has n_contigs + 1 entries: starts at 0, never decreases, ends at n_amplicons.  QMCP_OK or QMCP_EINVAL.
inline int check_amplicon_offsets(const uint32_t* offs, uint32_t n_contigs, uint64_t n_amplicons) {
    if (!offs || offs[0] != 0 || offs[n_contigs] != n_amplicons) return QMCP_EINVAL;
    for (uint32_t c = 0; c < n_contigs; ++c)
        if (offs[c + 1] < offs[c]) return QMCP_EINVAL;
    return QMCP_OK;
}

// sorted_starts / pmax_end (offs[n_contigs] entries each, same CSR as the input): per contig, the starts in ascending
// order and the running maximum of the ends taken in that order.  Offsets as check_amplicon_offsets accepts them.
inline int build_amplicon_table(const uint32_t* offs, const uint32_t* starts, const uint32_t* ends, uint32_t n_contigs,
                                std::vector<uint32_t>& sorted_starts, std::vector<uint32_t>& pmax_end) {
    const uint64_t n = offs ? offs[n_contigs] : 0;
    if (check_amplicon_offsets(offs, n_contigs, n) != QMCP_OK) return QMCP_EINVAL;
    if (n && (!starts || !ends)) return QMCP_EINVAL;
    sorted_starts.resize(n);
    pmax_end.resize(n);
    std::vector<std::pair<uint32_t, uint32_t>> amp;
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const uint32_t lo = offs[c], hi = offs[c + 1];
        amp.clear();
        for (uint32_t k = lo; k < hi; ++k) amp.emplace_back(starts[k], ends[k]);
        std::sort(amp.begin(), amp.end());
        uint32_t run = 0;
        for (uint32_t k = lo; k < hi; ++k) {
            const auto& a = amp[k - lo];
            run = k == lo ? a.second : std::max(run, a.second);
            sorted_starts[k] = a.first;
            pmax_end[k] = run;
        }
    }
    return QMCP_OK;
}

// the last index k in [lo, hi) with sorted_starts[k] <= x, or hi when there is none (the device kernel runs the same
// search on its copy of the table)
inline uint32_t last_start_at_or_before(const uint32_t* sorted_starts, uint32_t lo, uint32_t hi, uint32_t x) {
    uint32_t a = lo, b = hi;  // first index with start > x lies in [a, b]
    while (a < b) {
        const uint32_t m = a + (b - a) / 2;
        if (sorted_starts[m] <= x) a = m + 1;
        else b = m;
    }
    return a == lo ? hi : a - 1;
}

// host version of the FILTER's amplicon predicate for a pair on contig c (the tables of build_amplicon_table)
inline bool pair_in_one_amplicon(const uint32_t* offs, const uint32_t* sorted_starts, const uint32_t* pmax_end,
                                 uint32_t c, uint32_t s1, uint32_t e1, uint32_t s2, uint32_t e2) {
    const uint32_t lo = offs[c], hi = offs[c + 1];
    const uint32_t k = last_start_at_or_before(sorted_starts, lo, hi, std::min(s1, s2));
    return k != hi && pmax_end[k] >= std::max(e1, e2);
}

}  // namespace qmcp
#endif
