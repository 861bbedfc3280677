// amplicon_assign.h -- the amplicons of several contigs as the assign step of qmcp_hip_solve_amplicons_* reads them.
//
// Plain C++17 (no HIP): api/amplicon_clip.inc.hip includes it, and so can a host-only test.  The caller gives the
// amplicons of each contig in CSR form as amplicon_table.h takes them -- contig c owns [offs[c], offs[c + 1]) of starts /
// ends, in any order, duplicates and nesting allowed -- and optionally an insert [insert_start, insert_end] inside each.
// A unit of reads whose smallest start is s and whose largest end is e belongs to the amplicon of its contig that
// contains it (start <= s and end >= e, inclusive: Amplicon::includes) with
//   1. the greatest start, 2. then the smallest end, 3. then the smallest index in the caller's table.
// The table keeps, per contig, the amplicons sorted by (start ascending, end descending, index descending) with the
// running maximum of the ends, pmax[k] = max(end[offs[c]..k]).  Walking backwards from last_start_at_or_before(s) the
// starts fall, equal starts show their ends rising and equal (start, end) their indices rising: the first container met
// is the assigned one.  Nothing at or before k can contain the unit once pmax[k] < e, so the walk stops there.  Walking
// on to a second container tells whether several amplicons contain the unit.
// COST: on a tiled panel the walk is one or two steps.  On a deeply nested table (many amplicons that start before s,
// one early one that ends after e) it is linear in the amplicons of the contig.
#ifndef QMCP_AMPLICON_ASSIGN_H
#define QMCP_AMPLICON_ASSIGN_H
#include <algorithm>
#include <cstdint>
#include <vector>

#include "amplicon_table.h"
#include "qmcp_hip.h"

namespace qmcp {

// the sorted table: n amplicons, six words each, column by column (the device copy has the same layout)
struct AssignTable {
    uint32_t n = 0;
    std::vector<uint32_t> words;  // start | end | pmax | index in the caller's table | insert start | insert end
    const uint32_t* start() const { return words.data(); }
    const uint32_t* end() const { return words.data() + n; }
    const uint32_t* pmax() const { return words.data() + 2 * (size_t)n; }
    const uint32_t* index() const { return words.data() + 3 * (size_t)n; }
    const uint32_t* insert_start() const { return words.data() + 4 * (size_t)n; }
    const uint32_t* insert_end() const { return words.data() + 5 * (size_t)n; }
};

// The first amplicon k of the caller's table with start <= insert_start <= insert_end <= end violated, or n when every
// amplicon is fine.  Both insert arrays NULL: the insert is the amplicon, only start <= end is asked.
inline uint64_t first_bad_insert(const uint32_t* starts, const uint32_t* ends, const uint32_t* ins_starts,
                                 const uint32_t* ins_ends, uint64_t n) {
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t is = ins_starts ? ins_starts[k] : starts[k], ie = ins_ends ? ins_ends[k] : ends[k];
        if (!(starts[k] <= is && is <= ie && ie <= ends[k])) return k;
    }
    return n;
}

// what build_assign_table refuses (it owns these checks: the entry only words the messages)
enum AssignTableError {
    kAssignTableOk = 0,
    kAssignTableOffsets,       // offsets missing, not from 0 or decreasing (check_amplicon_offsets)
    kAssignTableNull,          // amplicons without starts / ends
    kAssignTableInsertArrays,  // one insert array without the other
    kAssignTableInsert         // *bad: the first amplicon with start <= insert_start <= insert_end <= end violated
};

inline AssignTableError build_assign_table(const uint32_t* offs, const uint32_t* starts, const uint32_t* ends,
                                           const uint32_t* ins_starts, const uint32_t* ins_ends, uint32_t n_contigs,
                                           AssignTable& t, uint64_t* bad = nullptr) {
    const uint64_t n = offs ? offs[n_contigs] : 0;
    if (check_amplicon_offsets(offs, n_contigs, n) != QMCP_OK) return kAssignTableOffsets;
    if (n && (!starts || !ends)) return kAssignTableNull;
    if ((ins_starts == nullptr) != (ins_ends == nullptr)) return kAssignTableInsertArrays;
    const uint64_t first_bad = first_bad_insert(starts, ends, ins_starts, ins_ends, n);
    if (bad) *bad = first_bad;
    if (first_bad != n) return kAssignTableInsert;
    t.n = (uint32_t)n;
    t.words.assign(6 * (size_t)n, 0);
    uint32_t* w = t.words.data();
    std::vector<uint32_t> order;
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const uint32_t lo = offs[c], hi = offs[c + 1];
        order.resize(hi - lo);
        for (uint32_t k = lo; k < hi; ++k) order[k - lo] = k;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            if (starts[a] != starts[b]) return starts[a] < starts[b];
            if (ends[a] != ends[b]) return ends[a] > ends[b];
            return a > b;
        });
        uint32_t run = 0;
        for (uint32_t k = lo; k < hi; ++k) {
            const uint32_t a = order[k - lo];
            run = k == lo ? ends[a] : std::max(run, ends[a]);
            w[k] = starts[a];
            w[n + k] = ends[a];
            w[2 * n + k] = run;
            w[3 * n + k] = a;
            w[4 * n + k] = ins_starts ? ins_starts[a] : starts[a];
            w[5 * n + k] = ins_ends ? ins_ends[a] : ends[a];
        }
    }
    return kAssignTableOk;
}

// Host twin of the device search: the sorted position of the amplicon of contig c assigned to a unit with smallest
// start s and largest end e, or QMCP_NO_AMPLICON; *several (may be NULL) tells whether a second amplicon contains it.
inline uint32_t assign_amplicon(const uint32_t* offs, const AssignTable& t, uint32_t c, uint32_t s, uint32_t e,
                                bool* several) {
    if (several) *several = false;
    const uint32_t lo = offs[c], hi = offs[c + 1];
    uint32_t k = last_start_at_or_before(t.start(), lo, hi, s);
    if (k == hi) return QMCP_NO_AMPLICON;
    uint32_t found = QMCP_NO_AMPLICON;
    for (;; --k) {
        if (t.pmax()[k] < e) break;
        if (t.end()[k] >= e) {
            if (found == QMCP_NO_AMPLICON) {
                found = k;
            } else {
                if (several) *several = true;
                break;
            }
        }
        if (k == lo) break;
    }
    return found;
}

}  // namespace qmcp
#endif
