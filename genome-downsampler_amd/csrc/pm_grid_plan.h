// pm_grid_plan.h -- where the pass-major form of the range-ranked route (kernels/pass_major.inc.hip) cuts its ranges.
// Plain C++, no HIP: tests/cpp/pm_grid_plan_driver.cpp drives it under g++ alone.
//
// A range is 2^shift positions of an axis the reads' starts are laid on; its digit is `v >> shift`, a record's key
// `v & (2^shift - 1)`.  Two axes:
//   global    v = poff[c] + s: the genome's own positions.  Ranges straddle contig borders, and a range that does gets
//             two slices per pass pair -- each padded to whole groups of 64 slots -- where the others get one: the same
//             records in more wave-slots, and the per-range kernels take as long as their slowest range.
//   aligned   v = (rbase[c] << shift) + s, rbase[c] = sum of ceil(len_k / 2^shift) over the contigs before c: every
//             contig begins a range, no range straddles a border.  Taken where the range count still fits one partition
//             level (<= 256) and -- unless the caller insists -- the heaviest range's expected wave-slots come out
//             strictly lighter than the global grid's.
// Both are the same tables to the kernels: vbase[c] (the virtual start of contig c) for the producer; per range the real
// global position of key 0 (pos0), the positions of the range that exist (live) and the range's contig (kPmNoContig
// where it straddles a border) for the consumers.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace qmcp {

static constexpr uint32_t kPmNoContig = 0xFFFFFFFFu;
static constexpr uint32_t kPmGridRows = 256u;  // ranges of one partition level

struct PmGridPlan {
    int aligned = 0;                  // the grid taken: 0 global, 1 aligned
    uint32_t n_ranges = 0;            // workgroups of the per-range kernels
    uint32_t aligned_ranges = 0;      // what the aligned grid needs (may exceed 256: then it is not taken)
    double heaviest_global = 0.0;     // expected wave-slots of the heaviest range, uniform starts
    double heaviest_aligned = 0.0;    // (0 where the aligned grid does not fit)
    // device tables, in this order in one buffer: pos0 | live | contig (kPmGridRows words each) | vbase (n_contigs + 1)
    std::vector<uint32_t> words;
    const uint32_t* pos0() const { return words.data(); }
    const uint32_t* live() const { return words.data() + kPmGridRows; }
    const uint32_t* contig() const { return words.data() + 2u * kPmGridRows; }
    const uint32_t* vbase() const { return words.data() + 3u * kPmGridRows; }
};

// Expected wave-slots per range under uniform starts: a contig's pass deals its reads to the ranges the contig overlaps
// in proportion to the overlap, and every slice is rounded up to whole groups of 64.  `first[c]` is the first range of
// contig c and `phase[c]` the key of its first position.  -> the heaviest range's.
inline double pm_grid_expected_heaviest(const uint64_t* roff, const uint64_t* poff, uint32_t n_contigs, uint32_t shift,
                                        uint32_t pass, const std::vector<uint32_t>& first, const std::vector<uint32_t>& phase,
                                        uint32_t n_ranges) {
    const uint64_t width = 1ull << shift;
    std::vector<double> slots(n_ranges, 0.0);
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const uint64_t reads = roff[c + 1] - roff[c], len = poff[c + 1] - poff[c];
        if (reads == 0 || len == 0) continue;
        const double passes = (double)reads / (double)pass < 1.0 ? 1.0 : (double)reads / (double)pass;
        const double per_pass = (double)reads / passes;
        uint64_t done = 0;  // positions of the contig dealt so far
        for (uint32_t r = first[c]; done < len && r < n_ranges; ++r) {
            const uint64_t room = r == first[c] ? width - phase[c] : width;
            const uint64_t o = len - done < room ? len - done : room;
            slots[r] += passes * std::ceil(per_pass * (double)o / (double)len / 64.0);
            done += o;
        }
    }
    double heaviest = 0.0;
    for (double s : slots) heaviest = s > heaviest ? s : heaviest;
    return heaviest;
}

// want: -1 the global grid, 0 the lighter one, +1 the aligned grid wherever it fits 256 ranges.
inline PmGridPlan pm_grid_plan(const uint64_t* roff, const uint64_t* poff, uint32_t n_contigs, uint32_t shift,
                               uint32_t pass, int want) {
    PmGridPlan g;
    const uint64_t width = 1ull << shift, ltot = poff[n_contigs];
    const uint32_t global_ranges = (uint32_t)(ltot >> shift) + 1u;  // covers positions 0..ltot
    std::vector<uint32_t> rbase((size_t)n_contigs + 1, 0u), first((size_t)n_contigs, 0u), phase((size_t)n_contigs, 0u);
    uint64_t sum = 0;
    for (uint32_t c = 0; c < n_contigs; ++c) {
        rbase[c] = (uint32_t)(sum < 0xFFFFFFFFull ? sum : 0xFFFFFFFFull);
        sum += (poff[c + 1] - poff[c] + width - 1) >> shift;
    }
    rbase[n_contigs] = (uint32_t)(sum < 0xFFFFFFFFull ? sum : 0xFFFFFFFFull);
    g.aligned_ranges = rbase[n_contigs];
    for (uint32_t c = 0; c < n_contigs; ++c) { first[c] = (uint32_t)(poff[c] >> shift); phase[c] = (uint32_t)(poff[c] & (width - 1)); }
    g.heaviest_global = pm_grid_expected_heaviest(roff, poff, n_contigs, shift, pass, first, phase, global_ranges);
    const bool fits = g.aligned_ranges >= 1u && g.aligned_ranges <= kPmGridRows && global_ranges <= kPmGridRows;
    if (fits) {
        const std::vector<uint32_t> zero((size_t)n_contigs, 0u);
        const std::vector<uint32_t> afirst(rbase.begin(), rbase.end() - 1);
        g.heaviest_aligned = pm_grid_expected_heaviest(roff, poff, n_contigs, shift, pass, afirst, zero, g.aligned_ranges);
    }
    g.aligned = fits && want >= 0 && (want > 0 || g.heaviest_aligned < g.heaviest_global) ? 1 : 0;
    g.n_ranges = g.aligned ? g.aligned_ranges : global_ranges;
    if (global_ranges > kPmGridRows) return g;  // (two partition levels: the pass-major form is not taken, no tables)
    g.words.assign((size_t)3u * kPmGridRows + n_contigs + 1, 0u);
    uint32_t* const pos0 = g.words.data();
    uint32_t* const live = pos0 + kPmGridRows;
    uint32_t* const contig = live + kPmGridRows;
    uint32_t* const vbase = contig + kPmGridRows;
    if (g.aligned) {
        // (a contig without positions begins where the next one does; one behind the last range is moved onto the axis'
        //  last key, so that a read given for it -- the call fails -- still has a digit inside the grid)
        const uint32_t v_last = (g.n_ranges << shift) - 1u;
        for (uint32_t c = 0; c <= n_contigs; ++c) vbase[c] = (rbase[c] << shift) < v_last ? rbase[c] << shift : v_last;
        for (uint32_t c = 0; c < n_contigs; ++c) {
            const uint64_t len = poff[c + 1] - poff[c];
            for (uint32_t j = 0; j < rbase[c + 1] - rbase[c]; ++j) {
                const uint32_t r = rbase[c] + j;
                pos0[r] = (uint32_t)(poff[c] + (uint64_t)j * width);
                live[r] = (uint32_t)(len - (uint64_t)j * width < width ? len - (uint64_t)j * width : width);
                contig[r] = c;
            }
        }
    } else {
        for (uint32_t c = 0; c <= n_contigs; ++c) vbase[c] = (uint32_t)poff[c];
        uint32_t c = 0;
        for (uint32_t r = 0; r < g.n_ranges; ++r) {
            const uint64_t p = (uint64_t)r << shift;
            pos0[r] = (uint32_t)p;
            live[r] = p < ltot ? (uint32_t)(ltot - p < width ? ltot - p : width) : 0u;
            while (c + 1 < n_contigs && poff[c + 1] <= p) ++c;  // the contig of the range's first position
            contig[r] = live[r] == 0u || p + live[r] <= poff[c + 1] ? c : kPmNoContig;
        }
    }
    return g;
}

}  // namespace qmcp
