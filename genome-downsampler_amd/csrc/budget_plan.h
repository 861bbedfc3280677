// budget_plan.h -- the host side of a budget solve (qmcp_hip_solve_budget_*): which coverage the next probe solves.
// Plain C++, no HIP: tests/cpp/budget_plan_driver.cpp drives it under g++ alone.
//
// count(M) is what a by-contig solve at M keeps (after pair completion, when asked).  The search keeps a FEASIBLE lo
// (count(lo) <= budget; 0 at first: count(0) = 0) and an INFEASIBLE hi (top + 1 at first, a sentinel that is never
// probed) and ends at hi == lo + 1: M* = lo then has count(M*) <= budget, and M* == top or count(M* + 1) > budget.
// Nothing here needs count to be monotone; where it is, M* is the one largest feasible coverage.
//   the bound    curve[M] = S(M) = sum over positions of min(cov(p), M) is the number of bases ANY answer at M holds, in
//                reads of at most max_span bases: count(M) >= LB(M) = ceil(S(M) / max_span).  LB rises with M, so hi
//                starts at the smallest M with LB(M) > budget without a probe.  Beyond the curve's last entry S is taken
//                as that entry: smaller than the truth, so still a lower bound.
//   first probe  the largest M < hi with S(M) / mean_span <= budget, mean_span = total_bases / reads_placed
//   later ones   the same on the curve scaled by what the last probe showed: the largest M inside (lo, hi) with
//                S(M) * count(last) / S(last) <= budget, clamped into (lo, hi)
//   bisection    a probe that leaves hi - lo above ceil(old / 2) is slow; after two slow probes in a row every further
//                probe bisects.  A probe that is not slow is one of at most L = ceil(log2(top + 1)) halvings, slow
//                probes come singly between them until the two that switch to bisection: at most 2 L + 2 probes.
#ifndef QMCP_BUDGET_PLAN_H
#define QMCP_BUDGET_PLAN_H
#include <cstdint>

namespace qmcp {

inline uint32_t budget_probe_limit(uint32_t top) {
    uint32_t l = 0;
    while (l < 32 && (1ull << l) < (uint64_t)top + 1) ++l;  // ceil(log2(top + 1))
    return 2 * l + 2;
}

struct BudgetPlan {
    typedef unsigned __int128 u128;
    // the call
    const uint64_t* curve = nullptr;  // S(0 .. curve_n - 1)
    uint32_t curve_n = 0;
    uint32_t top = 0, max_span = 1;
    uint64_t budget = 0, total_bases = 0, reads_placed = 0;
    // the search
    uint32_t lo = 0, hi = 1;
    uint64_t count_lo = 0;  // count(lo)
    uint64_t count_hi = 0;  // count(hi) where a probe measured it, else 0
    uint64_t bound_hi = 0;  // LB(hi) where the bound set hi, else 0
    uint32_t probes = 0, slow = 0, last_M = 0;
    uint64_t last_count = 0;
    bool bisect = false;

    uint64_t S(uint32_t M) const { return curve_n == 0 ? 0 : curve[M < curve_n ? M : curve_n - 1]; }
    uint64_t LB(uint32_t M) const { return (S(M) + max_span - 1) / max_span; }

    // the largest M in [a, b] with S(M) * mul <= rhs (S rises with M); a - 1 when there is none
    uint32_t largest_with(uint32_t a, uint32_t b, uint64_t mul, u128 rhs) const {
        uint32_t good = a - 1;
        while (a <= b) {
            const uint32_t mid = a + (b - a) / 2;
            if ((u128)S(mid) * mul <= rhs) {
                good = mid;
                a = mid + 1;
            } else {
                b = mid - 1;
            }
        }
        return good;
    }

    void start(const uint64_t* curve_, uint32_t curve_n_, uint32_t top_, uint32_t max_span_, uint64_t total_bases_,
               uint64_t reads_placed_, uint64_t budget_) {
        *this = BudgetPlan();
        curve = curve_;
        curve_n = curve_n_;
        top = top_;
        max_span = max_span_ ? max_span_ : 1;
        total_bases = total_bases_;
        reads_placed = reads_placed_;
        budget = budget_;
        hi = top + 1;
        // the smallest M in 1 .. top with LB(M) > budget: LB(M) <= budget is S(M) <= budget * max_span
        const uint32_t under = top ? largest_with(1, top, 1, (u128)budget * max_span) : 0;
        if (under < top) {
            hi = under + 1;
            bound_hi = LB(hi);
        }
    }

    bool done() const { return hi == lo + 1; }

    // the coverage to solve next, strictly inside (lo, hi); only while !done()
    uint32_t next() const {
        const uint32_t a = lo + 1, b = hi - 1;
        if (bisect) return lo + (hi - lo) / 2;
        uint32_t m;
        if (probes == 0)
            m = largest_with(a, b, reads_placed, (u128)budget * total_bases);
        else
            m = largest_with(a, b, last_count, (u128)budget * S(last_M));
        return m < a ? a : m;
    }

    void report(uint32_t M, uint64_t count) {
        const uint32_t before = hi - lo;
        if (count <= budget) {
            lo = M;
            count_lo = count;
        } else {
            hi = M;
            count_hi = count;
            bound_hi = 0;
        }
        const uint32_t after = hi - lo;
        slow = after > before - before / 2 ? slow + 1 : 0;
        if (slow >= 2) bisect = true;
        last_M = M;
        last_count = count;
        ++probes;
    }
};

}  // namespace qmcp
#endif
