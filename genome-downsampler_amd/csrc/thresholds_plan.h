// thresholds_plan.h -- what a thresholds solve (qmcp_hip_solve_thresholds_*) decides without a device: whether the call's
// range, flags and counts array are legal, and what one 64-bit word of a coverage's mask does to the reads seen so far.
// Plain C++ (no HIP needed): kernels/thresholds.inc.hip calls thresholds_word per lane, api/thresholds.inc.hip calls
// thresholds_check, and tests/cpp/thresholds_plan_driver.cpp drives both under g++ alone -- the only way a non-zero
// nesting violation is reached, since the canonical selection has never produced one.
#ifndef QMCP_THRESHOLDS_PLAN_H
#define QMCP_THRESHOLDS_PLAN_H
#include <stdint.h>

#if defined(__HIPCC__)
#define QMCP_TH_HD __host__ __device__
#else
#define QMCP_TH_HD
#endif

namespace qmcp {

static const uint32_t kThresholdNever = 0xFFFFu;       // QMCP_THRESHOLD_NEVER
static const uint32_t kThresholdsCoverageMax = 65534u;  // QMCP_THRESHOLDS_COVERAGE_MAX
static const uint32_t kThresholdsWholePairs = 1u;       // QMCP_THRESHOLDS_WHOLE_PAIRS

// One word of the step at coverage M.  mask: keep_M; seen: the reads that have a threshold already (all of them placed).
//   fresh  reads that get the threshold M: kept now, never before
//   lost   reads with a threshold that keep_M drops: each is one nesting violation
//   seen   the reads with a threshold after this step
struct ThresholdsWord {
    uint64_t fresh, lost, seen;
};
QMCP_TH_HD inline ThresholdsWord thresholds_word(uint64_t mask, uint64_t seen) {
    ThresholdsWord w;
    w.fresh = mask & ~seen;
    w.lost = seen & ~mask;
    w.seen = seen | mask;
    return w;
}

// A placed read's threshold under QMCP_THRESHOLDS_WHOLE_PAIRS: the smaller of its own and its PLACED mate's; an unplaced
// read keeps kThresholdNever and lends nothing (its own threshold is kThresholdNever already: no mask ever holds it).
QMCP_TH_HD inline uint32_t thresholds_pair(uint32_t own, uint32_t mate, bool own_placed, bool mate_placed) {
    if (!own_placed) return kThresholdNever;
    return mate_placed && mate < own ? mate : own;
}

// the checks both entries make on (lo, hi, flags, counts) before anything else; 0: legal
enum ThresholdsRefusal : int {
    kThresholdsOk = 0,
    kThresholdsBadFlags,      // EINVAL
    kThresholdsOddReads,      // EINVAL
    kThresholdsZeroLo,        // EINVAL
    kThresholdsLoAboveHi,     // EINVAL
    kThresholdsCapacityOnly,  // EINVAL
    kThresholdsHiTooLarge     // ERANGE
};
inline ThresholdsRefusal thresholds_check(uint64_t n_reads, uint32_t lo, uint32_t hi, uint32_t flags, bool has_counts_out,
                                          uint32_t counts_capacity) {
    if (flags & ~kThresholdsWholePairs) return kThresholdsBadFlags;
    if ((flags & kThresholdsWholePairs) && (n_reads & 1ull)) return kThresholdsOddReads;
    if (lo == 0) return kThresholdsZeroLo;
    if (lo > hi) return kThresholdsLoAboveHi;
    if (!has_counts_out && counts_capacity) return kThresholdsCapacityOnly;
    if (hi > kThresholdsCoverageMax) return kThresholdsHiTooLarge;
    return kThresholdsOk;
}

}  // namespace qmcp
#endif
