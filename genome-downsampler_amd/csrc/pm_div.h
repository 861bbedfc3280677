// Division by a run-time constant without a divide: the pass-major walk turns a position into its block of the sweep,
// (p - base) / ell, for every position of its range, and the GPU has no integer divide (a 32-bit `/` is tens of vector
// instructions).  The divisor is known on the host at launch, so the launcher computes a multiplier and a shift once
// and the kernel multiplies.
//
// For 1 <= d <= 512: s = ceil(log2 d), M = ceil(2^(32 + s) / d) = 2^32 + mul with 0 <= mul < 2^32 (2^(s-1) < d <= 2^s).
// Then for every n < 2^31:  floor(n / d) = (mulhi(n, mul) + n) >> s.
//   M d = 2^(32 + s) + e with 0 <= e < d <= 2^s, so n M / 2^(32 + s) = n / d + n e / (d 2^(32 + s)), and the excess
//   n e / 2^(32 + s) < 2^31 2^s / 2^(32 + s) = 1/2 < 1: it never carries the quotient over the next multiple of 1/d.
//   mulhi(n, mul) + n = floor(n M / 2^32), and mulhi(n, mul) < n (mul < 2^32), so the sum is below 2 n < 2^32: no wrap.
// A power of two gives mul = 0 and the plain shift; d = 1 gives s = 0.  (The argument bounds n, not d; the sweep's
// spans are at most 512 and that is what tests/test_pm_div.py goes through.)
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QMCP_PM_DIV_HD __host__ __device__
#else
#define QMCP_PM_DIV_HD
#endif

namespace qmcp {

static constexpr uint32_t kPmDivMaxDivisor = 512u;        // divisors the constants are exact for ...
static constexpr uint32_t kPmDivMaxDividend = 0x7FFFFFFFu;  // ... and dividends

struct PmDiv { uint32_t mul, shift; };

// the constants of divisor d (1 ... kPmDivMaxDivisor; 0 is treated as 1)
QMCP_PM_DIV_HD inline PmDiv pm_div_make(uint32_t d) {
    if (d == 0u) d = 1u;
    uint32_t s = 0;
    while ((1u << s) < d) ++s;
    const uint64_t two = 1ull << (32u + s);            // s <= 9 for d <= 512: no overflow
    const uint64_t M = (two + d - 1u) / d;             // in [2^32, 2^33)
    return PmDiv{(uint32_t)(M - (1ull << 32)), s};
}

// floor(n / d) for n <= kPmDivMaxDividend
QMCP_PM_DIV_HD inline uint32_t pm_div(uint32_t n, PmDiv k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (__umulhi(n, k.mul) + n) >> k.shift;
#else
    return ((uint32_t)(((uint64_t)n * k.mul) >> 32) + n) >> k.shift;
#endif
}

}  // namespace qmcp
