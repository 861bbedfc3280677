// Stand-alone host check of csrc/pm_div.h for tests/test_pm_div.py: the multiply-and-shift quotient against the `/`
// operator.  For every divisor 1 ... 512: the dividends k d - 1, k d and k d + 1 for every k whose k d lies within
// `kWindow` of 2^16, of 2^24 and below 2^31 - 1 (and the bounds themselves), then 10^6 random dividends below 2^31 with
// random divisors.  Prints the number of quotients checked; exit status 1 at the first difference.
#include <cstdint>
#include <cstdio>

#include "pm_div.h"

namespace {
unsigned long long g_checked = 0;

bool same(uint32_t n, uint32_t d, qmcp::PmDiv k) {
    ++g_checked;
    const uint32_t got = qmcp::pm_div(n, k), want = n / d;
    if (got == want) return true;
    std::printf("pm_div(%u, %u) = %u, not %u (mul %u, shift %u)\n", n, d, got, want, k.mul, k.shift);
    return false;
}
}  // namespace

int main() {
    const uint64_t kMax = qmcp::kPmDivMaxDividend;  // 2^31 - 1
    const uint64_t kWindow = 4096;                  // multiples of d this far around a centre: at least eight of them
    const uint64_t centres[3] = {1ull << 16, 1ull << 24, kMax};
    for (uint32_t d = 1; d <= qmcp::kPmDivMaxDivisor; ++d) {
        const qmcp::PmDiv k = qmcp::pm_div_make(d);
        if (!same(0u, d, k) || !same((uint32_t)kMax, d, k)) return 1;
        for (const uint64_t c : centres) {
            const uint64_t lo = c > kWindow ? c - kWindow : 0, hi = c + kWindow;
            for (uint64_t q = lo / d; q * d <= hi; ++q)
                for (int delta = -1; delta <= 1; ++delta) {
                    const int64_t n = (int64_t)(q * d) + delta;
                    if (n < 0 || (uint64_t)n > kMax) continue;
                    if (!same((uint32_t)n, d, k)) return 1;
                }
        }
    }
    uint64_t x = 0x9E3779B97F4A7C15ull;  // xorshift64*
    for (int i = 0; i < 1000000; ++i) {
        x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
        const uint64_t r = x * 0x2545F4914F6CDD1Dull;
        const uint32_t n = (uint32_t)(r >> 33), d = 1u + (uint32_t)(r & 0xFFFFu) % qmcp::kPmDivMaxDivisor;
        if (!same(n, d, qmcp::pm_div_make(d))) return 1;
    }
    std::printf("checked %llu\n", g_checked);
    return 0;
}
