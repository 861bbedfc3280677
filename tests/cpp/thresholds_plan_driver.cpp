// Driver of genome-downsampler_amd/csrc/thresholds_plan.h for tests/test_thresholds_cpu.py (g++ alone, no HIP).
// One request per stdin line:
//   W <mask hex> <seen hex>                         -> "fresh=<hex> lost=<hex> seen=<hex>"
//   P <own> <mate> <own placed 0|1> <mate placed>   -> "t=<threshold>"
//   C <n_reads> <lo> <hi> <flags> <has counts_out 0|1> <capacity>   -> "refusal=<ThresholdsRefusal>"
//   R <n_reads> <lo> <n_steps>, then per step one line of ceil(n_reads / 64) mask words in hex
//     -> "violations=<n> seen=<n> t=<threshold of read 0>,<read 1>,..."
//     the whole step loop as k_thresholds_step runs it, word by word: a fresh bit stores lo + step, a lost bit counts
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "thresholds_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind = 0;
        if (!(in >> kind)) continue;
        if (kind == 'W') {
            unsigned long long mask, seen;
            in >> std::hex >> mask >> seen;
            const qmcp::ThresholdsWord w = qmcp::thresholds_word(mask, seen);
            std::printf("fresh=%llx lost=%llx seen=%llx\n", (unsigned long long)w.fresh, (unsigned long long)w.lost,
                        (unsigned long long)w.seen);
        } else if (kind == 'P') {
            unsigned own, mate, own_placed, mate_placed;
            in >> own >> mate >> own_placed >> mate_placed;
            std::printf("t=%u\n", qmcp::thresholds_pair(own, mate, own_placed != 0, mate_placed != 0));
        } else if (kind == 'C') {
            unsigned long long n;
            unsigned lo, hi, flags, has, cap;
            in >> n >> lo >> hi >> flags >> has >> cap;
            std::printf("refusal=%d\n", (int)qmcp::thresholds_check(n, lo, hi, flags, has != 0, cap));
        } else if (kind == 'R') {
            unsigned long long n;
            unsigned lo, steps;
            in >> n >> lo >> steps;
            const size_t words = (size_t)((n + 63) / 64);
            std::vector<uint64_t> seen(words, 0);
            std::vector<unsigned> t((size_t)n, qmcp::kThresholdNever);
            unsigned long long violations = 0, seen_n = 0;
            for (unsigned k = 0; k < steps; ++k) {
                std::getline(std::cin, line);
                std::istringstream row(line);
                for (size_t w = 0; w < words; ++w) {
                    unsigned long long m = 0;
                    row >> std::hex >> m;
                    const qmcp::ThresholdsWord x = qmcp::thresholds_word(m, seen[w]);
                    for (unsigned b = 0; b < 64; ++b)
                        if ((x.fresh >> b) & 1ull) t[64 * w + b] = lo + k;
                    violations += (unsigned long long)__builtin_popcountll(x.lost);
                    seen_n += (unsigned long long)__builtin_popcountll(x.fresh);
                    seen[w] = x.seen;
                }
            }
            std::printf("violations=%llu seen=%llu t=", violations, seen_n);
            for (size_t i = 0; i < t.size(); ++i) std::printf("%s%u", i ? "," : "", t[i]);
            std::printf("\n");
        }
    }
    return 0;
}
