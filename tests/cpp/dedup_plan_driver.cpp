// Driver of genome-downsampler_amd/csrc/dedup_plan.h for tests/test_dedup_cpu.py (g++ alone, no HIP).
// One request per stdin line:
//   r <total_length> <min_span> <max_span> <tag_lo> <tag_hi> <q_lo> <q_hi> <with_quality>     read-mode fields
//   p <n_placed> <q_lo> <q_hi>                                                                pair-mode fields (stage 2)
//   -> "bits=<b0>,<b1>,... key_bits=<n> form=<0|1|2> passes=<n> rounds=<on>:<bits>:<passes>:<shift0>,<shift1>,..;..."
//      (fields least significant first; a round's shifts are listed for the fields it holds, in field order)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "dedup_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        uint32_t bits[4] = {0, 0, 0, 0};
        uint32_t n_fields = 0;
        if (kind == 'r') {
            uint64_t total = 0;
            uint32_t s0, s1, t0, t1, q0, q1, wq;
            in >> total >> s0 >> s1 >> t0 >> t1 >> q0 >> q1 >> wq;
            qmcp::dedup_read_fields(total, s0, s1, t0, t1, q0, q1, wq != 0, bits);
            n_fields = 4;
        } else if (kind == 'p') {
            uint64_t n_placed = 0;
            uint32_t q0, q1;
            in >> n_placed >> q0 >> q1;
            qmcp::dedup_pair_fields(n_placed, q0, q1, bits);
            n_fields = 3;
        } else {
            continue;
        }
        const qmcp::DedupSortPlan p = qmcp::plan_dedup_sort(bits, n_fields);
        std::printf("bits=");
        for (uint32_t f = 0; f < n_fields; ++f) std::printf("%s%u", f ? "," : "", bits[f]);
        std::printf(" key_bits=%u form=%u passes=%u rounds=", p.key_bits, p.form, p.passes);
        for (uint32_t r = 0; r < p.n_rounds; ++r) {
            std::printf("%s%u:%u:%u:", r ? ";" : "", p.rounds[r].pack.on, p.rounds[r].bits, p.rounds[r].passes);
            bool any = false;
            for (uint32_t f = 0; f < n_fields; ++f)
                if ((p.rounds[r].pack.on >> f) & 1u) {
                    std::printf("%s%u", any ? "," : "", p.rounds[r].pack.shift[f]);
                    any = true;
                }
            if (!any) std::printf("-");
        }
        std::printf("\n");
    }
    return 0;
}
