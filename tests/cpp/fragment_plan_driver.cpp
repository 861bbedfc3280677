// fragment_plan_driver.cpp -- fragment_plan.h under g++ alone (tests/test_fragments_cpu.py).
// stdin: one "n_templates n_contigs longest_contig" per line; stdout: one line of key=value pairs per input line.
#include <cstdio>

#include "fragment_plan.h"

int main() {
    unsigned long long nt, nc, longest;
    while (std::scanf("%llu %llu %llu", &nt, &nc, &longest) == 3) {
        const qmcp::FragmentPlan p = qmcp::plan_fragment_sort((uint32_t)nt, (uint32_t)nc, (uint32_t)longest);
        std::printf("rounds=%u passes=%u key_bytes=%u", p.n_rounds, p.passes, p.key_bytes);
        for (uint32_t r = 0; r < p.n_rounds; ++r)
            std::printf(" r%u=%u,%u,%u,%u", r, p.rounds[r].passes, p.rounds[r].start_bytes, p.rounds[r].contig_bytes,
                        p.rounds[r].template_bytes);
        std::printf("\n");
    }
    return 0;
}
