// Driver of genome-downsampler_amd/csrc/stratified_plan.h for tests/test_stratified_cpu.py (g++ alone, no HIP).
// One request per stdin line:
//   p <n_strata> <n_contigs> <max_reads> <max_positions> | <count>... | <length>... | <cap>...
//       (n_strata * n_contigs counts, stratum-major; n_contigs lengths; n_strata caps)
//   -> "rc=<code> bad=<stratum>,<contig> batches=<stratum>:<first_contig>:<n_contigs>:<first_read>:<n_reads>:<positions>:<M>;..."
//      ("batches=-" when there is none)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "stratified_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind != 'p') continue;
        uint32_t n_strata = 0, n_contigs = 0;
        uint64_t max_reads = 0, max_positions = 0;
        std::string bar;
        in >> n_strata >> n_contigs >> max_reads >> max_positions >> bar;
        std::vector<uint64_t> counts((size_t)n_strata * n_contigs);
        std::vector<uint32_t> lengths(n_contigs), caps(n_strata);
        for (auto& v : counts) in >> v;
        in >> bar;
        for (auto& v : lengths) in >> v;
        in >> bar;
        for (auto& v : caps) in >> v;
        std::vector<qmcp::StratumBatch> out;
        uint32_t bad_s = 77, bad_c = 77;
        const int rc = qmcp::plan_stratum_batches(counts.data(), lengths.data(), n_contigs, caps.data(), n_strata, out,
                                                  &bad_s, &bad_c, max_reads, max_positions);
        std::printf("rc=%d bad=%u,%u batches=", rc, bad_s, bad_c);
        if (out.empty()) std::printf("-");
        for (size_t b = 0; b < out.size(); ++b)
            std::printf("%s%u:%u:%u:%llu:%llu:%llu:%u", b ? ";" : "", out[b].stratum, out[b].first_contig, out[b].n_contigs,
                        (unsigned long long)out[b].first_read, (unsigned long long)out[b].n_reads,
                        (unsigned long long)out[b].positions, out[b].M);
        std::printf("\n");
    }
    return 0;
}
