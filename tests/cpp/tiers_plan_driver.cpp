// Driver of genome-downsampler_amd/csrc/tiers_plan.h for tests/test_tiers_cpu.py (g++ alone, no HIP).
// One request per stdin line:
//   c <has_lengths> <n_contigs> <has_tiers> <n_tiers> <M> <n_reads>
//   -> "rc=<code> why=<TierRefusal>"
//   p <n_tiers> <n_contigs> <M> <max_reads> <max_positions> | <count>... | <length>...
//       (n_tiers * n_contigs counts, tier-major; n_contigs lengths)
//   -> "rc=<code> bad=<tier>,<contig> batches=<tier>:<first_contig>:<n_contigs>:<first_read>:<n_reads>:<positions>;..."
//      ("batches=-" when there is none)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tiers_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind == 'c') {
            int has_lengths = 0, has_tiers = 0;
            uint32_t n_contigs = 0, n_tiers = 0;
            uint64_t M = 0, n_reads = 0;
            in >> has_lengths >> n_contigs >> has_tiers >> n_tiers >> M >> n_reads;
            qmcp::TierRefusal why = qmcp::kTierCallOk;
            const int rc = qmcp::check_tiers_call(has_lengths != 0, n_contigs, has_tiers != 0, n_tiers, (uint32_t)M, n_reads, &why);
            std::printf("rc=%d why=%u\n", rc, (unsigned)why);
            continue;
        }
        if (kind != 'p') continue;
        uint32_t n_tiers = 0, n_contigs = 0, M = 0;
        uint64_t max_reads = 0, max_positions = 0;
        std::string bar;
        in >> n_tiers >> n_contigs >> M >> max_reads >> max_positions >> bar;
        std::vector<uint64_t> counts((size_t)n_tiers * n_contigs);
        std::vector<uint32_t> lengths(n_contigs);
        for (auto& v : counts) in >> v;
        in >> bar;
        for (auto& v : lengths) in >> v;
        std::vector<qmcp::TierBatch> out;
        uint32_t bad_t = 77, bad_c = 77;
        const int rc = qmcp::plan_tier_batches(counts.data(), lengths.data(), n_contigs, n_tiers, M, out, &bad_t, &bad_c,
                                               max_reads, max_positions);
        std::printf("rc=%d bad=%u,%u batches=", rc, bad_t, bad_c);
        if (out.empty()) std::printf("-");
        for (size_t b = 0; b < out.size(); ++b) {
            if (out[b].M != M) return 3;  // every batch is solved at the call's M
            std::printf("%s%u:%u:%u:%llu:%llu:%llu", b ? ";" : "", out[b].stratum, out[b].first_contig, out[b].n_contigs,
                        (unsigned long long)out[b].first_read, (unsigned long long)out[b].n_reads,
                        (unsigned long long)out[b].positions);
        }
        std::printf("\n");
    }
    return 0;
}
