// Host-only driver of genome-downsampler_amd/csrc/cap_table.h (g++ alone, no HIP): tests/test_profile_cpu.py feeds it
// instances on stdin and checks what it prints.
//   table <mode> <n_contigs> <n> <first> <count>      mode: ok | null_offsets | null_regions | null_lengths
//   <n_contigs lengths> <n_contigs + 1 offsets> <n starts> <n ends> <n caps>
// prints "rc <code>", and when the code is 0: "regions_in <a> regions_used <b> positions <p> max_cap <m>", one line per
// contig "contig <c> :" followed by "rs re cap" triples, and "batch :" followed by the "gs ge cap" triples of the
// contigs [first, first + count) on their concatenated position axis.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "cap_table.h"

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd != "table") return 2;
        std::string mode;
        uint32_t n_contigs = 0, n = 0, first = 0, count = 0;
        std::cin >> mode >> n_contigs >> n >> first >> count;
        std::vector<uint32_t> lengths(n_contigs), offs(n_contigs + 1), starts(n), ends(n), caps(n);
        for (auto& v : lengths) std::cin >> v;
        for (auto& v : offs) std::cin >> v;
        for (auto& v : starts) std::cin >> v;
        for (auto& v : ends) std::cin >> v;
        for (auto& v : caps) std::cin >> v;
        qmcp::CapTable t;
        const bool no_regions = mode == "null_regions";
        const int rc = qmcp::build_cap_table(mode == "null_offsets" ? nullptr : offs.data(),
                                             no_regions ? nullptr : starts.data(), no_regions ? nullptr : ends.data(),
                                             no_regions ? nullptr : caps.data(),
                                             mode == "null_lengths" ? nullptr : lengths.data(), n_contigs, t);
        std::printf("rc %d\n", rc);
        if (rc != 0) continue;
        std::printf("regions_in %u regions_used %u positions %llu max_cap %u\n", t.regions_in, t.regions_used,
                    (unsigned long long)t.positions, t.max_cap);
        for (uint32_t c = 0; c < n_contigs; ++c) {
            std::printf("contig %u :", c);
            for (uint32_t k = t.offs[c]; k < t.offs[c + 1]; ++k) std::printf(" %u %u %u", t.rs[k], t.re[k], t.cap[k]);
            std::printf("\n");
        }
        std::vector<uint32_t> gs, ge, gc;
        qmcp::batch_cap_table(t, lengths.data(), first, count, gs, ge, gc);
        std::printf("batch :");
        for (size_t k = 0; k < gs.size(); ++k) std::printf(" %u %u %u", gs[k], ge[k], gc[k]);
        std::printf("\n");
    }
    return 0;
}
