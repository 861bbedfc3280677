// Host-only driver of what genome-downsampler_amd/csrc/cap_table.h adds for the template-aware solve under caps (g++
// alone, no HIP): tests/test_templates_profile_cpu.py feeds it instances on stdin and checks what it prints.
//   scale <cap> <T> <M>                          prints "scaled <ceil(cap * T / M)>"
//   prefix <n_contigs> <n> <default_cap>
//   <n_contigs lengths> <n_contigs + 1 offsets> <n starts> <n ends> <n caps>
//                                                prints "rc <code>", and when the code is 0 one line per contig
//                                                "contig <c> :" followed by "rs before" pairs of its kept regions
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "cap_table.h"

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "scale") {
            uint32_t cap = 0, T = 0, M = 0;
            std::cin >> cap >> T >> M;
            std::printf("scaled %u\n", qmcp::scale_cap(cap, T, M));
            continue;
        }
        if (cmd != "prefix") return 2;
        uint32_t n_contigs = 0, n = 0, default_cap = 0;
        std::cin >> n_contigs >> n >> default_cap;
        std::vector<uint32_t> lengths(n_contigs), offs(n_contigs + 1), starts(n), ends(n), caps(n);
        for (auto& v : lengths) std::cin >> v;
        for (auto& v : offs) std::cin >> v;
        for (auto& v : starts) std::cin >> v;
        for (auto& v : ends) std::cin >> v;
        for (auto& v : caps) std::cin >> v;
        qmcp::CapTable t;
        const int rc = qmcp::build_cap_table(offs.data(), starts.data(), ends.data(), caps.data(), lengths.data(), n_contigs, t);
        std::printf("rc %d\n", rc);
        if (rc != 0) continue;
        std::vector<uint32_t> before;
        qmcp::cap_positive_before(t, default_cap, before);
        for (uint32_t c = 0; c < n_contigs; ++c) {
            std::printf("contig %u :", c);
            for (uint32_t k = t.offs[c]; k < t.offs[c + 1]; ++k) std::printf(" %u %u", t.rs[k], before[k]);
            std::printf("\n");
        }
    }
    return 0;
}
