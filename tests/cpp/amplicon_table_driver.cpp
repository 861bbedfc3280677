// Drives genome-downsampler_amd/csrc/amplicon_table.h for tests/test_amplicons_by_reference_cpu.py (g++ only, no HIP).
// stdin, one case after another:
//   n_contigs n_amplicons
//   offsets (n_contigs + 1 numbers)  starts (n_amplicons)  ends (n_amplicons)
//   n_queries, then n_queries lines "c s1 e1 s2 e2"
// stdout, one line per case: "rc=<build_amplicon_table's code> <one 0/1 per query>" (no bits when rc != 0)
#include <cstdint>
#include <iostream>
#include <string>
#include <vector>

#include "amplicon_table.h"

int main() {
    uint64_t n_contigs = 0, n_amp = 0;
    while (std::cin >> n_contigs >> n_amp) {
        std::vector<uint32_t> offs(n_contigs + 1), starts(n_amp), ends(n_amp);
        for (auto& x : offs) std::cin >> x;
        for (auto& x : starts) std::cin >> x;
        for (auto& x : ends) std::cin >> x;
        uint64_t n_q = 0;
        std::cin >> n_q;
        std::vector<uint32_t> q(5 * n_q);
        for (auto& x : q) std::cin >> x;
        const int check = qmcp::check_amplicon_offsets(offs.data(), (uint32_t)n_contigs, n_amp);
        std::vector<uint32_t> ts, tp;
        int rc = check;
        if (rc == QMCP_OK) rc = qmcp::build_amplicon_table(offs.data(), starts.data(), ends.data(), (uint32_t)n_contigs, ts, tp);
        std::string bits;
        if (rc == QMCP_OK) {
            bits.reserve(n_q);
            for (uint64_t i = 0; i < n_q; ++i) {
                const uint32_t* r = &q[5 * i];
                bits += qmcp::pair_in_one_amplicon(offs.data(), ts.data(), tp.data(), r[0], r[1], r[2], r[3], r[4]) ? '1' : '0';
            }
        }
        std::cout << "rc=" << rc << " " << bits << "\n";
    }
    return 0;
}
