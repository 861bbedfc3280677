// Host-only driver of genome-downsampler_amd/csrc/target_table.h (g++ alone, no HIP): tests/test_target_table_cpu.py
// feeds it instances on stdin and compares what it prints with tests/target_model.py.
//   table <mode> <n_contigs> <padding>      mode: ok | null_offsets | null_regions | null_lengths
//   <n_contigs lengths> <n_contigs + 1 offsets> <n starts> <n ends>     (n = the count the test says: next token)
//   <n_reads> then per read: contig start end
// prints  "rc <code>", and when the code is 0: "regions_in <a> regions_merged <b> positions <p>", one line per contig
// "contig <c> tlen <t> :" followed by "rs re cum" triples, and one line per read "read <on> <cs> <ce>".
//   spread <x>   prints spread_bits_by_4(x) and a bit-by-bit restatement
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "target_table.h"

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "spread") {
            unsigned long long x = 0;
            std::cin >> x;
            unsigned long long want = 0;
            for (int i = 0; i < 16; ++i) want |= ((x >> i) & 1ull) << (4 * i);
            std::printf("spread %llu %llu\n", (unsigned long long)qmcp::spread_bits_by_4(x), want);
            continue;
        }
        if (cmd != "table") return 2;
        std::string mode;
        uint32_t n_contigs = 0, padding = 0, n = 0;
        std::cin >> mode >> n_contigs >> padding >> n;
        std::vector<uint32_t> lengths(n_contigs), offs(n_contigs + 1), starts(n), ends(n);
        for (auto& v : lengths) std::cin >> v;
        for (auto& v : offs) std::cin >> v;
        for (auto& v : starts) std::cin >> v;
        for (auto& v : ends) std::cin >> v;
        uint32_t n_reads = 0;
        std::cin >> n_reads;
        std::vector<uint32_t> rc_(n_reads), rs_(n_reads), re_(n_reads);
        for (uint32_t i = 0; i < n_reads; ++i) std::cin >> rc_[i] >> rs_[i] >> re_[i];
        qmcp::TargetTable t;
        const int rc = qmcp::build_target_table(mode == "null_offsets" ? nullptr : offs.data(),
                                                mode == "null_regions" ? nullptr : starts.data(),
                                                mode == "null_regions" ? nullptr : ends.data(), padding,
                                                mode == "null_lengths" ? nullptr : lengths.data(), n_contigs, t);
        std::printf("rc %d\n", rc);
        if (rc != 0) continue;
        std::printf("regions_in %u regions_merged %u positions %llu\n", t.regions_in, t.regions_merged,
                    (unsigned long long)t.positions);
        for (uint32_t c = 0; c < n_contigs; ++c) {
            std::printf("contig %u tlen %u :", c, t.tlen[c]);
            for (uint32_t k = t.offs[c]; k < t.offs[c + 1]; ++k) std::printf(" %u %u %u", t.rs[k], t.re[k], t.cum[k]);
            std::printf("\n");
        }
        for (uint32_t i = 0; i < n_reads; ++i) {
            uint32_t cs = 0, ce = 0;
            const uint32_t c = rc_[i];
            const bool on = qmcp::project_read(t.rs.data(), t.re.data(), t.cum.data(), t.offs[c], t.offs[c + 1], rs_[i],
                                               re_[i], &cs, &ce);
            std::printf("read %d %u %u\n", on ? 1 : 0, on ? cs : 0u, on ? ce : 0u);
        }
    }
    return 0;
}
