// Driver of genome-downsampler_amd/host/include/qmcp-solver/adapter_columns.hpp for tests/test_adapter_columns_cpu.py
// (g++ alone, no HIP, no library).  One case per stdin line:
//   N <ids: 1 | 0 (null contig ids)> <n> then per read  <start> <end> [<contig id> when ids]
//       -> "placed=<p> bad=<b> starts=<s0,s1,...> ends=<e0,e1,...>"   (the columns start out as 0xDEADBEEF)
//   M <n> <k> <i_1> ... <i_k>
//       -> "words=<w0,w1,...>"                                        (hex)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "qmcp-solver/adapter_columns.hpp"

template <class T>
static void print_list(const char* name, const std::vector<T>& v, const char* format) {
    std::printf("%s=", name);
    for (std::size_t i = 0; i < v.size(); ++i) {
        if (i) std::printf(",");
        std::printf(format, (unsigned long long)v[i]);
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind = 0;
        unsigned long long n = 0;
        if (!(in >> kind)) continue;
        if (kind == 'N') {
            int with_ids = 0;
            in >> with_ids >> n;
            std::vector<bam_api::Index> starts(n), ends(n);
            std::vector<std::uint32_t> ids(n);
            for (unsigned long long i = 0; i < n; ++i) {
                in >> starts[i] >> ends[i];
                if (with_ids) in >> ids[i];
            }
            std::vector<std::uint32_t> out_starts(n, 0xDEADBEEFu), out_ends(n, 0xDEADBEEFu);
            const qmcp::Narrowed r = qmcp::narrow_columns(starts.data(), ends.data(), with_ids ? ids.data() : nullptr, n,
                                                          out_starts.data(), out_ends.data());
            std::printf("placed=%zu bad=%zu ", r.placed, r.bad);
            print_list("starts", out_starts, "%llu");
            std::printf(" ");
            print_list("ends", out_ends, "%llu");
            std::printf("\n");
        } else if (kind == 'M') {
            unsigned long long k = 0;
            in >> n >> k;
            std::vector<bam_api::ReadIndex> kept(k);
            for (unsigned long long j = 0; j < k; ++j) in >> kept[j];
            print_list("words", qmcp::keep_mask_of(kept, n), "%llx");
            std::printf("\n");
        }
    }
    return 0;
}
