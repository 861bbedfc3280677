// The two pure steps of the solver adapter (quasi_mcp_hip_solver.cpp): the reference's 64-bit coordinate columns
// narrowed to the uint32 columns of the C ABI, and a kept list turned into a keep mask.  No device, no library call:
// tests/cpp/adapter_columns_driver.cpp compiles this header with g++ alone.
#ifndef QMCP_AMD_ADAPTER_COLUMNS_HPP
#define QMCP_AMD_ADAPTER_COLUMNS_HPP

#include <cstddef>
#include <cstdint>
#include <vector>

#include "bam-api/read.hpp"
#include "qmcp_hip.h"

namespace qmcp {

struct Narrowed {
    std::size_t placed;  // reads with a contig (all of them without contig ids), up to `bad`
    std::size_t bad;     // the first placed read with a coordinate above UINT32_MAX; n: none
};

// starts / ends of n reads -> out_starts / out_ends, in one pass.  contig_ids null: every read is placed.  An unplaced
// read (QMCP_NO_CONTIG) is never kept: it goes over as 0 / 0 whatever its coordinates are.  Stops at the first bad read
inline Narrowed narrow_columns(const bam_api::Index* starts, const bam_api::Index* ends, const std::uint32_t* contig_ids,
                               std::size_t n, std::uint32_t* out_starts, std::uint32_t* out_ends) {
    std::size_t placed = 0;
    for (std::size_t i = 0; i < n; ++i) {
        if (contig_ids != nullptr && contig_ids[i] == QMCP_NO_CONTIG) {
            out_starts[i] = out_ends[i] = 0;
            continue;
        }
        if (starts[i] > UINT32_MAX || ends[i] > UINT32_MAX) return {placed, i};
        out_starts[i] = static_cast<std::uint32_t>(starts[i]);
        out_ends[i] = static_cast<std::uint32_t>(ends[i]);
        ++placed;
    }
    return {placed, n};
}

// the reads of `kept` (in any order, repeats allowed) as a keep mask of (n + 63) / 64 words; an index >= n is ignored
inline std::vector<std::uint64_t> keep_mask_of(const std::vector<bam_api::ReadIndex>& kept, std::size_t n) {
    std::vector<std::uint64_t> mask((n + 63) / 64, 0);
    for (const bam_api::ReadIndex i : kept)
        if (i < n) mask[i >> 6] |= 1ull << (i & 63);
    return mask;
}

}  // namespace qmcp
#endif
