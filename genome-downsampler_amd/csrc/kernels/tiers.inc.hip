// tiers.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after pairs).
// Tiered downsampling (qmcp_hip_solve_tiers_*): the best tier first, a later tier tops the kept set up to M against the
// depth the earlier tiers' kept reads already give.  The grouping, the gather, the mask's scatter and the rows are
// radix_sort.inc.hip's, by_contig.inc.hip's and stratified.inc.hip's (k_st_tally: a tier is a stratum there).
//   k_tier_keep_list       the kept reads of one solved batch appended to the call's kept list as {contig, start, end, 0}
//   k_tier_credit_events   +1 at the global start, -1 behind the global end of the list's entries on a batch's contigs;
//                          the scan of these events is credit[p], the depth of the earlier tiers' kept reads at p
// The keys are k_st_keys<true> (kernels/stratified.inc.hip: a tier column is a strata column, and the reads without a
// tier are counted), need[] is k_pair_need<true> (kernels/pairs.inc.hip, with the positions that ask counted).
// Both stream: grid-stride loops of 256 threads, no LDS.

// One entry of the kept list is a uint4 {contig, start, end, 0}: 16 bytes, so that an entry is one aligned load or store.
static_assert(sizeof(uint4) == kTierKeptBytes, "one 16-byte load per entry");

// The kept reads of a solved batch, in grouped order (contig order is kept), appended at `out` (the caller's list plus
// the entries it holds).  k_ladder_compact's walk: a thread owns four consecutive reads -- one nibble of a mask word --
// and leaves without touching the columns when none is kept, which is nearly always on deep data.  Kept read i becomes
// entry word_base[i / 64] + (set bits of its word below it).  key_base: tier * n_contigs of the batch's tier.  room: the
// entries `out` has space for -- the kept count the solve reported, which is the mask's popcount.
__global__ __launch_bounds__(256) void k_tier_keep_list(const uint32_t* __restrict__ starts,
                                                        const uint32_t* __restrict__ ends,
                                                        const Rec* __restrict__ recs, const uint64_t* __restrict__ mask,
                                                        const uint32_t* __restrict__ word_base, uint32_t n,
                                                        uint32_t key_base, uint4* __restrict__ out, uint32_t room) {
    const uint32_t n_quads = (n + 3u) / 4u;  // (n <= 2^30)
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n_quads; q += gridDim.x * blockDim.x) {
        const uint32_t i0 = 4u * q;
        const uint64_t word = mask[i0 >> 6];
        const uint32_t bit = i0 & 63u;
        const uint32_t left = n - i0;  // reads of this quad that exist: >= 1
        const uint32_t nib = (uint32_t)(word >> bit) & (left >= 4u ? 0xFu : (1u << left) - 1u);
        if (nib == 0) continue;
        uint32_t dst = word_base[i0 >> 6] + (uint32_t)__popcll(word & ((1ull << bit) - 1ull));
#pragma unroll
        for (uint32_t r = 0; r < 4u; ++r) {
            if (((nib >> r) & 1u) && dst < room) {
                out[dst] = make_uint4(recs[i0 + r].key - key_base, starts[i0 + r], ends[i0 + r], 0u);
                ++dst;
            }
        }
    }
}

// ev is k_pair_credit_events' axis (zeroed, kPairCreditPad + positions words, shifted by kPairCreditPad - 1 entries:
// the in-place exclusive scan leaves credit[p] at ev[kPairCreditPad + p]).  The list holds the kept reads of every
// earlier tier on every contig; an entry counts when its contig is one of the batch's n_contigs from first_contig
// (pos_off: their batch-local position offsets).  The reads were validated by k_st_keys, so start <= end < the
// contig's length and both cells lie inside the axis.  The axis is touched twice per kept read and by nothing else.
__global__ __launch_bounds__(256) void k_tier_credit_events(const uint4* __restrict__ list, uint32_t n_list,
                                                            uint32_t first_contig, uint32_t n_contigs,
                                                            const uint32_t* __restrict__ pos_off,
                                                            uint32_t* __restrict__ ev) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_list; j += gridDim.x * blockDim.x) {
        const uint4 r = list[j];
        const uint32_t k = r.x - first_contig;  // (wraps above n_contigs for a contig before the batch's)
        if (k < n_contigs) {
            const uint32_t base = pos_off[k] + (kPairCreditPad - 1u);
            atomicAdd(&ev[base + r.y], 1u);
            atomicAdd(&ev[base + r.z + 1u], 0xFFFFFFFFu);
        }
    }
}

void launch_tier_keep_list(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const void* sorted,
                           const uint64_t* mask, const uint32_t* word_base, uint32_t n, uint32_t key_base, void* out,
                           uint32_t room) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_tier_keep_list, dim3(grid_for(((uint64_t)n + 3) / 4, 256)), dim3(256), 0, st, starts, ends,
                       (const Rec*)sorted, mask, word_base, n, key_base, (uint4*)out, room);
}

void launch_tier_credit_events(hipStream_t st, const void* list, uint32_t n_list, uint32_t first_contig, uint32_t n_contigs,
                               const uint32_t* pos_off, uint32_t* ev) {
    if (n_list == 0) return;
    hipLaunchKernelGGL(k_tier_credit_events, dim3(grid_for(n_list, 256)), dim3(256), 0, st, (const uint4*)list, n_list,
                       first_contig, n_contigs, pos_off, ev);
}
