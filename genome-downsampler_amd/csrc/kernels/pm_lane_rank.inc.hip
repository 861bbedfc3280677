// pm_lane_rank.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp).
// ------------------------------------------------------------------ pass-major producer: ranking by per-lane counts
// part_rank_rounds (ranked_route.inc.hip) pays for every digit bit of every record with a ballot and two mask words.
// Where a pass's digits span at most 32 ranges (k_pm_prepare_sort's match_bits <= 5) the stable rank of a record inside
// (wave, digit) is counted instead.  Lane l owns the wave's sixteen CONSECUTIVE reads [16 l, 16 l + 16), so the rank is
//     the records of the digit among the lane's own earlier records          (a)
//   + the records of the digit in the lower lanes of the wave                (b)
// and the cross-wave step on s_cnt that follows is the one part_rank_rounds feeds.
// The counts live in the wave's 4 KB of the stage (free until the scatter), laid out [digit pair][lane]: two 16-bit
// counters a word -- a wave holds 1 024 records, so neither a field nor a sum of fields over the lanes carries into its
// neighbour, and one 32-bit add or scan serves both digits of a pair.  No two lanes share a word in the counting, and a
// wave's LDS operations execute in order: the value a returning add hands back is (a), for both digits of the pair.
// (b) is an exclusive scan over the lanes, one DPP scan per pair word; it is stored one lane up, so that lane l later
// reads its exclusive prefix at its own slot, and lane 63's -- the wave's totals -- lands in slot 0, from where it goes
// to s_cnt before slot 0 is cleared for lane 0.  (tests/pm_lane_rank_model.py restates this on the host.)
typedef __attribute__((address_space(3))) uint32_t PmLdsWord;
typedef uint32_t PmQuad __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) PmQuad PmLdsQuad;

static constexpr uint32_t kPmLaneFormBits = 5;   // digit bits the form serves: 32 digits = 16 pair words a lane

// Between two phases that hand words from lane to lane through LDS: the hardware keeps a wave's LDS operations in
// order; this keeps the compiler from moving them across (no instruction is emitted).
__device__ __forceinline__ void pm_wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// rec[j]: the read first + j (j < 16), valid while first + j < bound; its digit is d_lo + rel with rel < 2 n_pairs <= 32.
// -> rank[j] inside (wave, digit); s_cnt_w[d] = the wave's records of digit d, for the digits the pair words cover.
// kFull: the pass is whole (every call's passes but the last), first + j < bound holds and is not asked.
template <bool kFull>
__device__ __forceinline__ void pm_rank_lane_counts(const Rec (&rec)[kSortItems], uint32_t (&rank)[kSortItems],
                                                    uint32_t first, uint32_t bound, uint32_t shift, uint32_t d_lo,
                                                    uint32_t n_pairs /* (uniform) 1 .. 16 */, int lane,
                                                    PmLdsWord* __restrict__ s_w /* the wave's 1 024 words of the stage */,
                                                    uint32_t* __restrict__ s_cnt_w /* the wave's 256 counters */) {
    static_assert(kSortItems == 16, "a lane's sixteen records: 64 lanes x 16 pair words fill the wave's share of the stage");
    // the rows are cleared, scanned and read four at a time: one 16-byte store a lane clears four rows
#pragma unroll
    for (uint32_t g = 0; g < 4; ++g)
        if (4u * g < n_pairs) ((PmLdsQuad*)s_w)[g * 64u + (uint32_t)lane] = (PmQuad)(0u);
    pm_wave_lds_order();
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const uint32_t rel = ((rec[j].key >> shift) & 255u) - d_lo;
        const uint32_t field = (rel & 1u) << 4;
        const uint32_t at = ((rel >> 1) & 15u) * 64u + (uint32_t)lane;   // (masked: never outside the wave's words)
        const uint32_t one = kFull || first + (uint32_t)j < bound ? 1u << field : 0u;
        rank[j] = __hip_atomic_fetch_add(s_w + at, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    pm_wave_lds_order();
#pragma unroll
    for (uint32_t g = 0; g < 4; ++g) {
        if (4u * g < n_pairs) {  // (uniform)
            uint32_t v[4];
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) v[t] = s_w[(4u * g + t) * 64u + (uint32_t)lane];
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) v[t] = wave_incl_scan_add(v[t]);
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) s_w[(4u * g + t) * 64u + (((uint32_t)lane + 1u) & 63u)] = v[t];
        }
    }
    pm_wave_lds_order();
    if (lane < 32) {
        const uint32_t r = (uint32_t)lane;
        if (r < 2u * n_pairs && d_lo + r < 256u) s_cnt_w[d_lo + r] = (s_w[(r >> 1) * 64u] >> ((r & 1u) << 4)) & 0xFFFFu;
    }
    pm_wave_lds_order();
    if ((uint32_t)lane < n_pairs) s_w[(uint32_t)lane * 64u] = 0u;
    pm_wave_lds_order();
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const uint32_t rel = ((rec[j].key >> shift) & 255u) - d_lo;
        const uint32_t field = (rel & 1u) << 4;
        const uint32_t at = ((rel >> 1) & 15u) * 64u + (uint32_t)lane;
        rank[j] = ((rank[j] + s_w[at]) >> field) & 0xFFFFu;
    }
    pm_wave_lds_order();   // (the stage is the workgroup's again only after the kernel's next barrier)
}
