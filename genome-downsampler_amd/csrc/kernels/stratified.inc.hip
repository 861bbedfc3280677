// stratified.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after by_contig).
// Stratified downsampling (qmcp_hip_solve_stratified_*): every read carries a stratum id next to its contig id, and every
// stratum is a by-contig problem of its own with its own coverage cap.  Two kernels; the grouping, the gather and the
// scatter of the mask are radix_sort.inc.hip's and by_contig.inc.hip's.
//   k_st_keys   validation and the stratum-major grouping key  stratum * n_contigs + contig
//   k_st_tally  the per-stratum rows {reads, kept, bases in, bases kept}: a segmented reduction over the grouped records

// One pass over the four columns; a thread's loads are all issued before anything depends on them.  A read without a
// contig or without a stratum gets the key n_strata * n_contigs, which sorts behind every (stratum, contig) and is never
// solved; it is still validated.  err (one word, zeroed by the host): bits 0 and 1 as k_bc_keys sets them, bit 2 a
// stratum id that is neither < n_strata nor QMCP_NO_STRATUM.  COUNT_NONE (the tiered entry, whose tier column is a
// strata column): *none_count (zeroed by the host) += the reads whose id is QMCP_NO_STRATUM, reduced per wave -- one
// atomic per wave that saw any; without it the kernel is what it was.
template <bool COUNT_NONE>
__global__ __launch_bounds__(256) void k_st_keys(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                 const uint32_t* __restrict__ ids, const uint32_t* __restrict__ strata,
                                                 uint32_t n, const uint32_t* __restrict__ lengths, uint32_t n_contigs,
                                                 uint32_t n_strata, uint32_t* __restrict__ keys,
                                                 uint32_t* __restrict__ err,
                                                 unsigned long long* __restrict__ none_count) {
    uint32_t bad = 0, none = 0;
    const uint32_t unplaced = n_strata * n_contigs;  // <= 2^24 (checked by the host)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t id = ids[i], sid = strata[i], s = starts[i], e = ends[i];
        uint32_t key = unplaced;
        if (id < n_contigs) {
            if (s > e || e >= lengths[id]) bad |= 2u;
            if (sid < n_strata) key = sid * n_contigs + id;
        } else if (id != QMCP_NO_CONTIG) {
            bad |= 1u;
        }
        if (sid >= n_strata && sid != QMCP_NO_STRATUM) bad |= 4u;
        if (COUNT_NONE && sid == QMCP_NO_STRATUM) ++none;
        keys[i] = key;
    }
    if (bad) atomicOr(err, bad);
    if (COUNT_NONE) {
        none = wave_sum_u32(none);  // (a thread sees at most 2^31 / 2^19 reads: the wave's sum fits)
        if ((threadIdx.x & 63u) == 0 && none) atomicAdd(none_count, (unsigned long long)none);
    }
}

// One step of a wave64 segmented inclusive scan over lanes whose segment ids `seg` do not decrease with the lane: a lane
// takes its source lane's partial sums only when the source is in the same segment -- the lanes between the two then are
// too.  Lanes the DPP control leaves without a source see a segment id no lane holds.  cnt packs two counts (each at
// most 64 per wave) in its halves; the two 64-bit sums travel as halves.  Every lane of the wave must be active.
template <int CTRL, int RMASK>
__device__ __forceinline__ void st_seg_step(uint32_t seg, uint32_t& cnt, uint64_t& bin, uint64_t& bkept) {
    const uint32_t sseg = QMCP_DPP(0xFFFFFFFFu, seg, CTRL, RMASK);
    const uint32_t scnt = QMCP_DPP(0u, cnt, CTRL, RMASK);
    const uint32_t il = QMCP_DPP(0u, (uint32_t)bin, CTRL, RMASK);
    const uint32_t ih = QMCP_DPP(0u, (uint32_t)(bin >> 32), CTRL, RMASK);
    const uint32_t kl = QMCP_DPP(0u, (uint32_t)bkept, CTRL, RMASK);
    const uint32_t kh = QMCP_DPP(0u, (uint32_t)(bkept >> 32), CTRL, RMASK);
    const bool same = sseg == seg;
    cnt += same ? scnt : 0u;
    bin += same ? (((uint64_t)ih << 32) | il) : 0ull;
    bkept += same ? (((uint64_t)kh << 32) | kl) : 0ull;
}
__device__ __forceinline__ void st_seg_scan(uint32_t seg, uint32_t& cnt, uint64_t& bin, uint64_t& bkept) {
    st_seg_step<0x111, 0xF>(seg, cnt, bin, bkept);  // row_shr:1, 2, 4, 8 within the rows of 16 lanes
    st_seg_step<0x112, 0xF>(seg, cnt, bin, bkept);
    st_seg_step<0x114, 0xF>(seg, cnt, bin, bkept);
    st_seg_step<0x118, 0xF>(seg, cnt, bin, bkept);
    st_seg_step<0x142, 0xA>(seg, cnt, bin, bkept);  // row_bcast:15 into rows 1 and 3
    st_seg_step<0x143, 0xC>(seg, cnt, bin, bkept);  // row_bcast:31 into rows 2 and 3
}

// rows[4 * s ..]: {reads, kept reads, bases, kept bases} of stratum s, zeroed by the host.  `sorted` holds the n PLACED
// grouped records (key = stratum * n_contigs + contig, val = input index), so the strata do not decrease along it.
// A workgroup owns kStratumTallyTile consecutive records, each of its four waves kStratumTallyTile / 4 of them in
// kStTallyIters steps of 64 (a wave's loads stay contiguous).  Per record: the read's span and its bit of the final
// input-order mask.  Per step the wave's runs of equal stratum are reduced by the segmented DPP scan, a run that goes on
// into the next step is carried in registers, and the lane that ends a run (the next record is of another stratum, or
// the wave's records end) hands the run's sums on: to LDS when the stratum is the tile's first or its last -- those are
// the runs other waves and other workgroups may share --, straight to the row otherwise (such a stratum lies inside this
// tile, and a wave ends each stratum once).  After the barrier the two LDS sets go to their rows, four 64-bit atomics
// each: a workgroup that lies inside one stratum issues four atomics in all.
static constexpr int kStTallyIters = (int)(kStratumTallyTile / 4 / 64);
static_assert(kStratumTallyTile == 4u * 64u * (uint32_t)kStTallyIters, "four waves, whole steps of 64");

__global__ __launch_bounds__(256) void k_st_tally(const Rec* __restrict__ sorted, uint32_t n, uint32_t n_contigs,
                                                  const uint32_t* __restrict__ starts,
                                                  const uint32_t* __restrict__ ends,
                                                  const uint64_t* __restrict__ mask,
                                                  unsigned long long* __restrict__ rows) {
    __shared__ unsigned long long edge[8];  // the tile's first stratum's sums, then its last stratum's
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < 8) edge[threadIdx.x] = 0ull;
    const uint32_t tile0 = blockIdx.x * kStratumTallyTile;  // < n <= 2^31
    const uint32_t tile_end = min(n, tile0 + kStratumTallyTile);
    const uint32_t s_first = sorted[tile0].key / n_contigs;
    const uint32_t s_last = sorted[tile_end - 1u].key / n_contigs;
    __syncthreads();

    const uint32_t w0 = tile0 + wave * (kStratumTallyTile / 4);
    constexpr uint32_t kNone = 0xFFFFFFFEu;  // the stratum of a lane without a record
    Rec r[kStTallyIters];
    uint32_t rs[kStTallyIters], re[kStTallyIters];
    uint64_t rm[kStTallyIters];
#pragma unroll
    for (int it = 0; it < kStTallyIters; ++it) {
        const uint32_t g = w0 + (uint32_t)it * 64u + lane;
        r[it] = g < tile_end ? sorted[g] : Rec{0xFFFFFFFFu, 0u};
    }
#pragma unroll
    for (int it = 0; it < kStTallyIters; ++it) {
        const bool valid = r[it].key != 0xFFFFFFFFu;
        const uint32_t i = r[it].val;
        rs[it] = valid ? starts[i] : 1u;
        re[it] = valid ? ends[i] : 0u;
        rm[it] = valid ? mask[i >> 6] : 0ull;
    }
    uint32_t seg[kStTallyIters];
#pragma unroll
    for (int it = 0; it < kStTallyIters; ++it)
        seg[it] = r[it].key != 0xFFFFFFFFu ? r[it].key / n_contigs : kNone;

    uint32_t c_seg = 0xFFFFFFFFu, c_cnt = 0;  // the run the step before left open (wave-uniform)
    uint64_t c_bin = 0, c_bkept = 0;
#pragma unroll
    for (int it = 0; it < kStTallyIters; ++it) {
        const bool valid = seg[it] != kNone;
        const uint32_t kept = (uint32_t)(rm[it] >> (r[it].val & 63u)) & 1u;
        const uint64_t span = (uint64_t)(re[it] - rs[it]) + 1ull;
        uint32_t cnt = valid ? (1u | (kept << 16)) : 0u;
        uint64_t bin = valid ? span : 0ull;
        uint64_t bkept = (valid && kept) ? span : 0ull;
        st_seg_scan(seg[it], cnt, bin, bkept);
        if (seg[it] == c_seg) {
            cnt += c_cnt;
            bin += c_bin;
            bkept += c_bkept;
        }
        // the stratum of the record after this lane's: the next lane's, or the next step's first
        uint32_t next = (uint32_t)__shfl_down((int)seg[it], 1, kWave);
        const bool more = it + 1 < kStTallyIters;
        const uint32_t next_step = more ? (uint32_t)__shfl((int)seg[more ? it + 1 : it], 0, kWave) : 0xFFFFFFFFu;
        if (lane == 63u) next = next_step;
        if (valid && next != seg[it]) {
            const uint32_t s = seg[it];
            const unsigned long long v[4] = {cnt & 0xFFFFu, cnt >> 16, bin, bkept};
            if (s == s_first || s == s_last) {
                unsigned long long* dst = &edge[s == s_first ? 0 : 4];
#pragma unroll
                for (int k = 0; k < 4; ++k) atomicAdd(&dst[k], v[k]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (v[k]) atomicAdd(&rows[4ull * s + k], v[k]);
            }
        }
        c_seg = (uint32_t)__shfl((int)seg[it], 63, kWave);
        c_cnt = (uint32_t)__shfl((int)cnt, 63, kWave);
        c_bin = (uint64_t)__shfl((long long)bin, 63, kWave);
        c_bkept = (uint64_t)__shfl((long long)bkept, 63, kWave);
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        atomicAdd(&rows[4ull * s_first + threadIdx.x], edge[threadIdx.x]);
    } else if (threadIdx.x < 8 && s_last != s_first) {
        atomicAdd(&rows[4ull * s_last + (threadIdx.x - 4u)], edge[threadIdx.x]);
    }
}

void launch_st_keys(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                    const uint32_t* strata, uint32_t n, const uint32_t* lengths, uint32_t n_contigs, uint32_t n_strata,
                    uint32_t* keys, uint32_t* err, unsigned long long* none_count) {
    if (n == 0) return;
    if (none_count)
        hipLaunchKernelGGL(k_st_keys<true>, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, ends, ids, strata, n, lengths,
                           n_contigs, n_strata, keys, err, none_count);
    else
        hipLaunchKernelGGL(k_st_keys<false>, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, ends, ids, strata, n, lengths,
                           n_contigs, n_strata, keys, err, none_count);
}
void launch_st_tally(hipStream_t st, const void* sorted, uint32_t n_placed, uint32_t n_contigs, const uint32_t* starts,
                     const uint32_t* ends, const uint64_t* mask, uint64_t* rows) {
    if (n_placed == 0) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n_placed + kStratumTallyTile - 1) / kStratumTallyTile);
    hipLaunchKernelGGL(k_st_tally, dim3(blocks), dim3(256), 0, st, (const Rec*)sorted, n_placed, n_contigs, starts, ends,
                       mask, (unsigned long long*)rows);
}
