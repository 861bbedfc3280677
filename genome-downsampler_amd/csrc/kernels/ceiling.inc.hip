// ceiling.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after pairs).
// Ceiling downsampling (qmcp_hip_solve_ceiling_*): kept(p) <= cap(p) everywhere with the most reads kept.  The DROPPED set
// D is the canonical selection under need(p) = max(0, cov(p) - cap(p)), swept by the profile's capped sweeps; the answer
// is every placed read outside D.
//   k_ceiling_need     the dual of k_profile_need: need[p] = max(0, cov(p) - cap(p)), the cut bit where need(p) == cov(p)
//                      (cov == 0 or cap == 0: every read over p is in D), and three counters
//   k_ceiling_check    the same pass over a batch once D is marked: kept(p) = cov(p) - depth_D(p) against cap(p) and
//                      min(cov(p), cap(p)); four counters
//   k_ceiling_finish   over the mask words in input order: keep = placed & ~D, the mates of D's reads joined to D first
//                      when asked; three counters
// Counters (unsigned long long each, the CeilingStat words of qmcp_kernels.h): reduced per wave, then one atomic per
// workgroup.

// the sum of a per-thread total below 2^48 over the wave: three 16 / 16 / 32-bit parts, 64 lanes of each fit 32 bits
__device__ __forceinline__ unsigned long long wave_sum_u48(unsigned long long v) {
    const uint32_t lo = wave_sum_u32((uint32_t)(v & 0xFFFFu)), mid = wave_sum_u32((uint32_t)((v >> 16) & 0xFFFFu));
    const uint32_t hi = wave_sum_u32((uint32_t)(v >> 32));
    return (unsigned long long)lo + ((unsigned long long)mid << 16) + ((unsigned long long)hi << 32);
}

// The one pass behind k_ceiling_need and k_ceiling_check: profile_need_pass' shape -- a thread takes four consecutive
// positions at a time (16-byte loads of boff, eoff and, with kCheck, depth; without it one 16-byte store of need; the
// arrays are arena buffers, 256-byte aligned -- depth from its 16-byte aligned entry on), the last positions of the axis
// go one by one; the table in LDS ([rs | re | cap], n_regions each) with kLds, else read from global memory.
// kCheck: depth[p] is the depth of D; nothing is written but cst.
template <bool kLds, bool kCheck>
__device__ __forceinline__ void ceiling_pass(const uint32_t* __restrict__ boff, const uint32_t* __restrict__ eoff,
                                             const uint32_t* __restrict__ depth, uint32_t ltot,
                                             const uint32_t* __restrict__ g_rs, const uint32_t* __restrict__ g_re,
                                             const uint32_t* __restrict__ g_cap, uint32_t n_regions, uint32_t default_cap,
                                             uint32_t* __restrict__ need, unsigned long long* __restrict__ cst) {
    extern __shared__ uint32_t s_cap_tab[];
    __shared__ unsigned long long s_acc[4];  // counts a, b; sum; max
    const uint32_t* rs = g_rs;
    const uint32_t* re = g_re;
    const uint32_t* cp = g_cap;
    if (threadIdx.x < 4) s_acc[threadIdx.x] = 0;
    if constexpr (kLds) {
        for (uint32_t i = threadIdx.x; i < n_regions; i += blockDim.x) {
            s_cap_tab[i] = g_rs[i];
            s_cap_tab[n_regions + i] = g_re[i];
            s_cap_tab[2 * n_regions + i] = g_cap[i];
        }
        rs = s_cap_tab;
        re = s_cap_tab + n_regions;
        cp = s_cap_tab + 2 * n_regions;
    }
    __syncthreads();
    const uint32_t n_groups = (ltot + 3u) / 4u;
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t count_a = 0, count_b = 0, largest = 0;  // need: over positions, -; check: excess, short positions
    unsigned long long sum = 0;                      // need: the sum of need; check: the sum of the shortfall
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += stride) {
        const uint32_t p0 = 4u * g;
        uint32_t cov[4], dd[4] = {0u, 0u, 0u, 0u};
        const bool whole = p0 + 3u < ltot;  // (then boff[p0 + 4] exists: boff has ltot + 1 entries)
        if (whole) {
            const uint4 b = *(const uint4*)(boff + p0), e = *(const uint4*)(eoff + p0);
            const uint32_t b4 = boff[p0 + 4];
            cov[0] = b.y - e.x; cov[1] = b.z - e.y; cov[2] = b.w - e.z; cov[3] = b4 - e.w;  // cov(p) = boff[p + 1] - eoff[p]
            if constexpr (kCheck) {
                const uint4 d = *(const uint4*)(depth + p0);
                dd[0] = d.x; dd[1] = d.y; dd[2] = d.z; dd[3] = d.w;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool in = p0 + r < ltot;
                cov[r] = in ? boff[p0 + r + 1] - eoff[p0 + r] : 0u;
                if constexpr (kCheck) dd[r] = in ? depth[p0 + r] : 0u;
            }
        }
        uint32_t k = profile_first_region(re, n_regions, p0);
        uint32_t out[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t p = p0 + (uint32_t)r;
            while (k < n_regions && re[k] < p) ++k;
            const uint32_t cap = (k < n_regions && rs[k] <= p) ? cp[k] : default_cap;
            const bool in = p < ltot;
            if constexpr (kCheck) {
                const uint32_t kept = cov[r] - dd[r];  // D holds placed reads only: depth_D <= cov
                const uint32_t floor_p = min(cov[r], cap);
                if (in) {
                    count_a += kept > cap ? 1u : 0u;
                    count_b += kept < floor_p ? 1u : 0u;
                    sum += kept < floor_p ? floor_p - kept : 0u;
                    largest = max(largest, kept);
                }
            } else {
                const uint32_t nd = cov[r] > cap ? cov[r] - cap : 0u;
                out[r] = nd | ((cov[r] == 0u || cap == 0u) ? kNeedCutBit : 0u);  // need(p) == cov(p)
                if (in) {
                    count_a += nd != 0u ? 1u : 0u;
                    sum += nd;
                    largest = max(largest, nd);
                }
            }
        }
        if constexpr (!kCheck) {
            if (whole) {
                *(uint4*)(need + p0) = make_uint4(out[0], out[1], out[2], out[3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (p0 + r < ltot) need[p0 + r] = out[r];
            }
        }
    }
    count_a = wave_sum_u32(count_a);
    count_b = wave_sum_u32(count_b);
    largest = wave_max_u32(largest);
    sum = wave_sum_u48(sum);
    if ((threadIdx.x & 63u) == 0) {
        if (count_a) atomicAdd(&s_acc[0], (unsigned long long)count_a);
        if (count_b) atomicAdd(&s_acc[1], (unsigned long long)count_b);
        if (sum) atomicAdd(&s_acc[2], sum);
        if (largest) atomicMax(&s_acc[3], (unsigned long long)largest);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (kCheck) {
            if (s_acc[0]) atomicAdd(&cst[kCeilExcessPositions], s_acc[0]);
            if (s_acc[1]) atomicAdd(&cst[kCeilShortPositions], s_acc[1]);
            if (s_acc[2]) atomicAdd(&cst[kCeilShortBases], s_acc[2]);
            if (s_acc[3]) atomicMax(&cst[kCeilMaxKept], s_acc[3]);
        } else {
            if (s_acc[0]) atomicAdd(&cst[kCeilOverPositions], s_acc[0]);
            if (s_acc[2]) atomicAdd(&cst[kCeilOverBases], s_acc[2]);
            if (s_acc[3]) atomicMax(&cst[kCeilMaxNeed], s_acc[3]);
        }
    }
}

template <bool kLds>
__global__ __launch_bounds__(256) void k_ceiling_need(const uint32_t* __restrict__ boff, const uint32_t* __restrict__ eoff,
                                                      uint32_t ltot, const uint32_t* __restrict__ g_rs,
                                                      const uint32_t* __restrict__ g_re, const uint32_t* __restrict__ g_cap,
                                                      uint32_t n_regions, uint32_t default_cap, uint32_t* __restrict__ need,
                                                      unsigned long long* __restrict__ cst) {
    ceiling_pass<kLds, false>(boff, eoff, nullptr, ltot, g_rs, g_re, g_cap, n_regions, default_cap, need, cst);
}

template <bool kLds>
__global__ __launch_bounds__(256) void k_ceiling_check(const uint32_t* __restrict__ boff, const uint32_t* __restrict__ eoff,
                                                       const uint32_t* __restrict__ depth, uint32_t ltot,
                                                       const uint32_t* __restrict__ g_rs, const uint32_t* __restrict__ g_re,
                                                       const uint32_t* __restrict__ g_cap, uint32_t n_regions,
                                                       uint32_t default_cap, unsigned long long* __restrict__ cst) {
    ceiling_pass<kLds, true>(boff, eoff, depth, ltot, g_rs, g_re, g_cap, n_regions, default_cap, nullptr, cst);
}

// mask holds D in input order and leaves as the keep mask.  A wave takes 256 consecutive reads -- four mask words -- at a
// time: a lane loads the ids of four reads (one 16-byte load with kVec: ids is then 16-byte aligned; the reads past
// n_reads go one by one) into a nibble of placed bits, sixteen lanes OR their nibbles into one word, and the first lane
// of each sixteen rewrites that word.  kPairs: reads (2q, 2q + 1) are mates, and a read whose mate is in D joins D.
template <bool kVec, bool kPairs>
__global__ __launch_bounds__(256) void k_ceiling_finish(const uint32_t* __restrict__ ids, uint64_t n_reads,
                                                        uint64_t* __restrict__ mask, unsigned long long* __restrict__ cst) {
    __shared__ unsigned long long s_acc[4];
    if (threadIdx.x < 4) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = (n_reads + 255u) / 256u;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    const uint64_t even = 0x5555555555555555ull;
    uint32_t placed_n = 0, kept_n = 0, mates_n = 0;  // (a lane counts at most 2^31 reads)
    for (uint64_t ch = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); ch < n_chunks; ch += waves) {
        const uint64_t i0 = 256u * ch + 4u * lane;
        uint32_t id[4] = {QMCP_NO_CONTIG, QMCP_NO_CONTIG, QMCP_NO_CONTIG, QMCP_NO_CONTIG};
        if (kVec && i0 + 3u < n_reads) {
            const uint4 v = *(const uint4*)(ids + i0);
            id[0] = v.x; id[1] = v.y; id[2] = v.z; id[3] = v.w;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (i0 + r < n_reads) id[r] = ids[i0 + r];
        }
        uint64_t placed = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) placed |= (uint64_t)(id[r] != QMCP_NO_CONTIG ? 1u : 0u) << r;
        placed <<= 4u * (lane & 15u);
#pragma unroll
        for (int s = 1; s < 16; s <<= 1) placed |= (uint64_t)__shfl_xor((unsigned long long)placed, s, 64);
        const uint64_t w = 4u * ch + (lane >> 4);
        if ((lane & 15u) == 0 && 64u * w < n_reads) {
            const uint64_t d = mask[w];
            uint64_t dp = d;
            if constexpr (kPairs) dp |= ((d & even) << 1) | ((d >> 1) & even);
            const uint64_t keep = placed & ~dp;
            mask[w] = keep;
            placed_n += (uint32_t)__popcll(placed);
            kept_n += (uint32_t)__popcll(keep);
            mates_n += (uint32_t)__popcll(placed & dp & ~d);
        }
    }
    placed_n = wave_sum_u32(placed_n);
    kept_n = wave_sum_u32(kept_n);
    mates_n = wave_sum_u32(mates_n);
    if (lane == 0) {
        if (placed_n) atomicAdd(&s_acc[0], (unsigned long long)placed_n);
        if (kept_n) atomicAdd(&s_acc[1], (unsigned long long)kept_n);
        if (mates_n) atomicAdd(&s_acc[2], (unsigned long long)mates_n);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_acc[0]) atomicAdd(&cst[kCeilPlaced], s_acc[0]);
        if (s_acc[1]) atomicAdd(&cst[kCeilKept], s_acc[1]);
        if (s_acc[2]) atomicAdd(&cst[kCeilMatesDropped], s_acc[2]);
    }
}

void launch_ceiling_need(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, uint32_t ltot, const uint32_t* rs,
                         const uint32_t* re, const uint32_t* cap, uint32_t n_regions, uint32_t default_cap, uint32_t* need,
                         unsigned long long* cst) {
    if (ltot == 0) return;
    const dim3 grid(grid_for(((uint64_t)ltot + 3) / 4, 256)), block(256);
    if (n_regions <= kProfileLdsMax)
        hipLaunchKernelGGL(k_ceiling_need<true>, grid, block, 3 * (size_t)n_regions * sizeof(uint32_t), st, boff, eoff, ltot,
                           rs, re, cap, n_regions, default_cap, need, cst);
    else
        hipLaunchKernelGGL(k_ceiling_need<false>, grid, block, 0, st, boff, eoff, ltot, rs, re, cap, n_regions,
                           default_cap, need, cst);
}

void launch_ceiling_check(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, const uint32_t* depth, uint32_t ltot,
                          const uint32_t* rs, const uint32_t* re, const uint32_t* cap, uint32_t n_regions,
                          uint32_t default_cap, unsigned long long* cst) {
    if (ltot == 0) return;
    const dim3 grid(grid_for(((uint64_t)ltot + 3) / 4, 256)), block(256);
    if (n_regions <= kProfileLdsMax)
        hipLaunchKernelGGL(k_ceiling_check<true>, grid, block, 3 * (size_t)n_regions * sizeof(uint32_t), st, boff, eoff,
                           depth, ltot, rs, re, cap, n_regions, default_cap, cst);
    else
        hipLaunchKernelGGL(k_ceiling_check<false>, grid, block, 0, st, boff, eoff, depth, ltot, rs, re, cap, n_regions,
                           default_cap, cst);
}

void launch_ceiling_finish(hipStream_t st, const uint32_t* ids, uint64_t n_reads, bool whole_pairs, uint64_t* mask,
                           unsigned long long* cst) {
    if (n_reads == 0) return;
    const dim3 grid(grid_for((n_reads + 255) / 256, 4)), block(256);
    const bool vec = ((uintptr_t)ids & 15u) == 0;
#define QMCP_CEIL_FINISH(VEC, PAIRS) \
    hipLaunchKernelGGL((k_ceiling_finish<VEC, PAIRS>), grid, block, 0, st, ids, n_reads, mask, cst)
    if (vec) {
        if (whole_pairs) QMCP_CEIL_FINISH(true, true);
        else QMCP_CEIL_FINISH(true, false);
    } else {
        if (whole_pairs) QMCP_CEIL_FINISH(false, true);
        else QMCP_CEIL_FINISH(false, false);
    }
#undef QMCP_CEIL_FINISH
}
