// pairs.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after profile).
// Pair-aware downsampling (qmcp_hip_solve_pairs_*): a stage after the first tops the kept set S up to its target T
// against the depth S already gives.  Per batch of the by-contig grouping:
//   k_pair_gather_mask     the input-order mask of S as bits in the batch's grouped order (the inverse of
//                          k_bc_scatter_mask), and its complement inside the batch: the stage's candidates
//   k_pair_credit_events   +1 at the global start, -1 behind the global end of the batch's reads in S; the scan of
//                          these events is credit[p], the depth of S at p
//   k_pair_need            k_profile_need with cap(p) = max(0, T - credit[p]): need[p] = min(cov_rest(p), cap(p)) over
//                          the candidates' boff / eoff, its cut bit, and the two counters
//   k_pair_count_bits      |S|: the popcount of a mask
// The candidates are compacted by the ladder's kernels, swept by the profile's capped sweeps and their bits go back to
// input order through k_expand_mask_reads.

// One wave turns 64 grouped records into one word with a ballot.  n <= 2^30, so the word count fits 32 bits.
__global__ __launch_bounds__(256) void k_pair_gather_mask(const Rec* __restrict__ sorted, uint32_t n,
                                                          const uint64_t* __restrict__ mask,
                                                          uint64_t* __restrict__ in_bits, uint64_t* __restrict__ rest_bits) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_words = (n + 63u) / 64u;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_words; w += waves) {
        const uint32_t j = 64u * w + lane;
        bool in = false;
        if (j < n) {
            const uint32_t i = sorted[j].val;
            in = ((mask[i >> 6] >> (i & 63u)) & 1ull) != 0;
        }
        const uint64_t word = __ballot(in);
        const uint32_t live = n - 64u * w;  // records of this word that exist: >= 1
        const uint64_t valid = live >= 64u ? ~0ull : ((1ull << live) - 1ull);
        if (lane == 0) {
            in_bits[w] = word;
            rest_bits[w] = ~word & valid;
        }
    }
}

// ev (zeroed, kPairCreditPad + positions + 1 words) is shifted by kPairCreditPad - 1 entries: the exclusive scan of the
// buffer then holds the INCLUSIVE sum of position p's events at entry p + kPairCreditPad, a 16-byte aligned array.
// Reads never leave their contig (k_bc_keys checked them), so gs <= ge < positions.  The -1 is +0xFFFFFFFF: the sums
// wrap and come out right, also where a -1 and a +1 meet in one cell.
constexpr uint32_t kPairCreditPad = 4;
__global__ __launch_bounds__(256) void k_pair_credit_events(const Rec* __restrict__ sorted, uint32_t n,
                                                            const uint64_t* __restrict__ in_bits,
                                                            const uint32_t* __restrict__ starts,
                                                            const uint32_t* __restrict__ ends,
                                                            const uint32_t* __restrict__ pos_off, uint32_t first_contig,
                                                            uint32_t* __restrict__ ev) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        if ((in_bits[j >> 6] >> (j & 63u)) & 1ull) {
            const uint32_t base = pos_off[sorted[j].key - first_contig] + (kPairCreditPad - 1u);
            atomicAdd(&ev[base + starts[j]], 1u);
            atomicAdd(&ev[base + ends[j] + 1u], 0xFFFFFFFFu);
        }
    }
}

// k_profile_need's shape: four positions per thread, 16-byte loads of boff, eoff and credit, one 16-byte store; the
// last positions of the axis go one by one.  pstat: [0] positions with cov_rest > cap, [1] the sum of need; ASKED (the
// tiered entry): [2] the positions with need > 0 as well -- without it the kernel is what it was.
template <bool ASKED>
__global__ __launch_bounds__(256) void k_pair_need(const uint32_t* __restrict__ boff, const uint32_t* __restrict__ eoff,
                                                   const uint32_t* __restrict__ credit, uint32_t ltot, uint32_t target,
                                                   uint32_t* __restrict__ need, unsigned long long* __restrict__ pstat) {
    __shared__ unsigned long long s_acc[3];
    if (threadIdx.x < 3) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t n_groups = (ltot + 3u) / 4u;
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t capped = 0, asked = 0;
    unsigned long long demand = 0;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += stride) {
        const uint32_t p0 = 4u * g;
        uint32_t cov[4], cr[4];
        const bool whole = p0 + 3u < ltot;  // (then boff[p0 + 4] exists: boff has ltot + 1 entries)
        if (whole) {
            const uint4 b = *(const uint4*)(boff + p0), e = *(const uint4*)(eoff + p0), c = *(const uint4*)(credit + p0);
            const uint32_t b4 = boff[p0 + 4];
            cov[0] = b.y - e.x; cov[1] = b.z - e.y; cov[2] = b.w - e.z; cov[3] = b4 - e.w;  // cov(p) = boff[p + 1] - eoff[p]
            cr[0] = c.x; cr[1] = c.y; cr[2] = c.z; cr[3] = c.w;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool in = p0 + r < ltot;
                cov[r] = in ? boff[p0 + r + 1] - eoff[p0 + r] : 0u;
                cr[r] = in ? credit[p0 + r] : 0u;
            }
        }
        uint32_t out[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t cap = target > cr[r] ? target - cr[r] : 0u;
            const uint32_t nd = min(cov[r], cap);
            out[r] = nd | (cov[r] <= cap ? kNeedCutBit : 0u);
            if (p0 + (uint32_t)r < ltot) {
                capped += cov[r] > cap ? 1u : 0u;
                if (ASKED) asked += nd != 0u ? 1u : 0u;
                demand += nd;
            }
        }
        if (whole) {
            *(uint4*)(need + p0) = make_uint4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (p0 + r < ltot) need[p0 + r] = out[r];
        }
    }
    capped = wave_sum_u32(capped);
    if (ASKED) asked = wave_sum_u32(asked);
    const uint32_t d_lo = wave_sum_u32((uint32_t)(demand & 0xFFFFu)), d_mid = wave_sum_u32((uint32_t)((demand >> 16) & 0xFFFFu));
    const uint32_t d_hi = wave_sum_u32((uint32_t)(demand >> 32));  // (a thread's sum stays far below 2^48: 64 lanes of 16 bits fit)
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(&s_acc[0], (unsigned long long)capped);
        atomicAdd(&s_acc[1], (unsigned long long)d_lo + ((unsigned long long)d_mid << 16) + ((unsigned long long)d_hi << 32));
        if (ASKED) atomicAdd(&s_acc[2], (unsigned long long)asked);
    }
    __syncthreads();
    if (threadIdx.x == 0 && (s_acc[0] | s_acc[1]) != 0) {
        if (s_acc[0]) atomicAdd(&pstat[0], s_acc[0]);
        if (s_acc[1]) atomicAdd(&pstat[1], s_acc[1]);
        if (ASKED && s_acc[2]) atomicAdd(&pstat[2], s_acc[2]);  // (need > 0 somewhere: the demand is not 0 either)
    }
}

// *count += the set bits of n_words words: reduced per wave, one atomic per workgroup
__global__ __launch_bounds__(256) void k_pair_count_bits(const uint64_t* __restrict__ mask, uint32_t n_words,
                                                         unsigned long long* __restrict__ count) {
    __shared__ uint32_t s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    uint32_t bits = 0;  // (a thread sees at most 2^25 / 2^19 words of 64 bits: no overflow)
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += gridDim.x * blockDim.x)
        bits += (uint32_t)__popcll(mask[w]);
    bits = wave_sum_u32(bits);
    if ((threadIdx.x & 63u) == 0 && bits) atomicAdd(&s_sum, bits);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(count, (unsigned long long)s_sum);
}

uint32_t pair_credit_pad() { return kPairCreditPad; }

void launch_pair_gather_mask(hipStream_t st, const void* sorted, uint32_t n, const uint64_t* mask, uint64_t* in_bits,
                             uint64_t* rest_bits) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_pair_gather_mask, dim3(grid_for(((uint64_t)n + 63) / 64, 4)), dim3(256), 0, st, (const Rec*)sorted, n,
                       mask, in_bits, rest_bits);
}

void launch_pair_credit_events(hipStream_t st, const void* sorted, uint32_t n, const uint64_t* in_bits,
                               const uint32_t* starts, const uint32_t* ends, const uint32_t* pos_off, uint32_t first_contig,
                               uint32_t* ev) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_pair_credit_events, dim3(grid_for(n, 256)), dim3(256), 0, st, (const Rec*)sorted, n, in_bits, starts,
                       ends, pos_off, first_contig, ev);
}

void launch_pair_need(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, const uint32_t* credit, uint32_t ltot,
                      uint32_t target, uint32_t* need, unsigned long long* pstat, bool count_asked) {
    if (ltot == 0) return;
    const dim3 grid(grid_for(((uint64_t)ltot + 3) / 4, 256)), block(256);
    if (count_asked)
        hipLaunchKernelGGL(k_pair_need<true>, grid, block, 0, st, boff, eoff, credit, ltot, target, need, pstat);
    else
        hipLaunchKernelGGL(k_pair_need<false>, grid, block, 0, st, boff, eoff, credit, ltot, target, need, pstat);
}

void launch_pair_count_bits(hipStream_t st, const uint64_t* mask, uint32_t n_words, unsigned long long* count) {
    if (n_words == 0) return;
    hipLaunchKernelGGL(k_pair_count_bits, dim3(grid_for(n_words, 256)), dim3(256), 0, st, mask, n_words, count);
}
