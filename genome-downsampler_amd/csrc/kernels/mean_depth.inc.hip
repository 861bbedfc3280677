// mean_depth.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after budget).
// Mean-depth downsampling (qmcp_hip_solve_mean_depth_*): the deepest coverage whose by-contig solve keeps at most a number
// of BASES inside a region set R (all positions without one).  k_budget_curve and k_budget_finish are shared with the
// budget entries; without a region table so is k_budget_tally.
//   k_md_tally      per batch with a region table: k_budget_tally's histogram and sum over the positions of R only, walked
//                   by their rank in R, and the largest depth over ALL positions of the batch
//   k_md_weights    once per call: w[i] = |read i n R| (the span without a table; 0 for an unplaced or off-target read)
//   k_md_count      per probe: the sum of w over the set bits of the input-order mask, and their number
// Accumulators are unsigned long long, reduced per wave, then per workgroup, then one atomic per workgroup.

constexpr uint32_t kMdLdsMax = kTargetLdsMax;  // merged regions whose bounds k_md_weights stages in LDS (32 KiB)

// R's positions inside one batch, by rank: merged region k of the batch starts at position rpos[k] of the batch's
// concatenated axis and holds the ranks [rcum[k], rcum[k + 1]) (rcum[n_reg] = n_pos is not stored).  A wave takes 64
// consecutive ranks: ONE search over the table for the region of its first rank (wave-uniform), then every lane looks
// among the at most `lane` regions that follow (a region holds a position at least): six steps, whatever the table's size.
// The histogram is k_budget_tally's: one LDS histogram per workgroup, the clamped last bin counted once per wave by ballot
// and popcount; the loop runs whole waves.  Then the one pass for the maximum: 16-byte loads of cov (an arena buffer), the
// last positions one by one.
__global__ __launch_bounds__(256) void k_md_tally(const uint32_t* __restrict__ cov, uint32_t ltot,
                                                  const uint32_t* __restrict__ rpos, const uint32_t* __restrict__ rcum,
                                                  uint32_t n_reg, uint32_t n_pos, uint32_t H,
                                                  unsigned long long* __restrict__ acc,
                                                  unsigned long long* __restrict__ hist) {
    extern __shared__ uint32_t s_md_hist[];
    __shared__ unsigned long long s_acc[2];  // max; sum
    for (uint32_t i = threadIdx.x; i < H; i += blockDim.x) s_md_hist[i] = 0;
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, last = H - 1u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long sum = 0;  // (a thread sees at most 2^12 positions of less than 2^31 each)
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n_pos; base += stride) {
        const uint64_t q0 = base + (threadIdx.x & ~63u);  // the wave's first rank
        uint32_t d = 0;
        bool in = false;
        if (q0 < n_pos) {  // (wave-uniform)
            uint32_t a = 0, b = n_reg - 1u;  // the last region with rcum <= q0 lies in [a, b]: rcum[0] == 0
            const uint32_t wq = __builtin_amdgcn_readfirstlane((uint32_t)q0);
            while (a < b) {
                const uint32_t m = a + ((b - a + 1u) >> 1);
                if (rcum[m] <= wq) a = m;
                else b = m - 1u;
            }
            const uint64_t q = q0 + lane;
            in = q < n_pos;
            if (in) {
                b = min(a + lane, n_reg - 1u);
                while (a < b) {
                    const uint32_t m = a + ((b - a + 1u) >> 1);
                    if (rcum[m] <= (uint32_t)q) a = m;
                    else b = m - 1u;
                }
                const uint32_t p = rpos[a] + ((uint32_t)q - rcum[a]);
                in = p < ltot;  // (the host clips every region to its contig: always)
                d = in ? cov[p] : 0u;
            }
        }
        const bool clamped = in && d >= last;
        const unsigned long long top_lanes = __ballot(clamped);
        if (in && !clamped) atomicAdd(&s_md_hist[d], 1u);
        if (lane == 0 && top_lanes) atomicAdd(&s_md_hist[last], (uint32_t)__popcll(top_lanes));
        sum += d;
    }
    uint32_t largest = 0;
    const uint32_t quads = ltot >> 2;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < quads; i += stride) {
        const uint4 v = ((const uint4*)cov)[i];
        largest = max(max(largest, max(v.x, v.y)), max(v.z, v.w));
    }
    if (blockIdx.x == 0 && threadIdx.x < (ltot & 3u)) largest = max(largest, cov[4u * quads + threadIdx.x]);
    largest = wave_max_u32(largest);
    sum = wave_sum_u48(sum);
    if (lane == 0) {
        if (largest) atomicMax(&s_acc[0], (unsigned long long)largest);
        if (sum) atomicAdd(&s_acc[1], sum);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < H; i += blockDim.x) {
        const uint32_t v = s_md_hist[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
    if (threadIdx.x == 0) {
        if (s_acc[0]) atomicMax(&acc[kBudgetMaxDepth], s_acc[0]);
        if (s_acc[1]) atomicAdd(&acc[kBudgetTotalBases], s_acc[1]);
    }
}

// one read's weight.  kTab 0: no table, the span.  The reads were validated by the grouping before this runs; a read it
// would have refused weighs nothing here.
template <int kTab>
__device__ __forceinline__ uint32_t md_weight_one(uint32_t s, uint32_t e, uint32_t id, uint32_t n_contigs,
                                                  const uint32_t* __restrict__ offs, const uint32_t* rs, const uint32_t* re,
                                                  const uint32_t* __restrict__ cum) {
    if (id >= n_contigs || s > e) return 0u;
    if constexpr (kTab == 0) {
        return e - s + 1u;
    } else {
        uint32_t cs, ce;
        return project_read(rs, re, cum, offs[id], offs[id + 1], s, e, &cs, &ce) ? ce - cs + 1u : 0u;
    }
}

// kTab: 0 no table, 1 the regions' bounds in LDS (at most kMdLdsMax merged regions), 2 read from global memory, as
// k_target_project.  kVec: the three columns are 16-byte aligned -- a thread takes four consecutive reads with one 128-bit
// load of each column and one 128-bit store of w (an arena buffer); otherwise a thread takes one read at a time.
template <int kTab, bool kVec>
__global__ __launch_bounds__(256) void k_md_weights(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                    const uint32_t* __restrict__ ids, uint32_t n, uint32_t n_contigs,
                                                    const uint32_t* __restrict__ offs, const uint32_t* __restrict__ g_rs,
                                                    const uint32_t* __restrict__ g_re, const uint32_t* __restrict__ cum,
                                                    uint32_t n_regions, uint32_t* __restrict__ w) {
    extern __shared__ uint32_t s_md_tab[];  // kTab == 1: [n_regions starts | n_regions ends]
    const uint32_t* rs = g_rs;
    const uint32_t* re = g_re;
    if constexpr (kTab == 1) {
        for (uint32_t i = threadIdx.x; i < n_regions; i += blockDim.x) {
            s_md_tab[i] = g_rs[i];
            s_md_tab[n_regions + i] = g_re[i];
        }
        __syncthreads();
        rs = s_md_tab;
        re = s_md_tab + n_regions;
    }
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (kVec) {
        const uint64_t groups = ((uint64_t)n + 3u) / 4u;
        for (uint64_t g = t; g < groups; g += stride) {
            const uint64_t i0 = 4u * g;
            if (i0 + 3u < n) {
                const uint4 s = *(const uint4*)(starts + i0), e = *(const uint4*)(ends + i0), d = *(const uint4*)(ids + i0);
                *(uint4*)(w + i0) = make_uint4(md_weight_one<kTab>(s.x, e.x, d.x, n_contigs, offs, rs, re, cum),
                                               md_weight_one<kTab>(s.y, e.y, d.y, n_contigs, offs, rs, re, cum),
                                               md_weight_one<kTab>(s.z, e.z, d.z, n_contigs, offs, rs, re, cum),
                                               md_weight_one<kTab>(s.w, e.w, d.w, n_contigs, offs, rs, re, cum));
            } else {
                for (uint64_t i = i0; i < n; ++i)
                    w[i] = md_weight_one<kTab>(starts[i], ends[i], ids[i], n_contigs, offs, rs, re, cum);
            }
        }
    } else {
        for (uint64_t i = t; i < n; i += stride)
            w[i] = md_weight_one<kTab>(starts[i], ends[i], ids[i], n_contigs, offs, rs, re, cum);
    }
}

// A wave takes 64 consecutive mask words at a time, one per lane (one coalesced 512-byte load), and then, for each of
// them that is not zero (a ballot names them), the 64 weights of its reads: lane l loads w[64 word + l] when bit l is set.
// Sparse masks -- a deep input kept at a few per cent has many empty words -- load no weight for those.
__global__ __launch_bounds__(256) void k_md_count(const uint64_t* __restrict__ mask, uint64_t n_words,
                                                  const uint32_t* __restrict__ w, uint64_t n_reads,
                                                  unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long s_acc[2];  // bases; reads
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = (n_words + 63u) / 64u;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    unsigned long long bases = 0;  // (a lane adds at most 2^12 weights of less than 2^32 each)
    uint32_t kept = 0;
    for (uint64_t ch = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); ch < n_chunks; ch += waves) {
        const uint64_t wi = 64u * ch + lane;
        const unsigned long long word = wi < n_words ? mask[wi] : 0ull;
        kept += (uint32_t)__popcll(word);
        unsigned long long live = __ballot(word != 0);
        while (live) {  // (wave-uniform)
            const int j = __ffsll(live) - 1;
            live &= live - 1ull;
            const unsigned long long wj = (unsigned long long)__shfl((long long)word, j, kWave);
            const uint64_t i = 64u * (64u * ch + (uint32_t)j) + lane;
            if (((wj >> lane) & 1ull) && i < n_reads) bases += w[i];
        }
    }
    bases = wave_sum_u48(bases);
    kept = wave_sum_u32(kept);
    if (lane == 0) {
        if (bases) atomicAdd(&s_acc[0], bases);
        if (kept) atomicAdd(&s_acc[1], (unsigned long long)kept);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_acc[0]) atomicAdd(&acc[kMdBases], s_acc[0]);
        if (s_acc[1]) atomicAdd(&acc[kMdKept], s_acc[1]);
    }
}

void launch_md_tally(hipStream_t st, const uint32_t* cov, uint32_t ltot, const uint32_t* rpos, const uint32_t* rcum,
                     uint32_t n_reg, uint32_t n_pos, uint32_t H, unsigned long long* acc, unsigned long long* hist) {
    if (ltot == 0 || H == 0 || H > kBudgetBinsMax) return;
    if (n_reg == 0) n_pos = 0;
    const uint64_t work = std::max<uint64_t>(n_pos, ltot / 4u);
    hipLaunchKernelGGL(k_md_tally, dim3(grid_for(work, 256)), dim3(256), (size_t)H * sizeof(uint32_t), st, cov, ltot, rpos,
                       rcum, n_reg, n_pos, H, acc, hist);
}

void launch_md_weights(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids, uint32_t n,
                       uint32_t n_contigs, bool has_table, const uint32_t* offs, const uint32_t* rs, const uint32_t* re,
                       const uint32_t* cum, uint32_t n_regions, uint32_t* w) {
    if (n == 0) return;
    const bool vec = (((uintptr_t)starts | (uintptr_t)ends | (uintptr_t)ids) & 15u) == 0;
    const dim3 grid(grid_for(vec ? ((uint64_t)n + 3) / 4 : n, 256)), block(256);
    const bool lds = n_regions <= kMdLdsMax;
    const size_t shm = has_table && lds ? 2 * (size_t)n_regions * sizeof(uint32_t) : 0;
#define QMCP_MDW(TAB, VEC)                                                                                              \
    hipLaunchKernelGGL((k_md_weights<TAB, VEC>), grid, block, shm, st, starts, ends, ids, n, n_contigs, offs, rs, re, cum, \
                       n_regions, w)
    if (!has_table) {
        if (vec) QMCP_MDW(0, true);
        else QMCP_MDW(0, false);
    } else if (lds) {
        if (vec) QMCP_MDW(1, true);
        else QMCP_MDW(1, false);
    } else {
        if (vec) QMCP_MDW(2, true);
        else QMCP_MDW(2, false);
    }
#undef QMCP_MDW
}

void launch_md_count(hipStream_t st, const uint64_t* mask, const uint32_t* w, uint64_t n_reads, unsigned long long* acc) {
    if (n_reads == 0) return;
    const uint64_t n_words = (n_reads + 63) / 64;
    hipLaunchKernelGGL(k_md_count, dim3(grid_for((n_words + 63) / 64, 4)), dim3(256), 0, st, mask, n_words, w, n_reads,
                       acc);
}
