// budget.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after ceiling).
// Budget downsampling (qmcp_hip_solve_budget_*): the deepest coverage whose by-contig solve fits a number of reads.
//   k_budget_tally     per batch, over its per-position depth: a histogram of min(cov, H - 1), the largest depth and
//                      the sum of the depths, into accumulators that live across the batches of a call
//   k_budget_curve     once, one workgroup: S(M) = sum over positions of min(cov, M) for M = 0 .. H - 1, from the
//                      histogram's suffix counts #{p : cov(p) >= M} and their running sum
//   k_budget_finish    per probe, under QMCP_BUDGET_WHOLE_PAIRS: every aligned bit pair of the input-order mask ORed
//                      among the placed reads, and the popcount of the result
// Accumulators (unsigned long long each, the BudgetWord words of qmcp_kernels.h): reduced per wave, then per workgroup.

// LDS: one histogram of H u32 bins per workgroup (H <= 8192: 32 KiB).  A workgroup sees at most 2^31 / gridDim.x
// positions, so a bin fits 32 bits.  Deep data puts nearly every position into the clamped last bin: those lanes are
// counted once per wave by ballot and popcount, the other lanes take one LDS atomic each.  The loop runs whole waves
// (the ballot needs every lane), a lane past the end counts nothing.
__global__ __launch_bounds__(256) void k_budget_tally(const uint32_t* __restrict__ cov, uint32_t ltot, uint32_t H,
                                                      unsigned long long* __restrict__ acc,
                                                      unsigned long long* __restrict__ hist) {
    extern __shared__ uint32_t s_budget_hist[];
    __shared__ unsigned long long s_acc[2];  // max; sum
    for (uint32_t i = threadIdx.x; i < H; i += blockDim.x) s_budget_hist[i] = 0;
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, last = H - 1u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t largest = 0;
    unsigned long long sum = 0;  // (a thread sees at most 2^12 positions of less than 2^31 each)
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < ltot; base += stride) {
        const uint64_t p = base + threadIdx.x;
        const bool in = p < ltot;
        const uint32_t d = in ? cov[p] : 0u;
        const bool clamped = in && d >= last;
        const unsigned long long top_lanes = __ballot(clamped);
        if (in && !clamped) atomicAdd(&s_budget_hist[d], 1u);
        if (lane == 0 && top_lanes) atomicAdd(&s_budget_hist[last], (uint32_t)__popcll(top_lanes));
        largest = max(largest, d);
        sum += d;
    }
    largest = wave_max_u32(largest);
    sum = wave_sum_u48(sum);
    if (lane == 0) {
        if (largest) atomicMax(&s_acc[0], (unsigned long long)largest);
        if (sum) atomicAdd(&s_acc[1], sum);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < H; i += blockDim.x) {
        const uint32_t v = s_budget_hist[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
    if (threadIdx.x == 0) {
        if (s_acc[0]) atomicMax(&acc[kBudgetMaxDepth], s_acc[0]);
        if (s_acc[1]) atomicAdd(&acc[kBudgetTotalBases], s_acc[1]);
    }
}

// One workgroup of 256: thread t owns the bins [t * per, (t + 1) * per) in both scans, so curve[] doubles as the place
// of the suffix counts without another thread reading them; the 256 partial sums go through LDS and one thread.
// hist[H - 1] holds every position of depth H - 1 OR MORE, which is what the suffix count at H - 1 asks for.
__global__ __launch_bounds__(256) void k_budget_curve(const unsigned long long* __restrict__ hist, uint32_t H,
                                                      unsigned long long* __restrict__ curve) {
    __shared__ unsigned long long s_part[256];
    const uint32_t t = threadIdx.x, per = (H + 255u) / 256u;
    const uint32_t lo = min(t * per, H), hi = min(lo + per, H);
    unsigned long long run = 0;
    for (uint32_t i = lo; i < hi; ++i) run += hist[i];
    s_part[t] = run;
    __syncthreads();
    if (t == 0) {  // the bins behind each thread's own
        unsigned long long behind = 0;
        for (int k = 255; k >= 0; --k) {
            const unsigned long long v = s_part[k];
            s_part[k] = behind;
            behind += v;
        }
    }
    __syncthreads();
    run = s_part[t];
    unsigned long long total = 0;
    for (uint32_t i = hi; i-- > lo;) {
        run += hist[i];
        const unsigned long long at_least = i == 0 ? 0ull : run;  // #{p : cov(p) >= i}; S(0) = 0
        curve[i] = at_least;
        total += at_least;
    }
    __syncthreads();
    s_part[t] = total;
    __syncthreads();
    if (t == 0) {  // the bins before each thread's own
        unsigned long long before = 0;
        for (int k = 0; k < 256; ++k) {
            const unsigned long long v = s_part[k];
            s_part[k] = before;
            before += v;
        }
    }
    __syncthreads();
    run = s_part[t];
    for (uint32_t i = lo; i < hi; ++i) {
        run += curve[i];
        curve[i] = run;
    }
}

// k_ceiling_finish's walk over the mask words in input order (a wave takes 256 reads -- four words -- at a time, sixteen
// lanes OR their nibbles of placed bits into one word): a read is kept when it or its mate (reads 2q, 2q + 1; n_reads is
// even) is, and it is placed.
template <bool kVec>
__global__ __launch_bounds__(256) void k_budget_finish(const uint32_t* __restrict__ ids, uint64_t n_reads,
                                                       uint64_t* __restrict__ mask, unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long s_kept;
    if (threadIdx.x == 0) s_kept = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = (n_reads + 255u) / 256u;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    const uint64_t even = 0x5555555555555555ull;
    uint32_t kept_n = 0;  // (a lane counts at most 2^31 reads)
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
            const uint64_t k = mask[w];
            const uint64_t keep = (k | ((k & even) << 1) | ((k >> 1) & even)) & placed;
            mask[w] = keep;
            kept_n += (uint32_t)__popcll(keep);
        }
    }
    kept_n = wave_sum_u32(kept_n);
    if (lane == 0 && kept_n) atomicAdd(&s_kept, (unsigned long long)kept_n);
    __syncthreads();
    if (threadIdx.x == 0 && s_kept) atomicAdd(&acc[kBudgetKept], s_kept);
}

void launch_budget_tally(hipStream_t st, const uint32_t* cov, uint32_t ltot, uint32_t H, unsigned long long* acc,
                         unsigned long long* hist) {
    if (ltot == 0 || H == 0 || H > kBudgetBinsMax) return;
    hipLaunchKernelGGL(k_budget_tally, dim3(grid_for(ltot, 256)), dim3(256), (size_t)H * sizeof(uint32_t), st, cov, ltot, H,
                       acc, hist);
}

void launch_budget_curve(hipStream_t st, const unsigned long long* hist, uint32_t H, unsigned long long* curve) {
    if (H == 0) return;
    hipLaunchKernelGGL(k_budget_curve, dim3(1), dim3(256), 0, st, hist, H, curve);
}

void launch_budget_finish(hipStream_t st, const uint32_t* ids, uint64_t n_reads, uint64_t* mask, unsigned long long* acc) {
    if (n_reads == 0) return;
    const dim3 grid(grid_for((n_reads + 255) / 256, 4)), block(256);
    if (((uintptr_t)ids & 15u) == 0)
        hipLaunchKernelGGL(k_budget_finish<true>, grid, block, 0, st, ids, n_reads, mask, acc);
    else
        hipLaunchKernelGGL(k_budget_finish<false>, grid, block, 0, st, ids, n_reads, mask, acc);
}
