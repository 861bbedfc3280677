// thresholds.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after budget).
// Coverage thresholds (qmcp_hip_solve_thresholds_*): every read's smallest coverage in lo .. hi whose by-contig solve keeps
// it.  The thresholds array is filled with kThresholdNever BEFORE the first step (one memset by the host), so:
//   k_thresholds_step     per coverage M: the reads of keep_M without a threshold get M, the reads with one that keep_M
//                         drops are counted (thresholds_plan.h: thresholds_word), seen |= keep_M
//   k_thresholds_finish   once: under QMCP_THRESHOLDS_WHOLE_PAIRS the pair minimum among placed mates, then the histogram
//                         of the final thresholds over the bins lo .. top
//   k_thresholds_counts   once, one workgroup: the histogram's running sum in place -- the reads with threshold <= M
// Accumulators (unsigned long long each, the ThresholdsAccWord words of qmcp_kernels.h): reduced per wave, then per workgroup.

// A lane takes one word of the mask and of seen: 3 n / 8 bytes a step (two loads, one store where seen changes) plus one
// 16-bit store per fresh read -- over a whole call every read is stored at most once.  The mask holds no bit at or
// beyond n_reads (the grouping clears it, the scatter ORs real reads); the tail word is cut all the same, so that no
// store can leave the array.
__global__ __launch_bounds__(256) void k_thresholds_step(const uint64_t* __restrict__ mask, uint64_t* __restrict__ seen,
                                                         uint64_t n_reads, uint32_t M, uint16_t* __restrict__ thr,
                                                         unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long s_acc[2];  // fresh; lost
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t words = (n_reads + 63u) / 64u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t fresh_n = 0, lost_n = 0;  // (a lane sees at most 2^31 reads)
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += stride) {
        uint64_t m = mask[w];
        const uint64_t left = n_reads - 64u * w;
        if (left < 64u) m &= (1ull << left) - 1ull;
        const uint64_t s = seen[w];
        const ThresholdsWord t = thresholds_word(m, s);
        if (t.seen != s) seen[w] = t.seen;
        uint64_t f = t.fresh;
        while (f) {
            const uint32_t bit = (uint32_t)__ffsll((unsigned long long)f) - 1u;
            thr[64u * w + bit] = (uint16_t)M;
            f &= f - 1ull;
        }
        fresh_n += (uint32_t)__popcll(t.fresh);
        lost_n += (uint32_t)__popcll(t.lost);
    }
    fresh_n = wave_sum_u32(fresh_n);
    lost_n = wave_sum_u32(lost_n);
    if ((threadIdx.x & 63u) == 0) {
        if (fresh_n) atomicAdd(&s_acc[0], (unsigned long long)fresh_n);
        if (lost_n) atomicAdd(&s_acc[1], (unsigned long long)lost_n);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_acc[0]) atomicAdd(&acc[kThSeen], s_acc[0]);
        if (s_acc[1]) atomicAdd(&acc[kThViolations], s_acc[1]);
    }
}

// A lane takes four reads -- two pairs -- at a time: one 8-byte load of thresholds, under the flag one 16-byte load of
// contig ids (placed-ness, as in k_budget_finish) and one 8-byte store where a mate's threshold is the smaller.  Bin
// t - lo of the histogram counts the reads with final threshold t; kThresholdNever has no bin.  kLds: one histogram of
// n_bins u32 per workgroup in LDS (n_bins <= kThresholdsBinsMax: 32 KiB; a workgroup sees at most 2^31 reads), flushed
// to the non-empty global bins; otherwise every read with a threshold takes one global atomic.
template <bool kPairs, bool kVec, bool kLds>
__global__ __launch_bounds__(256) void k_thresholds_finish(const uint32_t* __restrict__ ids, uint64_t n_reads, uint32_t lo,
                                                           uint32_t n_bins, uint16_t* __restrict__ thr,
                                                           unsigned long long* __restrict__ hist) {
    extern __shared__ uint32_t s_thresholds_hist[];
    if (kLds) {
        for (uint32_t i = threadIdx.x; i < n_bins; i += blockDim.x) s_thresholds_hist[i] = 0;
        __syncthreads();
    }
    const uint64_t quads = (n_reads + 3u) / 4u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
        const uint64_t i0 = 4u * q;
        const uint32_t have = (uint32_t)(n_reads - i0 < 4u ? n_reads - i0 : 4u);
        uint32_t t[4] = {kThresholdNever, kThresholdNever, kThresholdNever, kThresholdNever};
        if (kVec && have == 4u) {
            const uint2 v = *(const uint2*)(thr + i0);
            t[0] = v.x & 0xFFFFu; t[1] = v.x >> 16; t[2] = v.y & 0xFFFFu; t[3] = v.y >> 16;
        } else {
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r)
                if (r < have) t[r] = thr[i0 + r];
        }
        if (kPairs) {  // (n_reads is even: a pair never straddles the end)
            uint32_t id[4] = {QMCP_NO_CONTIG, QMCP_NO_CONTIG, QMCP_NO_CONTIG, QMCP_NO_CONTIG};
            if (kVec && have == 4u) {
                const uint4 v = *(const uint4*)(ids + i0);
                id[0] = v.x; id[1] = v.y; id[2] = v.z; id[3] = v.w;
            } else {
#pragma unroll
                for (uint32_t r = 0; r < 4; ++r)
                    if (r < have) id[r] = ids[i0 + r];
            }
            uint32_t u[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                u[r] = thresholds_pair(t[r], t[r ^ 1], id[r] != QMCP_NO_CONTIG, id[r ^ 1] != QMCP_NO_CONTIG);
            const bool changed = u[0] != t[0] || u[1] != t[1] || u[2] != t[2] || u[3] != t[3];
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = u[r];
            if (changed) {
                if (kVec && have == 4u) {
                    *(uint2*)(thr + i0) = make_uint2(t[0] | (t[1] << 16), t[2] | (t[3] << 16));
                } else {
#pragma unroll
                    for (uint32_t r = 0; r < 4; ++r)
                        if (r < have) thr[i0 + r] = (uint16_t)t[r];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t bin = t[r] - lo;  // (kThresholdNever - lo >= n_bins: hi <= 65534; a threshold is never below lo)
            if (t[r] != kThresholdNever && bin < n_bins) {
                if (kLds) atomicAdd(&s_thresholds_hist[bin], 1u);
                else atomicAdd(&hist[bin], 1ull);
            }
        }
    }
    if (kLds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_bins; i += blockDim.x) {
            const uint32_t v = s_thresholds_hist[i];
            if (v) atomicAdd(&hist[i], (unsigned long long)v);
        }
    }
}

// One workgroup of 256: thread t owns the bins [t * per, (t + 1) * per); the 256 partial sums go through LDS and one
// thread, as in k_budget_curve.  In place: counts[b] = hist[0] + ... + hist[b].
__global__ __launch_bounds__(256) void k_thresholds_counts(unsigned long long* __restrict__ counts, uint32_t n_bins) {
    __shared__ unsigned long long s_part[256];
    const uint32_t t = threadIdx.x, per = (n_bins + 255u) / 256u;
    const uint32_t lo = min(t * per, n_bins), hi = min(lo + per, n_bins);
    unsigned long long run = 0;
    for (uint32_t i = lo; i < hi; ++i) run += counts[i];
    s_part[t] = run;
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
        run += counts[i];
        counts[i] = run;
    }
}

void launch_thresholds_step(hipStream_t st, const uint64_t* mask, uint64_t* seen, uint64_t n_reads, uint32_t M,
                            uint16_t* thr, unsigned long long* acc) {
    if (n_reads == 0) return;
    hipLaunchKernelGGL(k_thresholds_step, dim3(grid_for((n_reads + 63) / 64, 256)), dim3(256), 0, st, mask, seen, n_reads, M,
                       thr, acc);
}

template <bool kPairs, bool kVec>
static void launch_thresholds_finish_as(hipStream_t st, const uint32_t* ids, uint64_t n_reads, uint32_t lo, uint32_t n_bins,
                                        uint16_t* thr, unsigned long long* hist) {
    const dim3 grid(grid_for((n_reads + 3) / 4, 256)), block(256);
    if (n_bins <= kThresholdsBinsMax)
        hipLaunchKernelGGL((k_thresholds_finish<kPairs, kVec, true>), grid, block, (size_t)n_bins * sizeof(uint32_t), st, ids,
                           n_reads, lo, n_bins, thr, hist);
    else
        hipLaunchKernelGGL((k_thresholds_finish<kPairs, kVec, false>), grid, block, 0, st, ids, n_reads, lo, n_bins, thr, hist);
}

void launch_thresholds_finish(hipStream_t st, const uint32_t* ids, uint64_t n_reads, bool whole_pairs, uint32_t lo,
                              uint32_t n_bins, uint16_t* thr, unsigned long long* hist) {
    if (n_reads == 0 || n_bins == 0) return;
    const bool vec = (((uintptr_t)thr & 7u) | ((uintptr_t)ids & 15u)) == 0;
    if (whole_pairs) {
        if (vec) launch_thresholds_finish_as<true, true>(st, ids, n_reads, lo, n_bins, thr, hist);
        else launch_thresholds_finish_as<true, false>(st, ids, n_reads, lo, n_bins, thr, hist);
    } else {
        if (vec) launch_thresholds_finish_as<false, true>(st, ids, n_reads, lo, n_bins, thr, hist);
        else launch_thresholds_finish_as<false, false>(st, ids, n_reads, lo, n_bins, thr, hist);
    }
}

void launch_thresholds_counts(hipStream_t st, unsigned long long* counts, uint32_t n_bins) {
    if (n_bins == 0) return;
    hipLaunchKernelGGL(k_thresholds_counts, dim3(1), dim3(256), 0, st, counts, n_bins);
}
