// templates_profile.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after
// templates).
// Template-aware downsampling under a cap table (qmcp_hip_solve_templates_profile_*): the staged solve of templates.inc.hip
// with a cap per region in the place of the one target.
//   k_tpl_profile_need   k_profile_need and k_pair_need in one: need[p] = min(cov_rest(p), max(0, cap(p) - credit[p])) over
//                        the candidates' boff / eoff, the stage's caps (scaled by the host) looked up in the batch's region
//                        table, the cut bit, and the two counters
//   k_tpl_on_cap         once per call, per placed segment: does it cover a position whose cap is positive?  The template's
//                        bit goes into a bitset of its own, the segments are counted

// profile_need_pass (kernels/profile.inc.hip) with the credit: the stage's caps arrive scaled, the kernel only does
// cap > credit ? cap - credit : 0 and a min.  kLds as in k_profile_need.
template <bool kLds>
__global__ __launch_bounds__(256) void k_tpl_profile_need(const uint32_t* __restrict__ boff, const uint32_t* __restrict__ eoff,
                                                          const uint32_t* __restrict__ credit, uint32_t ltot,
                                                          const uint32_t* __restrict__ g_rs, const uint32_t* __restrict__ g_re,
                                                          const uint32_t* __restrict__ g_cap, uint32_t n_regions,
                                                          uint32_t default_cap, uint32_t* __restrict__ need,
                                                          unsigned long long* __restrict__ pstat) {
    profile_need_pass<kLds, true>(boff, eoff, credit, ltot, g_rs, g_re, g_cap, n_regions, default_cap, need, pstat);
}

// F(x): the positions p < x of one contig with cap(p) > 0.  The contig owns regions [a, b) of the call's table, ascending
// and disjoint; before[k] = F(rs[k]) comes from the host (cap_table.h).  One binary search for the last region that
// begins below x; x itself indexes nothing.
__device__ __forceinline__ uint32_t tpl_positive_before(const uint32_t* __restrict__ rs, const uint32_t* __restrict__ re,
                                                        const uint32_t* __restrict__ cap, const uint32_t* __restrict__ before,
                                                        uint32_t a, uint32_t b, bool default_positive, uint32_t x) {
    uint32_t lo = a, hi = b;
    while (lo < hi) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (rs[m] < x) lo = m + 1;
        else hi = m;
    }
    if (lo == a) return default_positive ? x : 0u;
    const uint32_t j = lo - 1u;
    const uint32_t behind = re[j] + 1u;  // (re < the contig's length < 2^31)
    uint32_t f = before[j];
    if (cap[j] != 0u) f += min(x, behind) - rs[j];
    if (default_positive && x > behind) f += x - behind;
    return f;
}

// per segment in input order: placed (contig id < n_contigs) and F(end + 1) - F(start) > 0 sets the template's bit with a
// no-return atomicOr and counts.  An id >= n_templates never writes.  The count is reduced per wave, one atomic per
// workgroup.
__global__ __launch_bounds__(256) void k_tpl_on_cap(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                    const uint32_t* __restrict__ contig_ids, const uint32_t* __restrict__ tids,
                                                    uint32_t n, uint32_t n_contigs, uint32_t n_templates,
                                                    const uint32_t* __restrict__ roffs, const uint32_t* __restrict__ rs,
                                                    const uint32_t* __restrict__ re, const uint32_t* __restrict__ cap,
                                                    const uint32_t* __restrict__ before, uint32_t default_positive,
                                                    uint32_t* __restrict__ flags, unsigned long long* __restrict__ count) {
    __shared__ uint32_t s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    uint32_t mine = 0;  // (a thread sees at most 2^31 / 2^19 segments: no overflow)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t c = contig_ids[i];
        if (c >= n_contigs) continue;  // unplaced
        const uint32_t s = starts[i], e = ends[i];
        if (e < s || e == 0xFFFFFFFFu) continue;  // (the solve refused such a segment before this pass)
        const uint32_t a = roffs[c], b = roffs[c + 1];
        const uint32_t f1 = tpl_positive_before(rs, re, cap, before, a, b, default_positive != 0u, e + 1u);
        const uint32_t f0 = tpl_positive_before(rs, re, cap, before, a, b, default_positive != 0u, s);
        if (f1 != f0) {
            ++mine;
            const uint32_t t = tids[i];
            if (t < n_templates) atomicOr(&flags[t >> 5], 1u << (t & 31u));
        }
    }
    mine = wave_sum_u32(mine);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(count, (unsigned long long)s_sum);
}

void launch_tpl_profile_need(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, const uint32_t* credit, uint32_t ltot,
                             const uint32_t* rs, const uint32_t* re, const uint32_t* cap, uint32_t n_regions,
                             uint32_t default_cap, uint32_t* need, unsigned long long* pstat) {
    if (ltot == 0) return;
    const dim3 grid(grid_for(((uint64_t)ltot + 3) / 4, 256)), block(256);
    if (n_regions <= kProfileLdsMax)
        hipLaunchKernelGGL(k_tpl_profile_need<true>, grid, block, 3 * (size_t)n_regions * sizeof(uint32_t), st, boff, eoff,
                           credit, ltot, rs, re, cap, n_regions, default_cap, need, pstat);
    else
        hipLaunchKernelGGL(k_tpl_profile_need<false>, grid, block, 0, st, boff, eoff, credit, ltot, rs, re, cap, n_regions,
                           default_cap, need, pstat);
}

void launch_tpl_on_cap(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                       const uint32_t* tids, uint32_t n, uint32_t n_contigs, uint32_t n_templates, const uint32_t* roffs,
                       const uint32_t* rs, const uint32_t* re, const uint32_t* cap, const uint32_t* before,
                       bool default_positive, uint32_t* flags, unsigned long long* count) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_tpl_on_cap, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, ends, contig_ids, tids, n, n_contigs,
                       n_templates, roffs, rs, re, cap, before, default_positive ? 1u : 0u, flags, count);
}
