// profile.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after launchers).
// Coverage profile (qmcp_hip_solve_profile_*): the cap varies along the position axis, need(p) = min(cov(p), cap(p)).
//   k_profile_need   one pass over a batch's positions once boff / eoff exist: need[p], its top bit set where
//                    cov(p) <= cap(p) (a cut position: every read over p is kept), and the call's two counters
//   k_profile_cuts   k_find_cuts' window scan reading that bit instead of comparing with M; the same cut[] array, so
//                    k_build_segments and the stretch tables are reused as they are
// The capped forms of the mixed-span sweeps (kernels/sweep_mixed.inc.hip, kCapped) read need[] where the scalar
// forms compute min(cov, M); launch_sweep_general and launch_sweep_general_reg launch both (SweepDemand).

constexpr uint32_t kProfileLdsMax = 4096;  // regions staged in LDS (3 x 4 096 words = 48 KiB); above that they stay in L2
constexpr uint32_t kNeedCutBit = 0x80000000u;

// cap of position p: regions [rs[k], re[k]] ascending and disjoint; k = the first region with re >= p (the caller's
// cursor: found by binary search for a thread's first position, walked forward after that)
__device__ __forceinline__ uint32_t profile_first_region(const uint32_t* re, uint32_t n_regions, uint32_t p) {
    uint32_t a = 0, b = n_regions;
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (re[m] < p) a = m + 1;
        else b = m;
    }
    return a;
}

// The one pass behind k_profile_need and k_tpl_profile_need (kernels/templates_profile.inc.hip).
// kLds: the table in LDS ([rs | re | cap], n_regions each), else read from global memory.  kCredit: the cap of a
// position is what its region (or default_cap) leaves above credit[p] -- max(0, cap - credit[p]) -- and cov is the
// candidates' coverage; without it credit is not read.
// A thread takes four consecutive positions at a time (16-byte loads of boff, eoff and, with kCredit, credit, one 16-byte
// store of need; the arrays are arena buffers, 256-byte aligned -- credit from its 16-byte aligned entry on -- and groups
// start at multiples of four); the last positions of the axis go one by one.  pstat: [0] positions with cov > cap,
// [1] the sum of need -- one atomic each per workgroup.
template <bool kLds, bool kCredit>
__device__ __forceinline__ void profile_need_pass(const uint32_t* __restrict__ boff, const uint32_t* __restrict__ eoff,
                                                  const uint32_t* __restrict__ credit, uint32_t ltot,
                                                  const uint32_t* __restrict__ g_rs, const uint32_t* __restrict__ g_re,
                                                  const uint32_t* __restrict__ g_cap, uint32_t n_regions,
                                                  uint32_t default_cap, uint32_t* __restrict__ need,
                                                  unsigned long long* __restrict__ pstat) {
    extern __shared__ uint32_t s_cap_tab[];
    __shared__ unsigned long long s_acc[2];
    const uint32_t* rs = g_rs;
    const uint32_t* re = g_re;
    const uint32_t* cp = g_cap;
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
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
    uint32_t capped = 0;
    unsigned long long demand = 0;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += stride) {
        const uint32_t p0 = 4u * g;
        uint32_t cov[4], cr[4] = {0u, 0u, 0u, 0u};
        const bool whole = p0 + 3u < ltot;  // (then boff[p0 + 4] exists: boff has ltot + 1 entries)
        if (whole) {
            const uint4 b = *(const uint4*)(boff + p0), e = *(const uint4*)(eoff + p0);
            const uint32_t b4 = boff[p0 + 4];
            cov[0] = b.y - e.x; cov[1] = b.z - e.y; cov[2] = b.w - e.z; cov[3] = b4 - e.w;  // cov(p) = boff[p + 1] - eoff[p]
            if constexpr (kCredit) {
                const uint4 c = *(const uint4*)(credit + p0);
                cr[0] = c.x; cr[1] = c.y; cr[2] = c.z; cr[3] = c.w;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool in = p0 + r < ltot;
                cov[r] = in ? boff[p0 + r + 1] - eoff[p0 + r] : 0u;
                if constexpr (kCredit) cr[r] = in ? credit[p0 + r] : 0u;
            }
        }
        uint32_t k = profile_first_region(re, n_regions, p0);
        uint32_t out[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t p = p0 + (uint32_t)r;
            while (k < n_regions && re[k] < p) ++k;
            uint32_t cap = (k < n_regions && rs[k] <= p) ? cp[k] : default_cap;
            if constexpr (kCredit) cap = cap > cr[r] ? cap - cr[r] : 0u;
            const uint32_t nd = min(cov[r], cap);
            out[r] = nd | (cov[r] <= cap ? kNeedCutBit : 0u);
            if (p < ltot) {
                capped += cov[r] > cap ? 1u : 0u;
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
    const uint32_t d_lo = wave_sum_u32((uint32_t)(demand & 0xFFFFu)), d_mid = wave_sum_u32((uint32_t)((demand >> 16) & 0xFFFFu));
    const uint32_t d_hi = wave_sum_u32((uint32_t)(demand >> 32));  // (a thread's sum stays far below 2^48: 64 lanes of 16 bits fit)
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(&s_acc[0], (unsigned long long)capped);
        atomicAdd(&s_acc[1], (unsigned long long)d_lo + ((unsigned long long)d_mid << 16) + ((unsigned long long)d_hi << 32));
    }
    __syncthreads();
    if (threadIdx.x == 0 && (s_acc[0] | s_acc[1]) != 0) {
        if (s_acc[0]) atomicAdd(&pstat[0], s_acc[0]);
        if (!kCredit || s_acc[1]) atomicAdd(&pstat[1], s_acc[1]);
    }
}

template <bool kLds>
__global__ __launch_bounds__(256) void k_profile_need(const uint32_t* __restrict__ boff, const uint32_t* __restrict__ eoff,
                                                      uint32_t ltot, const uint32_t* __restrict__ g_rs,
                                                      const uint32_t* __restrict__ g_re, const uint32_t* __restrict__ g_cap,
                                                      uint32_t n_regions, uint32_t default_cap, uint32_t* __restrict__ need,
                                                      unsigned long long* __restrict__ pstat) {
    profile_need_pass<kLds, false>(boff, eoff, nullptr, ltot, g_rs, g_re, g_cap, n_regions, default_cap, need, pstat);
}

// k_find_cuts with the profile's own rule: window w reports the first position q in it at which a stretch may start --
// need[q - 1] carries the cut bit (cov(q - 1) <= cap(q - 1)) and q is no contig's first position.
__global__ __launch_bounds__(256) void k_profile_cuts(const uint32_t* __restrict__ need,
                                                      const uint64_t* __restrict__ contig_pos_off, uint32_t n_contigs,
                                                      uint32_t ltot, uint32_t win, uint32_t* __restrict__ cut) {
    __shared__ uint32_t s_first;
    __shared__ uint32_t s_cstart[256];  // contig starts (fewer than 256 contigs when this runs)
    const uint32_t w = blockIdx.x;
    const uint32_t lo = max(w * win, 1u);
    const uint32_t hi = (uint32_t)min((uint64_t)(w + 1) * win, (uint64_t)ltot);
    if (threadIdx.x == 0) s_first = kNoCut;
    if (threadIdx.x < n_contigs) s_cstart[threadIdx.x] = (uint32_t)contig_pos_off[threadIdx.x];
    __syncthreads();
    for (uint32_t q0 = lo; q0 < hi; q0 += 16 * blockDim.x) {
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t q = q0 + k * blockDim.x + threadIdx.x;
            if (q < hi && (need[q - 1] & kNeedCutBit) != 0) {
                bool contig_start = false;
                for (uint32_t c = 0; c < n_contigs; ++c) contig_start |= s_cstart[c] == q;
                if (!contig_start) atomicMin(&s_first, q);
            }
        }
        __syncthreads();
        if (s_first != kNoCut) break;  // uniform: read after the barrier
        __syncthreads();
    }
    if (threadIdx.x == 0) cut[w] = s_first;
}

void launch_profile_need(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, uint32_t ltot, const uint32_t* rs,
                         const uint32_t* re, const uint32_t* cap, uint32_t n_regions, uint32_t default_cap, uint32_t* need,
                         unsigned long long* pstat) {
    if (ltot == 0) return;
    const dim3 grid(grid_for(((uint64_t)ltot + 3) / 4, 256)), block(256);
    if (n_regions <= kProfileLdsMax)
        hipLaunchKernelGGL(k_profile_need<true>, grid, block, 3 * (size_t)n_regions * sizeof(uint32_t), st, boff, eoff, ltot,
                           rs, re, cap, n_regions, default_cap, need, pstat);
    else
        hipLaunchKernelGGL(k_profile_need<false>, grid, block, 0, st, boff, eoff, ltot, rs, re, cap, n_regions,
                           default_cap, need, pstat);
}

// launch_sweep_segments for a profile: fills seg_words ([windows' cuts | count, stretches]) from need's cut bits
SweepAxis launch_profile_segments(const SweepAxis& ax, const uint32_t* need, uint32_t n_windows, uint32_t* seg_words) {
    const uint32_t win = (ax.ltot + n_windows - 1) / n_windows;
    hipLaunchKernelGGL(k_profile_cuts, dim3(n_windows), dim3(256), 0, ax.st, need, ax.poff, ax.n_contigs, ax.ltot, win,
                       seg_words);
    return with_exact_segments(ax, n_windows, seg_words);
}
