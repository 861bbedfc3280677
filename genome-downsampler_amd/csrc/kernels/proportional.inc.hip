// proportional.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after ceiling).
// Proportional downsampling (qmcp_hip_solve_proportional_*): the demand comes from the data's own depth,
//   q(p) = ceil(cov(p) * num / den),   need(p) = min(cov(p), max_coverage, max(q(p), floor)),
// swept by the profile's capped sweeps.
//   k_prop_need    profile_need_pass' shape without a table: need[p], the cut bit where need(p) == cov(p) (every read over
//                  p is kept), four counters and two maxima
//   k_prop_tally   once per call, over the columns in input order and the final mask: the placed reads, the sum of their
//                  spans, and the sum of the kept reads' spans
// Counters (unsigned long long each, the PropStat words of qmcp_kernels.h): reduced per wave, then one atomic per
// workgroup; the maxima by atomicMax.

// ceil(cov * num / den), exact for cov < 2^31, num <= den <= 2^20 (the product stays below 2^51).  The estimate is the
// product times 1 / den in double precision: the product is exact in 53 bits, 1 / den and the multiplication are each
// off by at most half an ulp, and the quotient is at most cov < 2^31, so the estimate lies within 2^-20 of the true
// quotient and its floor within one of the true floor.  One integer step either way settles it; the remainder says
// whether to round up.
__device__ __forceinline__ uint32_t prop_quota(uint32_t cov, uint32_t num, uint32_t den, double inv_den) {
    const unsigned long long prod = (unsigned long long)cov * num;
    uint32_t q = (uint32_t)((double)prod * inv_den);
    long long r = (long long)prod - (long long)((unsigned long long)q * den);
    if (r < 0) {
        --q;
        r += den;
    } else if (r >= (long long)den) {
        ++q;
        r -= den;
    }
    return q + (r != 0 ? 1u : 0u);
}

// A thread takes four consecutive positions at a time (16-byte loads of boff and eoff, one 16-byte store of need; the
// arrays are arena buffers, 256-byte aligned, and groups start at multiples of four); the last positions of the axis go
// one by one.
__global__ __launch_bounds__(256) void k_prop_need(const uint32_t* __restrict__ boff, const uint32_t* __restrict__ eoff,
                                                   uint32_t ltot, uint32_t num, uint32_t den, double inv_den,
                                                   uint32_t floor_depth, uint32_t max_cov, uint32_t* __restrict__ need,
                                                   unsigned long long* __restrict__ pst) {
    __shared__ unsigned long long s_acc[6];  // demand; whole, floor, capped positions; largest depth, largest need
    if (threadIdx.x < 6) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t n_groups = (ltot + 3u) / 4u;
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t whole_n = 0, floor_n = 0, capped_n = 0, deepest = 0, largest = 0;
    unsigned long long demand = 0;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += stride) {
        const uint32_t p0 = 4u * g;
        uint32_t cov[4];
        const bool whole = p0 + 3u < ltot;  // (then boff[p0 + 4] exists: boff has ltot + 1 entries)
        if (whole) {
            const uint4 b = *(const uint4*)(boff + p0), e = *(const uint4*)(eoff + p0);
            const uint32_t b4 = boff[p0 + 4];
            cov[0] = b.y - e.x; cov[1] = b.z - e.y; cov[2] = b.w - e.z; cov[3] = b4 - e.w;  // cov(p) = boff[p + 1] - eoff[p]
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) cov[r] = p0 + r < ltot ? boff[p0 + r + 1] - eoff[p0 + r] : 0u;
        }
        uint32_t out[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t cv = cov[r];
            const uint32_t q = prop_quota(cv, num, den, inv_den);
            const uint32_t top = min(cv, max_cov);
            const uint32_t nd = min(top, max(q, floor_depth));
            out[r] = nd | (nd == cv ? kNeedCutBit : 0u);
            if (p0 + (uint32_t)r < ltot) {
                demand += nd;
                whole_n += (cv != 0u && nd == cv) ? 1u : 0u;
                floor_n += q < min(floor_depth, top) ? 1u : 0u;
                capped_n += (max(q, floor_depth) > max_cov && cv > max_cov) ? 1u : 0u;
                deepest = max(deepest, cv);
                largest = max(largest, nd);
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
    demand = wave_sum_u48(demand);  // (a thread's sum stays far below 2^48)
    whole_n = wave_sum_u32(whole_n);
    floor_n = wave_sum_u32(floor_n);
    capped_n = wave_sum_u32(capped_n);
    deepest = wave_max_u32(deepest);
    largest = wave_max_u32(largest);
    if ((threadIdx.x & 63u) == 0) {
        if (demand) atomicAdd(&s_acc[0], demand);
        if (whole_n) atomicAdd(&s_acc[1], (unsigned long long)whole_n);
        if (floor_n) atomicAdd(&s_acc[2], (unsigned long long)floor_n);
        if (capped_n) atomicAdd(&s_acc[3], (unsigned long long)capped_n);
        if (deepest) atomicMax(&s_acc[4], (unsigned long long)deepest);
        if (largest) atomicMax(&s_acc[5], (unsigned long long)largest);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_acc[0]) atomicAdd(&pst[kPropDemand], s_acc[0]);
        if (s_acc[1]) atomicAdd(&pst[kPropWholePositions], s_acc[1]);
        if (s_acc[2]) atomicAdd(&pst[kPropFloorPositions], s_acc[2]);
        if (s_acc[3]) atomicAdd(&pst[kPropCappedPositions], s_acc[3]);
        if (s_acc[4]) atomicMax(&pst[kPropMaxDepth], s_acc[4]);
        if (s_acc[5]) atomicMax(&pst[kPropMaxNeed], s_acc[5]);
    }
}

// One read per thread and trip: a wave's 64 reads share one mask word.  Unplaced reads (and their coordinates, which
// nothing has checked) count nowhere.
__global__ __launch_bounds__(256) void k_prop_tally(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                    const uint32_t* __restrict__ ids, uint64_t n_reads,
                                                    const uint64_t* __restrict__ mask,
                                                    unsigned long long* __restrict__ pst) {
    __shared__ unsigned long long s_acc[3];  // placed reads, their bases, the kept reads' bases
    if (threadIdx.x < 3) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t placed_n = 0;  // (a thread counts at most 2^31 reads)
    unsigned long long bases_in = 0, bases_kept = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_reads; i += stride) {
        if (ids[i] == QMCP_NO_CONTIG) continue;
        const unsigned long long span = (unsigned long long)(ends[i] - starts[i]) + 1ull;
        ++placed_n;
        bases_in += span;
        if ((mask[i >> 6] >> (i & 63u)) & 1ull) bases_kept += span;
    }
    placed_n = wave_sum_u32(placed_n);
    bases_in = wave_sum_u48(bases_in);  // (at most 2^31 / 2^19 reads a thread, spans below 2^32: far below 2^48)
    bases_kept = wave_sum_u48(bases_kept);
    if ((threadIdx.x & 63u) == 0) {
        if (placed_n) atomicAdd(&s_acc[0], (unsigned long long)placed_n);
        if (bases_in) atomicAdd(&s_acc[1], bases_in);
        if (bases_kept) atomicAdd(&s_acc[2], bases_kept);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_acc[0]) atomicAdd(&pst[kPropPlaced], s_acc[0]);
        if (s_acc[1]) atomicAdd(&pst[kPropBasesIn], s_acc[1]);
        if (s_acc[2]) atomicAdd(&pst[kPropBasesKept], s_acc[2]);
    }
}

void launch_prop_need(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, uint32_t ltot, uint32_t num, uint32_t den,
                      uint32_t floor_depth, uint32_t max_coverage, uint32_t* need, unsigned long long* pst) {
    if (ltot == 0) return;
    const dim3 grid(grid_for(((uint64_t)ltot + 3) / 4, 256)), block(256);
    hipLaunchKernelGGL(k_prop_need, grid, block, 0, st, boff, eoff, ltot, num, den, 1.0 / (double)den, floor_depth,
                       max_coverage, need, pst);
}

void launch_prop_tally(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids, uint64_t n_reads,
                       const uint64_t* mask, unsigned long long* pst) {
    if (n_reads == 0) return;
    hipLaunchKernelGGL(k_prop_tally, dim3(grid_for(n_reads, 256)), dim3(256), 0, st, starts, ends, ids, n_reads, mask, pst);
}
