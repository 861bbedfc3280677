// templates.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after pairs).
// Template-aware downsampling (qmcp_hip_solve_templates_*): the unit of selection is every segment that carries one
// template id.  Completion of the kept set S goes through a bitset of n_templates bits (flags, zeroed by the host):
//   k_tpl_check        err |= 1 when an id is >= n_templates (once per call)
//   k_tpl_sizes        sizes[id] += 1 per segment (once per call; sizes zeroed by the host)
//   k_tpl_size_hist    over the templates: the histogram of sizes 1 .. 7 and >= 8, the templates in use, the largest size
//   k_tpl_mark         flags |= the ids of the segments in S
//   k_tpl_spread       S = the segments whose template is flagged, and *count += |S|
// n <= 2^31 segments, so 64 * word + lane fits 32 bits.  tstat (unsigned long long): [0 .. 7] the histogram, [8] the
// templates in use, [9] the largest size.

__global__ __launch_bounds__(256) void k_tpl_check(const uint32_t* __restrict__ ids, uint32_t n, uint32_t n_templates,
                                                   uint32_t* __restrict__ err) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) bad |= ids[i] >= n_templates;
    if (__ballot(bad) != 0ull && (threadIdx.x & 63u) == 0) atomicOr(err, 1u);
}

// (ids checked by k_tpl_check; the bound is tested again so that a bad id never writes)
__global__ __launch_bounds__(256) void k_tpl_sizes(const uint32_t* __restrict__ ids, uint32_t n, uint32_t n_templates,
                                                   uint32_t* __restrict__ sizes) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t t = ids[i];
        if (t < n_templates) atomicAdd(&sizes[t], 1u);
    }
}

// a workgroup's ten counts in LDS, then one atomic per count that is not zero (a workgroup sees fewer than 2^32 templates)
__global__ __launch_bounds__(256) void k_tpl_size_hist(const uint32_t* __restrict__ sizes, uint32_t n_templates,
                                                       unsigned long long* __restrict__ tstat) {
    __shared__ uint32_t s_acc[10];
    if (threadIdx.x < 10) s_acc[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t largest = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_templates; t += stride) {
        const uint32_t sz = sizes[t];
        if (sz == 0) continue;
        atomicAdd(&s_acc[min(sz, 8u) - 1u], 1u);
        atomicAdd(&s_acc[8], 1u);
        largest = max(largest, sz);
    }
    if (largest) atomicMax(&s_acc[9], largest);
    __syncthreads();
    if (threadIdx.x < 9 && s_acc[threadIdx.x]) atomicAdd(&tstat[threadIdx.x], (unsigned long long)s_acc[threadIdx.x]);
    if (threadIdx.x == 9 && s_acc[9]) atomicMax(&tstat[9], (unsigned long long)s_acc[9]);
}

// one wave per word of S: the 64 ids coalesced, a no-return atomicOr per set bit
__global__ __launch_bounds__(256) void k_tpl_mark(const uint64_t* __restrict__ mask, const uint32_t* __restrict__ ids,
                                                  uint32_t n, uint32_t n_templates, uint32_t* __restrict__ flags) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_words = (uint32_t)(((uint64_t)n + 63u) / 64u);
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_words; w += waves) {
        const uint64_t word = mask[w];
        if (word == 0ull) continue;
        const uint32_t i = 64u * w + lane;
        if (i < n && ((word >> lane) & 1ull)) {
            const uint32_t t = ids[i];
            if (t < n_templates) atomicOr(&flags[t >> 5], 1u << (t & 31u));
        }
    }
}

// one wave per word: 64 ids, the gather of flags, a ballot, one store; bits at i >= n are never set
__global__ __launch_bounds__(256) void k_tpl_spread(const uint32_t* __restrict__ ids, uint32_t n, uint32_t n_templates,
                                                    const uint32_t* __restrict__ flags, uint64_t* __restrict__ mask,
                                                    unsigned long long* __restrict__ count) {
    __shared__ uint32_t s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_words = (uint32_t)(((uint64_t)n + 63u) / 64u);
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    uint32_t bits = 0;  // (a wave sees at most 2^25 words: no overflow)
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_words; w += waves) {
        const uint32_t i = 64u * w + lane;
        bool in = false;
        if (i < n) {
            const uint32_t t = ids[i];
            in = t < n_templates && ((flags[t >> 5] >> (t & 31u)) & 1u) != 0;
        }
        const uint64_t word = __ballot(in);
        if (lane == 0) {
            mask[w] = word;
            bits += (uint32_t)__popcll(word);
        }
    }
    if (lane == 0 && bits) atomicAdd(&s_sum, bits);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(count, (unsigned long long)s_sum);
}

void launch_tpl_check_sizes(hipStream_t st, const uint32_t* ids, uint32_t n, uint32_t n_templates, uint32_t* err,
                            uint32_t* sizes, unsigned long long* tstat) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_tpl_check, dim3(grid_for(n, 256)), dim3(256), 0, st, ids, n, n_templates, err);
    hipLaunchKernelGGL(k_tpl_sizes, dim3(grid_for(n, 256)), dim3(256), 0, st, ids, n, n_templates, sizes);
    hipLaunchKernelGGL(k_tpl_size_hist, dim3(grid_for(n_templates, 256)), dim3(256), 0, st, (const uint32_t*)sizes,
                       n_templates, tstat);
}

void launch_tpl_mark(hipStream_t st, const uint64_t* mask, const uint32_t* ids, uint32_t n, uint32_t n_templates,
                     uint32_t* flags) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_tpl_mark, dim3(grid_for(((uint64_t)n + 63) / 64, 4)), dim3(256), 0, st, mask, ids, n, n_templates,
                       flags);
}

void launch_tpl_spread(hipStream_t st, const uint32_t* ids, uint32_t n, uint32_t n_templates, const uint32_t* flags,
                       uint64_t* mask, unsigned long long* count) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_tpl_spread, dim3(grid_for(((uint64_t)n + 63) / 64, 4)), dim3(256), 0, st, ids, n, n_templates, flags,
                       mask, count);
}
