// by_contig.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after launchers).
// Reads in any order with a contig id each (qmcp_hip_solve_by_contig_*): validation and sort keys, the bounds of each
// contig's run in grouped order, the gather of a batch's columns, and the keep mask scattered back to input order.
// The grouping itself is the stable LSD record radix of radix_sort.inc.hip on the keys k_bc_keys writes: a stable sort
// keeps input order inside every contig, which is what makes the grouped solve equal to solving each contig on its own
// reads in input order (the canonical selection breaks ties by read index).
// Every kernel here moves bytes and nothing else: grid-stride loops of 256 threads, capped at grid_for's 2048 blocks.

// key = contig id; an unplaced read (QMCP_NO_CONTIG) gets n_contigs, which sorts behind every contig and is never
// solved.  err (one word, zeroed by the host): bit 0 an id that is neither < n_contigs nor the sentinel, bit 1 a placed
// read with start > end or end >= its contig's length.
__global__ __launch_bounds__(256) void k_bc_keys(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                 const uint32_t* __restrict__ ids, uint32_t n,
                                                 const uint32_t* __restrict__ lengths, uint32_t n_contigs,
                                                 uint32_t* __restrict__ keys, uint32_t* __restrict__ err) {
    uint32_t bad = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t id = ids[i];
        uint32_t key = n_contigs;
        if (id < n_contigs) {
            const uint32_t s = starts[i], e = ends[i];
            if (s > e || e >= lengths[id]) bad |= 2u;
            key = id;
        } else if (id != QMCP_NO_CONTIG) {
            bad |= 1u;
        }
        keys[i] = key;
    }
    if (bad) atomicOr(err, bad);
}

// offs[k] = the first grouped position whose key is >= k, for k in [0, n_groups]: contig c owns grouped reads
// [offs[c], offs[c + 1]), the unplaced reads are [offs[n_groups - 1], n).  Position g writes the entries of the keys that
// begin at it (those after key[g - 1] up to key[g]), so every entry is written exactly once, empty contigs included.
__global__ __launch_bounds__(256) void k_bc_bounds(const Rec* __restrict__ sorted, uint32_t n, uint32_t n_groups,
                                                   uint32_t* __restrict__ offs) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g <= n; g += gridDim.x * blockDim.x) {
        const uint32_t lo = g == 0 ? 0u : sorted[g - 1].key + 1u;
        const uint32_t hi = g == n ? n_groups : sorted[g].key;
        for (uint32_t k = lo; k <= hi; ++k) offs[k] = g;
    }
}

// a batch's columns in grouped order: out[j] = in[sorted[j].val]
__global__ __launch_bounds__(256) void k_bc_gather(const Rec* __restrict__ sorted, uint32_t n,
                                                   const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                   uint32_t* __restrict__ starts_out, uint32_t* __restrict__ ends_out) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const uint32_t i = sorted[j].val;
        starts_out[j] = starts[i];
        ends_out[j] = ends[i];
    }
}

// grouped-mask bit j of the batch -> input bit sorted[j].val of the (zeroed) input-order mask, one 32-bit atomicOr per
// kept read: only kept reads touch the permutation, and a word of the input mask collects bits from anywhere
__global__ __launch_bounds__(256) void k_bc_scatter_mask(const uint64_t* __restrict__ batch_mask, const Rec* __restrict__ sorted,
                                                         uint32_t n, uint32_t* __restrict__ mask) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        if ((batch_mask[j >> 6] >> (j & 63u)) & 1ull) {
            const uint32_t i = sorted[j].val;
            atomicOr(&mask[i >> 5], 1u << (i & 31u));
        }
    }
}

void launch_bc_keys(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids, uint32_t n,
                    const uint32_t* lengths, uint32_t n_contigs, uint32_t* keys, uint32_t* err) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_bc_keys, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, ends, ids, n, lengths, n_contigs,
                       keys, err);
}
void launch_bc_bounds(hipStream_t st, const void* sorted, uint32_t n, uint32_t n_groups, uint32_t* offs) {
    hipLaunchKernelGGL(k_bc_bounds, dim3(grid_for((uint64_t)n + 1, 256)), dim3(256), 0, st, (const Rec*)sorted, n,
                       n_groups, offs);
}
void launch_bc_gather(hipStream_t st, const void* sorted, uint32_t n, const uint32_t* starts, const uint32_t* ends,
                      uint32_t* starts_out, uint32_t* ends_out) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_bc_gather, dim3(grid_for(n, 256)), dim3(256), 0, st, (const Rec*)sorted, n, starts, ends,
                       starts_out, ends_out);
}
void launch_bc_scatter_mask(hipStream_t st, const uint64_t* batch_mask, const void* sorted, uint32_t n, uint64_t* mask) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_bc_scatter_mask, dim3(grid_for(n, 256)), dim3(256), 0, st, batch_mask, (const Rec*)sorted, n,
                       (uint32_t*)mask);
}
