// ladder.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after by_contig).
// The coverage ladder (qmcp_hip_solve_ladder_*): between two levels of a batch, the reads the last solve kept become
// the next solve's reads.  The stable compaction of a batch's columns with an origin column (the compact read's input
// index), the next level's contig offsets (the kept rank at each contig's offset), and the level bytes.
// Every kernel here moves bytes and nothing else: grid-stride loops of 256 threads, capped at grid_for's 2048 blocks.

// Stable compaction of the kept reads of one level.  A thread owns four consecutive reads -- one nibble of a mask word
// -- and skips them without touching the columns when none is kept (after the first level a few percent are).  Kept
// read i becomes compact read word_base[i / 64] + (set bits of its word below it).  FIRST: the origin comes from the
// grouping's {key, index} records, otherwise from the previous level's origin column.  VEC: the three columns are
// 16-byte aligned, so a whole quad is two (FIRST: four) 16-byte loads.
template <bool FIRST, bool VEC>
__global__ __launch_bounds__(256) void k_ladder_compact(const uint32_t* __restrict__ starts,
                                                        const uint32_t* __restrict__ ends,
                                                        const void* __restrict__ origin_in,
                                                        const uint64_t* __restrict__ mask,
                                                        const uint32_t* __restrict__ word_base, uint32_t n,
                                                        uint32_t* __restrict__ starts_c, uint32_t* __restrict__ ends_c,
                                                        uint32_t* __restrict__ origin_c) {
    const uint32_t n_quads = (n + 3u) / 4u;  // (n <= 2^30)
    const Rec* recs = (const Rec*)origin_in;
    const uint32_t* orig = (const uint32_t*)origin_in;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n_quads; q += gridDim.x * blockDim.x) {
        const uint32_t i0 = 4u * q;
        const uint64_t word = mask[i0 >> 6];
        const uint32_t bit = i0 & 63u;
        const uint32_t left = n - i0;  // reads of this quad that exist: >= 1
        const uint32_t nib = (uint32_t)(word >> bit) & (left >= 4u ? 0xFu : (1u << left) - 1u);
        if (nib == 0) continue;
        uint32_t s4[4], e4[4], o4[4];
        if (VEC && left >= 4u) {
            const uint4 s = *(const uint4*)(starts + i0);
            const uint4 e = *(const uint4*)(ends + i0);
            s4[0] = s.x; s4[1] = s.y; s4[2] = s.z; s4[3] = s.w;
            e4[0] = e.x; e4[1] = e.y; e4[2] = e.z; e4[3] = e.w;
            if (FIRST) {
                const uint4 a = *(const uint4*)(recs + i0);
                const uint4 b = *(const uint4*)(recs + i0 + 2);
                o4[0] = a.y; o4[1] = a.w; o4[2] = b.y; o4[3] = b.w;
            } else {
                const uint4 o = *(const uint4*)(orig + i0);
                o4[0] = o.x; o4[1] = o.y; o4[2] = o.z; o4[3] = o.w;
            }
        } else {
#pragma unroll
            for (uint32_t r = 0; r < 4u; ++r) {
                const bool in = r < left;
                s4[r] = in ? starts[i0 + r] : 0u;
                e4[r] = in ? ends[i0 + r] : 0u;
                o4[r] = in ? (FIRST ? recs[i0 + r].val : orig[i0 + r]) : 0u;
            }
        }
        uint32_t dst = word_base[i0 >> 6] + (uint32_t)__popcll(word & ((1ull << bit) - 1ull));
#pragma unroll
        for (uint32_t r = 0; r < 4u; ++r) {
            if ((nib >> r) & 1u) {
                starts_c[dst] = s4[r];
                ends_c[dst] = e4[r];
                origin_c[dst] = o4[r];
                ++dst;
            }
        }
    }
}

// next[k] = the number of kept reads before read offs[k], for k in [0, n_contigs]: the next level's contig offsets
// (next[n_contigs] is its number of reads).  word_base has the scan's total behind its last word, which is where
// offs[k] == n lands when n is a multiple of 64; an empty contig repeats its neighbour's value.
__global__ __launch_bounds__(256) void k_ladder_offsets(const uint32_t* __restrict__ offs, uint32_t n_contigs,
                                                        const uint64_t* __restrict__ mask,
                                                        const uint32_t* __restrict__ word_base,
                                                        uint32_t* __restrict__ next) {
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k <= n_contigs; k += gridDim.x * blockDim.x) {
        const uint32_t off = offs[k];
        const uint32_t bit = off & 63u;
        uint32_t rank = word_base[off >> 6];
        if (bit) rank += (uint32_t)__popcll(mask[off >> 6] & ((1ull << bit) - 1ull));  // (bit != 0: the word exists)
        next[k] = rank;
    }
}

// levels[origin of read j] = level for the reads this level's solve kept; the others keep the byte they have
template <bool FIRST>
__global__ __launch_bounds__(256) void k_ladder_levels(const uint64_t* __restrict__ mask,
                                                       const void* __restrict__ origin_in, uint32_t n, uint8_t level,
                                                       uint8_t* __restrict__ levels) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        if ((mask[j >> 6] >> (j & 63u)) & 1ull) {
            const uint32_t o = FIRST ? ((const Rec*)origin_in)[j].val : ((const uint32_t*)origin_in)[j];
            levels[o] = level;
        }
    }
}

void launch_ladder_compact(hipStream_t st, bool first, const uint32_t* starts, const uint32_t* ends,
                           const void* origin_in, const uint64_t* mask, const uint32_t* word_base, uint32_t n,
                           uint32_t* starts_c, uint32_t* ends_c, uint32_t* origin_c) {
    if (n == 0) return;
    const dim3 grid(grid_for(((uint64_t)n + 3) / 4, 256)), block(256);
    const bool vec = (((uintptr_t)starts | (uintptr_t)ends | (uintptr_t)origin_in) & 15u) == 0;
#define QMCP_LC(FIRST, VEC)                                                                                          \
    hipLaunchKernelGGL((k_ladder_compact<FIRST, VEC>), grid, block, 0, st, starts, ends, origin_in, mask, word_base, n, \
                       starts_c, ends_c, origin_c)
    if (first && vec) QMCP_LC(true, true);
    else if (first) QMCP_LC(true, false);
    else if (vec) QMCP_LC(false, true);
    else QMCP_LC(false, false);
#undef QMCP_LC
}

void launch_ladder_offsets(hipStream_t st, const uint32_t* offs, uint32_t n_contigs, const uint64_t* mask,
                           const uint32_t* word_base, uint32_t* next) {
    hipLaunchKernelGGL(k_ladder_offsets, dim3(grid_for((uint64_t)n_contigs + 1, 256)), dim3(256), 0, st, offs, n_contigs,
                       mask, word_base, next);
}

void launch_ladder_levels(hipStream_t st, bool first, const uint64_t* mask, const void* origin_in, uint32_t n,
                          uint32_t level, uint8_t* levels) {
    if (n == 0) return;
    if (first)
        hipLaunchKernelGGL(k_ladder_levels<true>, dim3(grid_for(n, 256)), dim3(256), 0, st, mask, origin_in, n,
                           (uint8_t)level, levels);
    else
        hipLaunchKernelGGL(k_ladder_levels<false>, dim3(grid_for(n, 256)), dim3(256), 0, st, mask, origin_in, n,
                           (uint8_t)level, levels);
}
