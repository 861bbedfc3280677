// replicates.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after ladder,
// targets and pairs).
// Disjoint replicates (qmcp_hip_solve_replicates_*): between two replicates the reads a solve did NOT take become the
// next solve's reads.  On deep data that is 90 % or more of them, the opposite of the ladder's few per cent, so the
// compaction here is a dense one: whole tiles staged in LDS and streamed out, not scattered stores of a few survivors.
//   k_rep_split            one pass over a replicate's candidates: the taken ones get their label, the free ones go,
//                          stably, to the other column set at their rank among the free reads
//   k_rep_offsets          the next replicate's contig offsets: the free rank at each contig's offset
//   k_rep_mark             whole pairs / several batches: labels and the input-order taken mask from a solve's mask
//   k_rep_gather_taken     ... and that mask back in candidate order (k_pair_gather_mask through either origin form)
//   k_rep_label_input      labels from an input-order mask (replicate 1 of such a call)
//   k_rep_complete_pairs   the free placed mates of a replicate's reads join it
//   k_rep_label_mask       the packed mask of one label (the shortfall pass reads it)
// No atomics in the split: the output position of every free read follows from the scanned popcounts alone.

// taken candidates before candidate i (word_base: the scanned word popcounts, the total behind the last word; a bit
// index of 0 never touches a word that may not exist)
__device__ __forceinline__ uint32_t rep_taken_before(const uint64_t* __restrict__ taken,
                                                     const uint32_t* __restrict__ taken_base, uint32_t i) {
    const uint32_t bit = i & 63u;
    uint32_t rank = taken_base[i >> 6];
    if (bit) rank += (uint32_t)__popcll(taken[i >> 6] & ((1ull << bit) - 1ull));
    return rank;
}

// A workgroup takes tiles of kRepTileReads candidates = 16 whole mask words; a thread owns four consecutive candidates,
// one nibble of a word.  The free rank of candidate i is i - (taken before i), so the tile's free reads go to
// [out0, out0 + count) with out0 the free rank of the tile's first candidate: each thread stores its free reads into LDS
// at (free rank - out0), and the tile then leaves LDS front to back -- 16-byte stores from the first 16-byte aligned
// output index on (WIDE: the output columns are 16-byte aligned), single words before and behind.
// Bits of the last word beyond n are ignored whatever they hold.  FIRST: the origin comes from the grouping's
// {key, index} records.  VEC: the three input columns are 16-byte aligned.  LABEL: taken candidates get labels[origin].
template <bool FIRST, bool VEC, bool LABEL, bool WIDE>
__global__ __launch_bounds__(256) void k_rep_split(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                   const void* __restrict__ origin_in,
                                                   const uint64_t* __restrict__ taken,
                                                   const uint32_t* __restrict__ taken_base, uint32_t n, uint8_t label,
                                                   uint8_t* __restrict__ labels, uint32_t* __restrict__ starts_f,
                                                   uint32_t* __restrict__ ends_f, uint32_t* __restrict__ origin_f) {
    __shared__ uint32_t s_s[kRepTileReads], s_e[kRepTileReads], s_o[kRepTileReads];
    const Rec* recs = (const Rec*)origin_in;
    const uint32_t* orig = (const uint32_t*)origin_in;
    const uint32_t n_tiles = (n + kRepTileReads - 1u) / kRepTileReads;  // (n <= 2^30)
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t r0 = tile * kRepTileReads;
        const uint32_t r1 = min(r0 + kRepTileReads, n);
        const uint32_t out0 = r0 - taken_base[r0 >> 6];
        const uint32_t count = (r1 - rep_taken_before(taken, taken_base, r1)) - out0;
        const uint32_t i0 = r0 + 4u * threadIdx.x;
        if (i0 < n) {
            const uint64_t word = taken[i0 >> 6];
            const uint32_t bit = i0 & 63u;
            const uint32_t left = n - i0;  // candidates of this quad that exist: >= 1
            const uint32_t valid = left >= 4u ? 0xFu : (1u << left) - 1u;
            const uint32_t tnib = (uint32_t)(word >> bit) & valid;
            const uint32_t fnib = ~tnib & valid;
            if (fnib != 0 || LABEL) {
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
                // (dst < count <= kRepTileReads: the free reads of the tile before this quad)
                uint32_t dst = i0 - (taken_base[i0 >> 6] + (uint32_t)__popcll(word & ((1ull << bit) - 1ull))) - out0;
#pragma unroll
                for (uint32_t r = 0; r < 4u; ++r) {
                    if ((fnib >> r) & 1u) {
                        s_s[dst] = s4[r];
                        s_e[dst] = e4[r];
                        s_o[dst] = o4[r];
                        ++dst;
                    } else if (LABEL && ((tnib >> r) & 1u)) {
                        labels[o4[r]] = label;
                    }
                }
            }
        }
        __syncthreads();
        if (WIDE) {
            const uint32_t head = min(count, (4u - (out0 & 3u)) & 3u);
            const uint32_t n_vec = (count - head) / 4u;
            if (threadIdx.x < head) {
                starts_f[out0 + threadIdx.x] = s_s[threadIdx.x];
                ends_f[out0 + threadIdx.x] = s_e[threadIdx.x];
                origin_f[out0 + threadIdx.x] = s_o[threadIdx.x];
            }
            for (uint32_t g = threadIdx.x; g < n_vec; g += blockDim.x) {
                const uint32_t t = head + 4u * g;
                *(uint4*)(starts_f + out0 + t) = make_uint4(s_s[t], s_s[t + 1], s_s[t + 2], s_s[t + 3]);
                *(uint4*)(ends_f + out0 + t) = make_uint4(s_e[t], s_e[t + 1], s_e[t + 2], s_e[t + 3]);
                *(uint4*)(origin_f + out0 + t) = make_uint4(s_o[t], s_o[t + 1], s_o[t + 2], s_o[t + 3]);
            }
            const uint32_t t = head + 4u * n_vec + threadIdx.x;
            if (t < count) {
                starts_f[out0 + t] = s_s[t];
                ends_f[out0 + t] = s_e[t];
                origin_f[out0 + t] = s_o[t];
            }
        } else {
            for (uint32_t t = threadIdx.x; t < count; t += blockDim.x) {
                starts_f[out0 + t] = s_s[t];
                ends_f[out0 + t] = s_e[t];
                origin_f[out0 + t] = s_o[t];
            }
        }
        __syncthreads();
    }
}

// next[k] = offs[k] - (taken candidates before offs[k]), k in [0, n_contigs]: the next replicate's contig offsets
// (next[n_contigs] is its number of reads); a contig whose reads are all taken repeats its neighbour's value
__global__ __launch_bounds__(256) void k_rep_offsets(const uint32_t* __restrict__ offs, uint32_t n_contigs,
                                                     const uint64_t* __restrict__ taken,
                                                     const uint32_t* __restrict__ taken_base, uint32_t* __restrict__ next) {
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k <= n_contigs; k += gridDim.x * blockDim.x) {
        const uint32_t off = offs[k];
        next[k] = off - rep_taken_before(taken, taken_base, off);
    }
}

// a solve's kept candidates: their label, and their bit in the input-order taken mask (one 32-bit atomicOr per kept
// read, as k_expand_mask_reads)
__global__ __launch_bounds__(256) void k_rep_mark(const uint64_t* __restrict__ kept, const uint32_t* __restrict__ origin,
                                                  uint32_t n, uint8_t label, uint8_t* __restrict__ labels,
                                                  uint32_t* __restrict__ taken32) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        if ((kept[j >> 6] >> (j & 63u)) & 1ull) {
            const uint32_t o = origin[j];
            labels[o] = label;
            atomicOr(&taken32[o >> 5], 1u << (o & 31u));
        }
    }
}

// one wave turns 64 candidates into one word of taken bits with a ballot; the last word's bits beyond n are 0
template <bool FIRST>
__global__ __launch_bounds__(256) void k_rep_gather_taken(const void* __restrict__ origin_in, uint32_t n,
                                                          const uint64_t* __restrict__ taken_in,
                                                          uint64_t* __restrict__ taken) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_words = (n + 63u) / 64u;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_words; w += waves) {
        const uint32_t j = 64u * w + lane;
        bool in = false;
        if (j < n) {
            const uint32_t i = FIRST ? ((const Rec*)origin_in)[j].val : ((const uint32_t*)origin_in)[j];
            in = ((taken_in[i >> 6] >> (i & 63u)) & 1ull) != 0;
        }
        const uint64_t word = __ballot(in);
        if (lane == 0) taken[w] = word;
    }
}

__global__ __launch_bounds__(256) void k_rep_label_input(const uint64_t* __restrict__ mask, uint64_t n_reads, uint8_t label,
                                                         uint8_t* __restrict__ labels) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_reads; i += stride)
        if ((mask[i >> 6] >> (i & 63u)) & 1ull) labels[i] = label;
}

// Pair q = reads (2q, 2q + 1).  Pairs move together, so a read with label 0 beside a mate with `label` is free; it joins
// when it is placed.  n_reads is even.
__global__ __launch_bounds__(256) void k_rep_complete_pairs(const uint32_t* __restrict__ ids, uint64_t n_pairs, uint8_t label,
                                                            uint8_t* __restrict__ labels, uint32_t* __restrict__ taken32,
                                                            unsigned long long* __restrict__ n_mates) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (n_pairs + stride - 1) / stride;  // every lane of a wave makes every trip: the ballot is whole
    uint32_t joined = 0;
    for (uint64_t t = 0; t < rounds; ++t) {
        const uint64_t q = t * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        bool join = false;
        uint64_t i = 0;
        if (q < n_pairs) {
            const uint8_t a = labels[2 * q], b = labels[2 * q + 1];
            if (a == label && b == 0) i = 2 * q + 1, join = true;
            else if (b == label && a == 0) i = 2 * q, join = true;
            if (join) join = ids[i] != 0xFFFFFFFFu;  // (QMCP_NO_CONTIG: an unplaced mate never joins)
            if (join) {
                labels[i] = label;
                atomicOr(&taken32[i >> 5], 1u << (uint32_t)(i & 31u));
            }
        }
        joined += (uint32_t)__popcll(__ballot(join));
    }
    if ((threadIdx.x & 63u) == 0 && joined) atomicAdd(n_mates, (unsigned long long)joined);
}

// one wave per word of the packed mask of labels == label
__global__ __launch_bounds__(256) void k_rep_label_mask(const uint8_t* __restrict__ labels, uint64_t n_reads, uint8_t label,
                                                        uint64_t* __restrict__ mask) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_words = (uint32_t)((n_reads + 63) / 64);
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_words; w += waves) {
        const uint64_t i = 64ull * w + lane;
        const uint64_t word = __ballot(i < n_reads && labels[i] == label);
        if (lane == 0) mask[w] = word;
    }
}

void launch_rep_split(hipStream_t st, bool first, const uint32_t* starts, const uint32_t* ends, const void* origin_in,
                      const uint64_t* taken, const uint32_t* taken_base, uint32_t n, uint32_t label, uint8_t* labels,
                      uint32_t* starts_f, uint32_t* ends_f, uint32_t* origin_f) {
    if (n == 0) return;
    const dim3 grid(grid_for(n, kRepTileReads)), block(256);
    const bool vec = (((uintptr_t)starts | (uintptr_t)ends | (uintptr_t)origin_in) & 15u) == 0;
    const bool wide = (((uintptr_t)starts_f | (uintptr_t)ends_f | (uintptr_t)origin_f) & 15u) == 0;
    const bool lab = label != 0;
#define QMCP_RS(FIRST, VEC, LABEL, WIDE)                                                                               \
    hipLaunchKernelGGL((k_rep_split<FIRST, VEC, LABEL, WIDE>), grid, block, 0, st, starts, ends, origin_in, taken,      \
                       taken_base, n, (uint8_t)label, labels, starts_f, ends_f, origin_f)
#define QMCP_RS2(FIRST, VEC)                          \
    do {                                              \
        if (lab && wide) QMCP_RS(FIRST, VEC, true, true);        \
        else if (lab) QMCP_RS(FIRST, VEC, true, false);          \
        else if (wide) QMCP_RS(FIRST, VEC, false, true);         \
        else QMCP_RS(FIRST, VEC, false, false);                  \
    } while (0)
    if (first && vec) QMCP_RS2(true, true);
    else if (first) QMCP_RS2(true, false);
    else if (vec) QMCP_RS2(false, true);
    else QMCP_RS2(false, false);
#undef QMCP_RS2
#undef QMCP_RS
}

void launch_rep_offsets(hipStream_t st, const uint32_t* offs, uint32_t n_contigs, const uint64_t* taken,
                        const uint32_t* taken_base, uint32_t* next) {
    hipLaunchKernelGGL(k_rep_offsets, dim3(grid_for((uint64_t)n_contigs + 1, 256)), dim3(256), 0, st, offs, n_contigs, taken,
                       taken_base, next);
}

void launch_rep_mark(hipStream_t st, const uint64_t* kept, const uint32_t* origin, uint32_t n, uint32_t label,
                     uint8_t* labels, uint64_t* taken_in) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_rep_mark, dim3(grid_for(n, 256)), dim3(256), 0, st, kept, origin, n, (uint8_t)label, labels,
                       (uint32_t*)taken_in);
}

void launch_rep_gather_taken(hipStream_t st, bool first, const void* origin_in, uint32_t n, const uint64_t* taken_in,
                             uint64_t* taken) {
    if (n == 0) return;
    const dim3 grid(grid_for(n, 256)), block(256);
    if (first) hipLaunchKernelGGL(k_rep_gather_taken<true>, grid, block, 0, st, origin_in, n, taken_in, taken);
    else hipLaunchKernelGGL(k_rep_gather_taken<false>, grid, block, 0, st, origin_in, n, taken_in, taken);
}

void launch_rep_label_input(hipStream_t st, const uint64_t* mask, uint64_t n_reads, uint32_t label, uint8_t* labels) {
    if (n_reads == 0) return;
    hipLaunchKernelGGL(k_rep_label_input, dim3(grid_for(n_reads, 256)), dim3(256), 0, st, mask, n_reads, (uint8_t)label,
                       labels);
}

void launch_rep_complete_pairs(hipStream_t st, const uint32_t* ids, uint64_t n_reads, uint32_t label, uint8_t* labels,
                               uint64_t* taken_in, unsigned long long* n_mates) {
    if (n_reads < 2) return;
    hipLaunchKernelGGL(k_rep_complete_pairs, dim3(grid_for(n_reads / 2, 256)), dim3(256), 0, st, ids, n_reads / 2,
                       (uint8_t)label, labels, (uint32_t*)taken_in, n_mates);
}

void launch_rep_label_mask(hipStream_t st, const uint8_t* labels, uint64_t n_reads, uint32_t label, uint64_t* mask) {
    if (n_reads == 0) return;
    hipLaunchKernelGGL(k_rep_label_mask, dim3(grid_for(n_reads, 256)), dim3(256), 0, st, labels, n_reads, (uint8_t)label,
                       mask);
}
