// targets.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after launchers).
// The pre- and post-pass of qmcp_hip_solve_targets_*: every read validated and projected onto the compressed axis of its
// contig's target positions (target_table.h: project_read is the one definition the host test shares), the stable
// compaction of the on-target reads, and the compact keep mask expanded back to input order.  All of it moves bytes:
// grid-stride loops of 256 threads, capped at grid_for's 2048 blocks.

constexpr uint32_t kTargetLdsMax = 4096;  // merged regions staged in LDS (bounds only: 2 x 4 096 words = 32 KiB, as the
                                          // amplicon FILTER; cum is read twice per on-target read and stays in L2)

// one read: validated as k_bc_keys does (bad |= 1 an id that is neither < n_contigs nor QMCP_NO_CONTIG, |= 2 a placed
// read with start > end or end >= its contig's length); returns 1 on target (*ps, *pe written), 2 placed and off target
// (a contig without target positions has only such reads), 0 unplaced or invalid
__device__ __forceinline__ uint32_t project_one(uint32_t s, uint32_t e, uint32_t id, const uint32_t* __restrict__ lengths,
                                                uint32_t n_contigs, const uint32_t* __restrict__ offs, const uint32_t* rs,
                                                const uint32_t* re, const uint32_t* __restrict__ cum, uint32_t& bad,
                                                uint32_t* ps, uint32_t* pe) {
    *ps = 0;
    *pe = 0;
    if (id >= n_contigs) {
        if (id != QMCP_NO_CONTIG) bad |= 1u;
        return 0;
    }
    if (s > e || e >= lengths[id]) {
        bad |= 2u;
        return 0;
    }
    return project_read(rs, re, cum, offs[id], offs[id + 1], s, e, ps, pe) ? 1u : 2u;
}

// kTab: 1 the regions' bounds in LDS (at most kTargetLdsMax merged regions), 2 read from global memory.
// kVec: the three columns are 16-byte aligned -- a lane loads four consecutive reads of each with one 128-bit load and
// stores their projections the same way (the outputs are arena buffers, always aligned); otherwise 32-bit accesses, lane
// l of a wave taking reads l, l + 64, l + 128, l + 192 of the wave's 256.  Either way a wave owns 256 consecutive reads
// = four 64-bit words of each mask, written by its lanes 0..3: kVec interleaves its four ballots (ballot r holds read
// 4 l + r at bit l) with spread_bits_by_4, the 32-bit form's ballot r is word r as it stands.
// on: bit i = read i is on target; off: bit i = read i is placed and off target.  ps / pe: the projection (0 elsewhere).
template <int kTab, bool kVec>
__global__ __launch_bounds__(256) void k_target_project(
    const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends, const uint32_t* __restrict__ ids, uint32_t n,
    const uint32_t* __restrict__ lengths, uint32_t n_contigs, const uint32_t* __restrict__ offs,
    const uint32_t* __restrict__ g_rs, const uint32_t* __restrict__ g_re, const uint32_t* __restrict__ cum,
    uint32_t n_regions, uint32_t* __restrict__ ps, uint32_t* __restrict__ pe, uint64_t* __restrict__ on,
    uint64_t* __restrict__ off, uint32_t* __restrict__ err) {
    extern __shared__ uint32_t s_tab[];  // kTab == 1: [n_regions starts | n_regions ends]
    const uint32_t* rs = g_rs;
    const uint32_t* re = g_re;
    if constexpr (kTab == 1) {
        for (uint32_t i = threadIdx.x; i < n_regions; i += blockDim.x) {
            s_tab[i] = g_rs[i];
            s_tab[n_regions + i] = g_re[i];
        }
        __syncthreads();
        rs = s_tab;
        re = s_tab + n_regions;
    }
    const uint32_t n_words = (n + 63u) / 64u;
    const uint32_t n_chunks = (n + 255u) / 256u;
    const uint32_t wave_global = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t bad = 0;
    for (uint32_t ch = wave_global; ch < n_chunks; ch += n_waves) {
        const uint64_t base = (uint64_t)ch * 256u;
        uint32_t s4[4], e4[4], id4[4], p4[4], q4[4], kind[4];
        if constexpr (kVec) {
            const uint64_t i0 = base + 4u * lane;
            if (i0 + 3 < n) {
                const uint4 s = *(const uint4*)(starts + i0), e = *(const uint4*)(ends + i0), d = *(const uint4*)(ids + i0);
                s4[0] = s.x; s4[1] = s.y; s4[2] = s.z; s4[3] = s.w;
                e4[0] = e.x; e4[1] = e.y; e4[2] = e.z; e4[3] = e.w;
                id4[0] = d.x; id4[1] = d.y; id4[2] = d.z; id4[3] = d.w;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool in = i0 + r < n;
                    s4[r] = in ? starts[i0 + r] : 0u;
                    e4[r] = in ? ends[i0 + r] : 0u;
                    id4[r] = in ? ids[i0 + r] : QMCP_NO_CONTIG;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint64_t i = base + 64u * r + lane;
                const bool in = i < n;
                s4[r] = in ? starts[i] : 0u;
                e4[r] = in ? ends[i] : 0u;
                id4[r] = in ? ids[i] : QMCP_NO_CONTIG;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            kind[r] = project_one(s4[r], e4[r], id4[r], lengths, n_contigs, offs, rs, re, cum, bad, &p4[r], &q4[r]);
        uint64_t b_on[4], b_off[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            b_on[r] = __ballot(kind[r] == 1u);
            b_off[r] = __ballot(kind[r] == 2u);
        }
        if constexpr (kVec) {
            const uint64_t i0 = base + 4u * lane;
            if (i0 + 3 < n) {
                *(uint4*)(ps + i0) = make_uint4(p4[0], p4[1], p4[2], p4[3]);
                *(uint4*)(pe + i0) = make_uint4(q4[0], q4[1], q4[2], q4[3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (i0 + r < n) {
                        ps[i0 + r] = p4[r];
                        pe[i0 + r] = q4[r];
                    }
            }
            if (lane < 4u && 4u * ch + lane < n_words) {
                const uint32_t sh = 16u * lane;  // word `lane` of the chunk: lanes 16 * lane .. + 15, four reads each
                on[4u * ch + lane] = spread_bits_by_4(b_on[0] >> sh) | (spread_bits_by_4(b_on[1] >> sh) << 1) |
                                     (spread_bits_by_4(b_on[2] >> sh) << 2) | (spread_bits_by_4(b_on[3] >> sh) << 3);
                off[4u * ch + lane] = spread_bits_by_4(b_off[0] >> sh) | (spread_bits_by_4(b_off[1] >> sh) << 1) |
                                      (spread_bits_by_4(b_off[2] >> sh) << 2) | (spread_bits_by_4(b_off[3] >> sh) << 3);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint64_t i = base + 64u * r + lane;
                if (i < n) {
                    ps[i] = p4[r];
                    pe[i] = q4[r];
                }
            }
            if (lane < 4u && 4u * ch + lane < n_words) {
                const uint64_t w_on = lane == 0 ? b_on[0] : lane == 1 ? b_on[1] : lane == 2 ? b_on[2] : b_on[3];
                const uint64_t w_off = lane == 0 ? b_off[0] : lane == 1 ? b_off[1] : lane == 2 ? b_off[2] : b_off[3];
                on[4u * ch + lane] = w_on;
                off[4u * ch + lane] = w_off;
            }
        }
    }
    if (bad) atomicOr(err, bad);
}

// Stable compaction of single reads: on-target read i becomes compact read word_base[i / 64] + (set bits of its word
// below it), carrying its projection, its contig's index among the contigs that have target positions (remap), its
// quality when the call has qualities, and orig[dst] = i, the way back.
__global__ __launch_bounds__(256) void k_compact_reads(const uint32_t* __restrict__ ps, const uint32_t* __restrict__ pe,
                                                       const uint32_t* __restrict__ ids, const uint32_t* __restrict__ q,
                                                       const uint32_t* __restrict__ remap, const uint64_t* __restrict__ on,
                                                       const uint32_t* __restrict__ word_base, uint32_t n,
                                                       uint32_t* __restrict__ starts_c, uint32_t* __restrict__ ends_c,
                                                       uint32_t* __restrict__ ids_c, uint32_t* __restrict__ q_c,
                                                       uint32_t* __restrict__ orig) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t word = on[i >> 6];
        const uint32_t bit = i & 63u;
        if ((word >> bit) & 1ull) {
            const uint32_t dst = word_base[i >> 6] + (uint32_t)__popcll(word & ((1ull << bit) - 1ull));
            starts_c[dst] = ps[i];
            ends_c[dst] = pe[i];
            ids_c[dst] = remap[ids[i]];
            if (q) q_c[dst] = q[i];
            orig[dst] = i;
        }
    }
}

// k_expand_mask for single reads: compact read i is input read orig[i] (the mask in input order is zeroed beforehand;
// one 32-bit atomicOr per kept read, as k_expand_mask and k_bc_scatter_mask)
__global__ __launch_bounds__(256) void k_expand_mask_reads(const uint64_t* __restrict__ mask_c,
                                                           const uint32_t* __restrict__ orig, uint32_t n_c,
                                                           uint32_t* __restrict__ mask32) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_c; i += stride) {
        if ((mask_c[i >> 6] >> (i & 63u)) & 1ull) {
            const uint32_t o = orig[i];
            atomicOr(&mask32[o >> 5], 1u << (o & 31u));
        }
    }
}

// QMCP_TARGETS_KEEP_OFF_TARGET: mask |= the placed off-target reads
__global__ __launch_bounds__(256) void k_or_words(uint64_t* __restrict__ mask, const uint64_t* __restrict__ other,
                                                  uint32_t n_words) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += stride) mask[w] |= other[w];
}

void launch_target_project(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids, uint32_t n,
                           const uint32_t* lengths, uint32_t n_contigs, const uint32_t* offs, const uint32_t* rs,
                           const uint32_t* re, const uint32_t* cum, uint32_t n_regions, uint32_t* ps, uint32_t* pe,
                           uint64_t* on, uint64_t* off, uint32_t* err) {
    if (n == 0) return;
    const dim3 grid(grid_for(((uint64_t)n + 255) / 256 * 64, 256)), block(256);  // a wave per 256 reads
    const bool vec = (((uintptr_t)starts | (uintptr_t)ends | (uintptr_t)ids) & 15u) == 0;
    const bool lds = n_regions <= kTargetLdsMax;
    const size_t shm = lds ? 2 * (size_t)n_regions * sizeof(uint32_t) : 0;
#define QMCP_TP(TAB, VEC)                                                                                               \
    hipLaunchKernelGGL((k_target_project<TAB, VEC>), grid, block, shm, st, starts, ends, ids, n, lengths, n_contigs, offs, \
                       rs, re, cum, n_regions, ps, pe, on, off, err)
    if (lds && vec) QMCP_TP(1, true);
    else if (lds) QMCP_TP(1, false);
    else if (vec) QMCP_TP(2, true);
    else QMCP_TP(2, false);
#undef QMCP_TP
}

void launch_compact_reads(hipStream_t st, const uint32_t* ps, const uint32_t* pe, const uint32_t* ids, const uint32_t* q,
                          const uint32_t* remap, const uint64_t* on, const uint32_t* word_base, uint32_t n,
                          uint32_t* starts_c, uint32_t* ends_c, uint32_t* ids_c, uint32_t* q_c, uint32_t* orig) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_compact_reads, dim3(grid_for(n, 256)), dim3(256), 0, st, ps, pe, ids, q, remap, on, word_base, n,
                       starts_c, ends_c, ids_c, q_c, orig);
}

void launch_expand_mask_reads(hipStream_t st, const uint64_t* mask_c, const uint32_t* orig, uint32_t n_c, uint64_t* mask) {
    if (n_c == 0) return;
    hipLaunchKernelGGL(k_expand_mask_reads, dim3(grid_for(n_c, 256)), dim3(256), 0, st, mask_c, orig, n_c,
                       (uint32_t*)mask);
}

void launch_or_words(hipStream_t st, uint64_t* mask, const uint64_t* other, uint32_t n_words) {
    if (n_words == 0) return;
    hipLaunchKernelGGL(k_or_words, dim3(grid_for(n_words, 256)), dim3(256), 0, st, mask, other, n_words);
}
