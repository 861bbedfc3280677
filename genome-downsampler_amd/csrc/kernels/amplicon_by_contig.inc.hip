// amplicon_by_contig.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after
// launchers).  The FILTER of qmcp_hip_filter_solve_by_contig_host: pairs (reads 2q, 2q + 1) of several contigs, each
// read with its contig id, against the amplicons of its own contig (amplicon_table.h); and the compaction of the
// surviving pairs that carries the ids along.  Both move bytes and nothing else: grid-stride loops of 256 threads,
// capped at grid_for's 2048 blocks.

constexpr uint32_t kAmpLdsMax = 4096;  // amplicons staged in LDS: 2 x 4 096 words = 32 KiB, as k_amplicon_filter

// kTab: 0 no amplicons (AmpliconBehaviour::IGNORE: only the length / MAPQ filters act), 1 the table in LDS (at most
// kAmpLdsMax amplicons), 2 the table read from global memory.  One wave emits one 64-pair word with a ballot.
// Every read is validated as k_bc_keys does, those of dropped pairs included (the by-contig solve only sees the
// survivors): err bit 0 an id that is neither < n_contigs nor QMCP_NO_CONTIG, bit 1 a placed read with start > end or
// end >= its contig's length.  A pair survives with amplicons iff both mates are placed on one contig c and the last
// amplicon of c starting at or before min(s1, s2) has a running maximum end >= max(e1, e2).
template <int kTab>
__global__ __launch_bounds__(256) void k_amplicon_filter_by_contig(
    const uint2* __restrict__ starts, const uint2* __restrict__ ends, const uint2* __restrict__ ids,
    const uint2* __restrict__ seq_lengths, const uint2* __restrict__ qualities, uint64_t n_pairs,
    const uint32_t* __restrict__ lengths, uint32_t n_contigs, const uint32_t* __restrict__ amp_offs,
    const uint32_t* __restrict__ amp_starts, const uint32_t* __restrict__ amp_pmax, uint32_t n_amp,
    uint32_t min_length, uint32_t min_mapq, uint64_t* __restrict__ pair_keep, uint32_t* __restrict__ err) {
    extern __shared__ uint32_t s_tab[];  // kTab == 1: [n_amp starts | n_amp running maxima]
    const uint32_t* tab_s = amp_starts;
    const uint32_t* tab_p = amp_pmax;
    if constexpr (kTab == 1) {
        for (uint32_t i = threadIdx.x; i < n_amp; i += blockDim.x) {
            s_tab[i] = amp_starts[i];
            s_tab[n_amp + i] = amp_pmax[i];
        }
        __syncthreads();
        tab_s = s_tab;
        tab_p = s_tab + n_amp;
    }
    const uint64_t n_words = (n_pairs + 63) / 64;
    const uint64_t wave_global = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t bad = 0;
    for (uint64_t w = wave_global; w < n_words; w += n_waves) {
        const uint64_t q = w * 64 + lane;
        bool ok = false;
        if (q < n_pairs) {
            const uint2 s = starts[q], e = ends[q], id = ids[q];
            // validation of both mates
            bool placed1 = false, placed2 = false;
            if (id.x < n_contigs) {
                placed1 = true;
                if (s.x > e.x || e.x >= lengths[id.x]) bad |= 2u;
            } else if (id.x != QMCP_NO_CONTIG) {
                bad |= 1u;
            }
            if (id.y < n_contigs) {
                placed2 = true;
                if (s.y > e.y || e.y >= lengths[id.y]) bad |= 2u;
            } else if (id.y != QMCP_NO_CONTIG) {
                bad |= 1u;
            }
            bool pass = true;
            if (qualities) {
                const uint2 mq = qualities[q];
                pass = pass && mq.x >= min_mapq && mq.y >= min_mapq;
            }
            if (seq_lengths) {
                const uint2 ln = seq_lengths[q];
                pass = pass && ln.x >= min_length && ln.y >= min_length;
            }
            if constexpr (kTab != 0) {
                bool in_one = false;
                if (placed1 && placed2 && id.x == id.y) {
                    const uint32_t lo = amp_offs[id.x], hi = amp_offs[id.x + 1];
                    const uint32_t m = min(s.x, s.y);
                    uint32_t a = lo, b = hi;  // first amplicon of the contig with start > m lies in [a, b]
                    while (a < b) {
                        const uint32_t mid = a + ((b - a) >> 1);
                        if (tab_s[mid] <= m) a = mid + 1;
                        else b = mid;
                    }
                    in_one = a != lo && tab_p[a - 1] >= max(e.x, e.y);
                }
                pass = pass && in_one;
            }
            ok = pass;
        }
        const uint64_t word = __ballot(ok);
        if (lane == 0) pair_keep[w] = word;
    }
    if (bad) atomicOr(err, bad);
}

// k_compact_pairs with the contig ids carried along (surviving pair q' becomes reads 2q', 2q' + 1; orig_pair[q'] = q)
__global__ __launch_bounds__(256) void k_compact_pairs_ids(const uint2* __restrict__ starts, const uint2* __restrict__ ends,
                                                           const uint2* __restrict__ ids,
                                                           const uint64_t* __restrict__ pair_keep,
                                                           const uint32_t* __restrict__ word_base, uint64_t n_pairs,
                                                           uint2* __restrict__ starts_c, uint2* __restrict__ ends_c,
                                                           uint2* __restrict__ ids_c, uint32_t* __restrict__ orig_pair) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_pairs; q += stride) {
        const uint64_t word = pair_keep[q >> 6];
        const uint32_t bit = (uint32_t)(q & 63);
        if ((word >> bit) & 1ull) {
            const uint32_t dst = word_base[q >> 6] + (uint32_t)__popcll(word & ((1ull << bit) - 1ull));
            starts_c[dst] = starts[q];
            ends_c[dst] = ends[q];
            ids_c[dst] = ids[q];
            orig_pair[dst] = (uint32_t)q;
        }
    }
}

void launch_amplicon_filter_by_contig(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                                      const uint32_t* seq_lengths, const uint32_t* qualities, uint64_t n_pairs,
                                      const uint32_t* lengths, uint32_t n_contigs, const uint32_t* amp_offs,
                                      const uint32_t* amp_starts, const uint32_t* amp_pmax, uint32_t n_amp,
                                      uint32_t min_length, uint32_t min_mapq, uint64_t* pair_keep, uint32_t* err) {
    if (n_pairs == 0) return;
    const dim3 grid(grid_for(((n_pairs + 63) / 64) * 64, 256)), block(256);
    const uint2 *s = (const uint2*)starts, *e = (const uint2*)ends, *id = (const uint2*)ids;
    const uint2 *ln = (const uint2*)seq_lengths, *mq = (const uint2*)qualities;
    if (!amp_offs) {
        hipLaunchKernelGGL(k_amplicon_filter_by_contig<0>, grid, block, 0, st, s, e, id, ln, mq, n_pairs, lengths,
                           n_contigs, amp_offs, amp_starts, amp_pmax, n_amp, min_length, min_mapq, pair_keep, err);
    } else if (n_amp <= kAmpLdsMax) {
        hipLaunchKernelGGL(k_amplicon_filter_by_contig<1>, grid, block, 2 * n_amp * sizeof(uint32_t), st, s, e, id, ln,
                           mq, n_pairs, lengths, n_contigs, amp_offs, amp_starts, amp_pmax, n_amp, min_length, min_mapq,
                           pair_keep, err);
    } else {
        hipLaunchKernelGGL(k_amplicon_filter_by_contig<2>, grid, block, 0, st, s, e, id, ln, mq, n_pairs, lengths,
                           n_contigs, amp_offs, amp_starts, amp_pmax, n_amp, min_length, min_mapq, pair_keep, err);
    }
}

void launch_compact_pairs_ids(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                              const uint64_t* pair_keep, const uint32_t* word_base, uint64_t n_pairs, uint32_t* starts_c,
                              uint32_t* ends_c, uint32_t* ids_c, uint32_t* orig_pair) {
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(k_compact_pairs_ids, dim3(grid_for(n_pairs, 256)), dim3(256), 0, st, (const uint2*)starts,
                       (const uint2*)ends, (const uint2*)ids, pair_keep, word_base, n_pairs, (uint2*)starts_c,
                       (uint2*)ends_c, (uint2*)ids_c, orig_pair);
}
