// dedup.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after launchers).
// Duplicate-aware downsampling (qmcp_hip_solve_dedup_*): duplicate families are collapsed to one representative each
// before the by-contig solve.  dedup_plan.h states the keys; api/dedup.inc.hip drives the kernels:
//   k_dd_range        one pass over the columns: every read validated as k_bc_keys does, min / max of tag, quality and
//                     span over the placed reads, the placed reads and the pairs without a placed mate counted
//                     (16-byte loads, four reads per lane, where every column is 16-byte aligned)
//   k_dd_read_keys    a round's key of read idx[j] (round 0: read j) from the fields {q_max - q, tag - tag_min,
//                     span - min_span, gstart}, packed as the round's DedupPack says
//   k_dd_heads        1 at the first sorted record of every cell / signature (compared on the sorted keys above the
//                     score field, or on the columns themselves when the sort went field by field); scanned afterwards
//   k_dd_cell_ids     pair mode, stage 1: the dense cell id of every read, scattered back to input order
//   k_dd_pair_keys    pair mode, stage 2: a round's key of unit idx[j] from {score_max - score, max id, min id}
//   k_dd_segments     over the sorted units: the head of a family is its representative (the score is the lowest key
//                     field and the sort is stable) -- its reads' survivor bits, the other units' duplicate bits (32-bit
//                     atomicOr, only set bits touched), and every family's first sorted position
//   k_dd_family_stats over the families: size = next head - head; the size histogram in per-workgroup LDS bins (one
//                     global atomic per non-empty bin and workgroup), families, duplicate units, the largest family
//                     (the start cap runs it with its K: the units beyond K per family, the families above K)
//   k_dd_compact      the stable compaction of the survivors' three columns and their input index
// Every kernel is a grid-stride loop of 256 threads (four waves of 64) that moves bytes and nothing else.

static constexpr uint32_t kDedupHistMax = 4096;  // histogram bins a workgroup keeps in LDS

__device__ __forceinline__ uint64_t dd_pack(const DedupPack& p, const uint64_t v[kDedupMaxFields]) {
    uint64_t key = 0;
#pragma unroll
    for (uint32_t f = 0; f < kDedupMaxFields; ++f)
        if ((p.on >> f) & 1u) key |= v[f] << p.shift[f];
    return key;
}

// out (u32, preset by the host to {~0u, 0, ~0u, 0, ~0u, 0, 0, 0, 0}): tag min / max, quality min / max, span min / max over
// the placed reads, the validation word of k_bc_keys, the placed reads, and (pairs) the aligned pairs without a placed mate
template <bool VEC>
__global__ __launch_bounds__(256) void k_dd_range(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                  const uint32_t* __restrict__ ids, const uint32_t* __restrict__ tags,
                                                  const uint32_t* __restrict__ q, uint32_t n,
                                                  const uint32_t* __restrict__ lengths, uint32_t n_contigs, bool pairs,
                                                  uint32_t* __restrict__ out) {
    __shared__ uint32_t s_red[9][4];
    uint32_t tmn = 0xFFFFFFFFu, tmx = 0u, qmn = 0xFFFFFFFFu, qmx = 0u, smn = 0xFFFFFFFFu, smx = 0u;
    uint32_t bad = 0, placed = 0, dead = 0;
    const uint32_t n_quads = (uint32_t)(((uint64_t)n + 3) / 4);
    for (uint32_t quad = blockIdx.x * blockDim.x + threadIdx.x; quad < n_quads; quad += gridDim.x * blockDim.x) {
        const uint32_t i0 = 4u * quad;
        const uint32_t cnt = min(4u, n - i0);
        uint32_t id4[4], s4[4], e4[4], t4[4] = {0u, 0u, 0u, 0u}, q4[4] = {0u, 0u, 0u, 0u};
        if (VEC && cnt == 4u) {
            const uint4 a = *(const uint4*)(ids + i0), b = *(const uint4*)(starts + i0), c = *(const uint4*)(ends + i0);
            id4[0] = a.x; id4[1] = a.y; id4[2] = a.z; id4[3] = a.w;
            s4[0] = b.x; s4[1] = b.y; s4[2] = b.z; s4[3] = b.w;
            e4[0] = c.x; e4[1] = c.y; e4[2] = c.z; e4[3] = c.w;
            if (tags) { const uint4 t = *(const uint4*)(tags + i0); t4[0] = t.x; t4[1] = t.y; t4[2] = t.z; t4[3] = t.w; }
            if (q) { const uint4 t = *(const uint4*)(q + i0); q4[0] = t.x; q4[1] = t.y; q4[2] = t.z; q4[3] = t.w; }
        } else {
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) {
                const bool in = r < cnt;
                id4[r] = in ? ids[i0 + r] : QMCP_NO_CONTIG;
                s4[r] = in ? starts[i0 + r] : 0u;
                e4[r] = in ? ends[i0 + r] : 0u;
                if (tags && in) t4[r] = tags[i0 + r];
                if (q && in) q4[r] = q[i0 + r];
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            if (r >= cnt) continue;
            const uint32_t id = id4[r];
            if (id < n_contigs) {
                if (s4[r] > e4[r] || e4[r] >= lengths[id]) {
                    bad |= 2u;
                } else {
                    const uint32_t span = e4[r] - s4[r];
                    tmn = min(tmn, t4[r]); tmx = max(tmx, t4[r]);
                    qmn = min(qmn, q4[r]); qmx = max(qmx, q4[r]);
                    smn = min(smn, span); smx = max(smx, span);
                }
                ++placed;
            } else if (id != QMCP_NO_CONTIG) {
                bad |= 1u;
            }
        }
        if (pairs) {  // (n is even: a pair never straddles the end)
            if (cnt >= 2u && id4[0] == QMCP_NO_CONTIG && id4[1] == QMCP_NO_CONTIG) ++dead;
            if (cnt == 4u && id4[2] == QMCP_NO_CONTIG && id4[3] == QMCP_NO_CONTIG) ++dead;
        }
    }
    tmn = wave_min_u32(tmn); tmx = wave_max_u32(tmx);
    qmn = wave_min_u32(qmn); qmx = wave_max_u32(qmx);
    smn = wave_min_u32(smn); smx = wave_max_u32(smx);
    bad = wave_max_u32(bad & 1u) | wave_max_u32(bad & 2u);
    placed = wave_sum_u32(placed);
    dead = wave_sum_u32(dead);
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_red[0][w] = tmn; s_red[1][w] = tmx; s_red[2][w] = qmn; s_red[3][w] = qmx; s_red[4][w] = smn; s_red[5][w] = smx;
        s_red[6][w] = bad; s_red[7][w] = placed; s_red[8][w] = dead;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const uint32_t k = threadIdx.x;
        const uint32_t a = s_red[k][0], b = s_red[k][1], c = s_red[k][2], d = s_red[k][3];
        if (k == 0 || k == 2 || k == 4) {
            const uint32_t v = min(min(a, b), min(c, d));
            if (v != 0xFFFFFFFFu) atomicMin(&out[k], v);
        } else if (k == 1 || k == 3 || k == 5) {
            const uint32_t v = max(max(a, b), max(c, d));
            if (v) atomicMax(&out[k], v);
        } else if (k == 6) {
            const uint32_t v = a | b | c | d;
            if (v) atomicOr(&out[k], v);
        } else {
            const uint32_t v = a + b + c + d;
            if (v) atomicAdd(&out[k], v);
        }
    }
}

// key of sorted record j = read idx[j] (idx == NULL: read j); tags / q may be NULL (every value 0)
template <typename KeyT>
__global__ __launch_bounds__(256) void k_dd_read_keys(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                      const uint32_t* __restrict__ ids, const uint32_t* __restrict__ tags,
                                                      const uint32_t* __restrict__ q, const uint32_t* __restrict__ idx,
                                                      const uint64_t* __restrict__ poff, uint64_t ltot, uint32_t n,
                                                      uint32_t min_span, uint32_t tag_min, uint32_t q_max, DedupPack pack,
                                                      KeyT* __restrict__ keys) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const uint32_t i = idx ? idx[j] : j;
        const uint32_t cid = ids[i];
        uint64_t v[kDedupMaxFields] = {0, 0, 0, ltot};
        if (cid != QMCP_NO_CONTIG) {
            const uint32_t s = starts[i];
            v[0] = q ? q_max - q[i] : 0u;
            v[1] = tags ? tags[i] - tag_min : 0u;
            v[2] = ends[i] - s - min_span;
            v[3] = poff[cid] + s;
        }
        keys[j] = (KeyT)dd_pack(pack, v);
    }
}

// cells of sorted records: equal keys above the `low` bits of the score field ...
struct DdCellRec { const Rec* r; uint32_t low;
                   __device__ bool same(uint32_t j) const { return (r[j].key >> low) == (r[j - 1].key >> low); } };
struct DdCell64 { const uint64_t* k; uint32_t low;
                  __device__ bool same(uint32_t j) const { return (k[j] >> low) == (k[j - 1] >> low); } };
// ... or, after a sort field by field, the columns of the records' reads / the cell ids of the records' units
struct DdCellReads { const uint32_t* v; const uint32_t* starts; const uint32_t* ends; const uint32_t* ids; const uint32_t* tags;
                     __device__ bool same(uint32_t j) const {
                         const uint32_t a = v[j], b = v[j - 1];
                         return ids[a] == ids[b] && starts[a] == starts[b] && ends[a] == ends[b] &&
                                (!tags || tags[a] == tags[b]);
                     } };
struct DdCellPairs { const uint32_t* v; const uint32_t* cid;
                     __device__ bool same(uint32_t j) const {
                         const uint32_t a = v[j], b = v[j - 1];
                         const uint32_t a0 = cid[2 * a], a1 = cid[2 * a + 1], b0 = cid[2 * b], b1 = cid[2 * b + 1];
                         return min(a0, a1) == min(b0, b1) && max(a0, a1) == max(b0, b1);
                     } };

template <typename Cells>
__global__ __launch_bounds__(256) void k_dd_heads(Cells cells, uint32_t n_act, uint32_t* __restrict__ flag) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_act; j += gridDim.x * blockDim.x)
        flag[j] = (j == 0 || !cells.same(j)) ? 1u : 0u;
}

// E: the exclusive scan of the head flags (n_placed + 1 entries).  vals[j * stride]: the read of sorted record j.  The
// placed reads are the first n_placed records; an unplaced read gets the id `idu`.
__global__ __launch_bounds__(256) void k_dd_cell_ids(const uint32_t* __restrict__ vals, uint32_t stride,
                                                     const uint32_t* __restrict__ E, uint32_t n_placed, uint32_t n,
                                                     uint32_t idu, uint32_t* __restrict__ cid) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
        cid[vals[(size_t)j * stride]] = j < n_placed ? E[j + 1] - 1u : idu;
}

// key of sorted record j = unit idx[j] (idx == NULL: unit j) = reads (2u, 2u + 1); a mate is placed iff its id != idu
template <typename KeyT>
__global__ __launch_bounds__(256) void k_dd_pair_keys(const uint32_t* __restrict__ cid, const uint32_t* __restrict__ q,
                                                      const uint32_t* __restrict__ idx, uint32_t n_units, uint32_t idu,
                                                      uint32_t q_min, uint32_t score_max, DedupPack pack,
                                                      KeyT* __restrict__ keys) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_units; j += gridDim.x * blockDim.x) {
        const uint32_t u = idx ? idx[j] : j;
        const uint2 c = *(const uint2*)(cid + 2 * (size_t)u);
        uint32_t score = 0;
        if (q) {
            const uint32_t q0 = q[2 * (size_t)u], q1 = q[2 * (size_t)u + 1];  // (the caller's column: any alignment)
            score = (c.x != idu ? q0 - q_min : 0u) + (c.y != idu ? q1 - q_min : 0u);
        }
        uint64_t v[kDedupMaxFields] = {score_max - score, max(c.x, c.y), min(c.x, c.y), 0};
        keys[j] = (KeyT)dd_pack(pack, v);
    }
}

// E: the exclusive scan of the head flags of the n_act active records (n_act + 1 entries).  surv / dup: zeroed masks in
// input order, 32-bit words; dup may be NULL.  headpos[f] = the first record of family f, headpos[families] = n_act.
template <bool PAIRS>
__global__ __launch_bounds__(256) void k_dd_segments(const uint32_t* __restrict__ vals, uint32_t stride,
                                                     const uint32_t* __restrict__ E, uint32_t n_act,
                                                     uint32_t* __restrict__ surv, uint32_t* __restrict__ dup,
                                                     uint32_t* __restrict__ headpos) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_act; j += gridDim.x * blockDim.x) {
        const uint32_t e0 = E[j], e1 = E[j + 1];
        const bool head = e1 != e0;
        const uint32_t u = vals[(size_t)j * stride];
        // a pair's two bits lie in one 32-bit word: 2u is even
        const uint32_t word = PAIRS ? u >> 4 : u >> 5;
        const uint32_t bits = PAIRS ? 3u << ((2u * u) & 31u) : 1u << (u & 31u);
        if (head) {
            headpos[e0] = j;
            atomicOr(&surv[word], bits);
        } else if (dup) {
            atomicOr(&dup[word], bits);
        }
        if (j == n_act - 1) headpos[e1] = n_act;
    }
}

// n_fam: the scan's total.  counters (u64, zeroed): families, the units beyond the first `keep` of their family (keep
// == 1: the duplicate units), largest family, families larger than `keep`.  hist (u64, zeroed, hist_bins <= kDedupHistMax
// words): hist[k - 1] = families of size k, the last bin the sizes >= hist_bins.
__global__ __launch_bounds__(256) void k_dd_family_stats(const uint32_t* __restrict__ headpos,
                                                         const uint32_t* __restrict__ n_fam, uint32_t keep,
                                                         uint32_t hist_bins, unsigned long long* __restrict__ hist,
                                                         unsigned long long* __restrict__ counters) {
    extern __shared__ uint32_t s_bins[];
    __shared__ uint32_t s_f[4], s_d[4], s_l[4], s_o[4];
    for (uint32_t b = threadIdx.x; b < hist_bins; b += blockDim.x) s_bins[b] = 0;
    __syncthreads();
    const uint32_t F = *n_fam;
    uint32_t fam = 0, dups = 0, largest = 0, over = 0;
    for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < F; f += gridDim.x * blockDim.x) {
        const uint32_t size = headpos[f + 1] - headpos[f];
        ++fam;
        dups += size - min(size, keep);
        over += size > keep ? 1u : 0u;
        largest = max(largest, size);
        if (hist_bins) atomicAdd(&s_bins[min(size, hist_bins) - 1u], 1u);
    }
    fam = wave_sum_u32(fam);
    dups = wave_sum_u32(dups);
    largest = wave_max_u32(largest);
    over = wave_sum_u32(over);
    if ((threadIdx.x & 63) == 0) {
        s_f[threadIdx.x >> 6] = fam; s_d[threadIdx.x >> 6] = dups; s_l[threadIdx.x >> 6] = largest; s_o[threadIdx.x >> 6] = over;
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < hist_bins; b += blockDim.x)
        if (s_bins[b]) atomicAdd(&hist[b], (unsigned long long)s_bins[b]);
    if (threadIdx.x == 0) {
        fam = s_f[0] + s_f[1] + s_f[2] + s_f[3];
        dups = s_d[0] + s_d[1] + s_d[2] + s_d[3];
        largest = max(max(s_l[0], s_l[1]), max(s_l[2], s_l[3]));
        over = s_o[0] + s_o[1] + s_o[2] + s_o[3];
        if (over) atomicAdd(&counters[3], (unsigned long long)over);
        if (fam) atomicAdd(&counters[0], (unsigned long long)fam);
        if (dups) atomicAdd(&counters[1], (unsigned long long)dups);
        if (largest) atomicMax(&counters[2], (unsigned long long)largest);
    }
}

// survivor i becomes compact read word_base[i / 64] + (set bits of its word below it): input order is kept
__global__ __launch_bounds__(256) void k_dd_compact(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                    const uint32_t* __restrict__ ids, const uint64_t* __restrict__ surv,
                                                    const uint32_t* __restrict__ word_base, uint32_t n,
                                                    uint32_t* __restrict__ starts_c, uint32_t* __restrict__ ends_c,
                                                    uint32_t* __restrict__ ids_c, uint32_t* __restrict__ orig) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t word = surv[i >> 6];
        const uint32_t bit = i & 63u;
        if ((word >> bit) & 1ull) {
            const uint32_t dst = word_base[i >> 6] + (uint32_t)__popcll(word & ((1ull << bit) - 1ull));
            starts_c[dst] = starts[i];
            ends_c[dst] = ends[i];
            ids_c[dst] = ids[i];
            orig[dst] = i;
        }
    }
}

uint32_t dedup_hist_max() { return kDedupHistMax; }

void launch_dd_range(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                     const uint32_t* tags, const uint32_t* q, uint32_t n, const uint32_t* lengths, uint32_t n_contigs,
                     bool pairs, uint32_t* out) {
    if (n == 0) return;
    const bool vec = (((uintptr_t)starts | (uintptr_t)ends | (uintptr_t)ids | (uintptr_t)tags | (uintptr_t)q) & 15u) == 0;
    const dim3 grid(grid_for(((uint64_t)n + 3) / 4, 256)), block(256);
    if (vec)
        hipLaunchKernelGGL(k_dd_range<true>, grid, block, 0, st, starts, ends, ids, tags, q, n, lengths, n_contigs, pairs, out);
    else
        hipLaunchKernelGGL(k_dd_range<false>, grid, block, 0, st, starts, ends, ids, tags, q, n, lengths, n_contigs, pairs, out);
}

void launch_dd_read_keys(hipStream_t st, uint32_t key_bytes, const uint32_t* starts, const uint32_t* ends,
                         const uint32_t* ids, const uint32_t* tags, const uint32_t* q, const uint32_t* idx,
                         const uint64_t* poff, uint64_t ltot, uint32_t n, uint32_t min_span, uint32_t tag_min,
                         uint32_t q_max, const DedupPack& pack, void* keys) {
    if (n == 0) return;
    if (key_bytes == 8)
        hipLaunchKernelGGL(k_dd_read_keys<uint64_t>, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, ends, ids, tags, q,
                           idx, poff, ltot, n, min_span, tag_min, q_max, pack, (uint64_t*)keys);
    else
        hipLaunchKernelGGL(k_dd_read_keys<uint32_t>, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, ends, ids, tags, q,
                           idx, poff, ltot, n, min_span, tag_min, q_max, pack, (uint32_t*)keys);
}

void launch_dd_pair_keys(hipStream_t st, uint32_t key_bytes, const uint32_t* cid, const uint32_t* q, const uint32_t* idx,
                         uint32_t n_units, uint32_t idu, uint32_t q_min, uint32_t score_max, const DedupPack& pack,
                         void* keys) {
    if (n_units == 0) return;
    if (key_bytes == 8)
        hipLaunchKernelGGL(k_dd_pair_keys<uint64_t>, dim3(grid_for(n_units, 256)), dim3(256), 0, st, cid, q, idx, n_units,
                           idu, q_min, score_max, pack, (uint64_t*)keys);
    else
        hipLaunchKernelGGL(k_dd_pair_keys<uint32_t>, dim3(grid_for(n_units, 256)), dim3(256), 0, st, cid, q, idx, n_units,
                           idu, q_min, score_max, pack, (uint32_t*)keys);
}

void launch_dd_heads(hipStream_t st, uint32_t form, const void* sorted, const uint32_t* svals, uint32_t low_bits,
                     uint32_t n_act, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                     const uint32_t* tags, const uint32_t* cid, uint32_t* flag) {
    if (n_act == 0) return;
    const dim3 grid(grid_for(n_act, 256)), block(256);
    if (form == DEDUP_SORT_REC32)
        hipLaunchKernelGGL(k_dd_heads<DdCellRec>, grid, block, 0, st, DdCellRec{(const Rec*)sorted, low_bits}, n_act, flag);
    else if (form == DEDUP_SORT_SPLIT64)
        hipLaunchKernelGGL(k_dd_heads<DdCell64>, grid, block, 0, st, DdCell64{(const uint64_t*)sorted, low_bits}, n_act, flag);
    else if (cid)
        hipLaunchKernelGGL(k_dd_heads<DdCellPairs>, grid, block, 0, st, DdCellPairs{svals, cid}, n_act, flag);
    else
        hipLaunchKernelGGL(k_dd_heads<DdCellReads>, grid, block, 0, st, DdCellReads{svals, starts, ends, ids, tags}, n_act,
                           flag);
}

void launch_dd_cell_ids(hipStream_t st, const uint32_t* vals, uint32_t stride, const uint32_t* E, uint32_t n_placed,
                        uint32_t n, uint32_t idu, uint32_t* cid) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_dd_cell_ids, dim3(grid_for(n, 256)), dim3(256), 0, st, vals, stride, E, n_placed, n, idu, cid);
}

void launch_dd_segments(hipStream_t st, bool pairs, const uint32_t* vals, uint32_t stride, const uint32_t* E,
                        uint32_t n_act, uint64_t* surv, uint64_t* dup, uint32_t* headpos) {
    if (n_act == 0) return;
    const dim3 grid(grid_for(n_act, 256)), block(256);
    if (pairs)
        hipLaunchKernelGGL(k_dd_segments<true>, grid, block, 0, st, vals, stride, E, n_act, (uint32_t*)surv, (uint32_t*)dup,
                           headpos);
    else
        hipLaunchKernelGGL(k_dd_segments<false>, grid, block, 0, st, vals, stride, E, n_act, (uint32_t*)surv, (uint32_t*)dup,
                           headpos);
}

void launch_dd_family_stats(hipStream_t st, const uint32_t* headpos, const uint32_t* n_fam, uint32_t n_act, uint32_t keep,
                            uint32_t hist_bins, uint64_t* hist, uint64_t* counters) {
    if (n_act == 0) return;
    hipLaunchKernelGGL(k_dd_family_stats, dim3(grid_for(n_act, 256, 256)), dim3(256), (size_t)hist_bins * sizeof(uint32_t),
                       st, headpos, n_fam, keep, hist_bins, (unsigned long long*)hist, (unsigned long long*)counters);
}

void launch_dd_compact(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                       const uint64_t* surv, const uint32_t* word_base, uint32_t n, uint32_t* starts_c, uint32_t* ends_c,
                       uint32_t* ids_c, uint32_t* orig) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_dd_compact, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, ends, ids, surv, word_base, n,
                       starts_c, ends_c, ids_c, orig);
}
