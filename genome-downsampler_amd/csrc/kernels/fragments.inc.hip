// fragments.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after templates).
// Fragment depth (qmcp_hip_clip_templates_*, qmcp_hip_solve_fragments_*): the placed segments of every (template, contig)
// group are clipped against the largest end among the group's earlier members, in the order (start, input index), so
// that a template covers a position at most once.
//   k_frag_check   once per call, input order: err |= 1 for a contig id that is neither < n_contigs nor QMCP_NO_CONTIG,
//                  err |= 2 for a placed row with start > end or end >= its contig's length; the placed rows and their
//                  bases (per wave, then one atomic per workgroup and count)
//   k_frag_keys    the round's u64 key of every row: start | contig << | template << as fragment_plan.h lays them out.
//                  An unplaced row takes contig 0 and start 0: it sorts into a group of its template and counts for
//                  nothing there (valid = 0 below)
//   -- radix_sort_wide (radix_sort.inc.hip) on those keys; its value column is the rows' input index in sorted order --
//   k_frag_tiles   a workgroup per tile of kFragTile sorted rows: the tile's aggregate under the operator below
//   k_frag_spine   one workgroup: the exclusive scan of the tiles' aggregates, kFragTile of them at a time
//   k_frag_apply   the tile scan again with the tile's carry: every row gets `reach`, the largest end among the earlier
//                  placed members of its group, or "none"; start' and the contig id go back to INPUT order through the
//                  sorted index; the statistics per wave, LDS across the four waves, one atomic per workgroup
// THE OPERATOR.  An element is (head, cnt, val): head = its (template, contig) differs from the row before it in sorted
// order, cnt = 1 for a placed row (valid) and 0 for an unplaced one, val = its end.  join(a, b) = b when b.head, else
// (a.head, a.cnt + b.cnt, max of the vals whose cnt is not 0): the segmented running maximum, with the segment's placed
// rows counted beside it.  It is associative with identity (0, 0, 0).  "No earlier member" is cnt == 0, never a value of
// val: an end of 2^32 - 2 (or 2^32 - 1) is carried as it is.  reach(j) is the EXCLUSIVE scan at j when j is no head.
// No atomics in the scan and no dependence on workgroup order: tiles -> spine -> apply are three launches.  The only
// atomics are the statistics' (commutative sums, a maximum, bits of the tp_flags bitset).  No inline assembly.
// Bounds: every index into the columns is idx[j] with j < n, and idx is a permutation of 0 .. n - 1 (the sort's value
// column); lengths[] is read only behind id < n_contigs; agg / carry hold n_tiles entries each.

static constexpr int kFragThreads = 256;
static constexpr int kFragItems = 4;
static constexpr uint32_t kFragTile = kFragThreads * kFragItems;  // 1024 rows: wave w owns rows [256 w, 256 w + 256)

struct FragSeg {
    uint32_t val, cnt, head;
};

__device__ __forceinline__ FragSeg frag_join(const FragSeg& a, const FragSeg& b) {
    if (b.head) return b;
    FragSeg r;
    r.head = a.head;
    r.cnt = a.cnt + b.cnt;
    r.val = a.cnt == 0u ? b.val : (b.cnt == 0u ? a.val : max(a.val, b.val));
    return r;
}

__device__ __forceinline__ FragSeg frag_shfl_up(const FragSeg& x, int o) {
    FragSeg t;
    t.val = (uint32_t)__shfl_up((int)x.val, o, kWave);
    t.cnt = (uint32_t)__shfl_up((int)x.cnt, o, kWave);
    t.head = (uint32_t)__shfl_up((int)x.head, o, kWave);
    return t;
}

__device__ __forceinline__ FragSeg frag_wave_incl_scan(FragSeg x, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const FragSeg t = frag_shfl_up(x, o);
        if (lane >= (uint32_t)o) x = frag_join(t, x);
    }
    return x;
}

// The tile's exclusive scan.  x[k] of lane l in wave w is the tile's element 256 w + 64 k + l; on return it is
// join(carry_in, every element of the tile before it).  Returns the join of the whole tile (without carry_in), the same
// in every thread.  s_wave: four entries of LDS, free again on return.
__device__ __forceinline__ FragSeg frag_block_excl_scan(FragSeg (&x)[kFragItems], const FragSeg& carry_in,
                                                        FragSeg* s_wave) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const FragSeg none = {0u, 0u, 0u};
    FragSeg run = none;  // the wave's rows before row k
#pragma unroll
    for (int k = 0; k < kFragItems; ++k) {
        const FragSeg inc = frag_wave_incl_scan(x[k], lane);
        FragSeg before = frag_shfl_up(inc, 1);
        if (lane == 0) before = none;
        x[k] = frag_join(run, before);
        FragSeg last;
        last.val = (uint32_t)__shfl((int)inc.val, kWave - 1, kWave);
        last.cnt = (uint32_t)__shfl((int)inc.cnt, kWave - 1, kWave);
        last.head = (uint32_t)__shfl((int)inc.head, kWave - 1, kWave);
        run = frag_join(run, last);
    }
    if (lane == 0) s_wave[w] = run;
    __syncthreads();
    FragSeg before = carry_in, total = none;
#pragma unroll
    for (uint32_t ww = 0; ww < (uint32_t)(kFragThreads / kWave); ++ww) {
        const FragSeg a = s_wave[ww];
        if (ww < w) before = frag_join(before, a);
        total = frag_join(total, a);
    }
#pragma unroll
    for (int k = 0; k < kFragItems; ++k) x[k] = frag_join(before, x[k]);
    __syncthreads();
    return total;
}

// sorted row j: its input index, template, contig and, when placed, its end; head from the row before it
struct FragRow {
    uint32_t i, tid, cid;
    bool live;
};
__device__ __forceinline__ FragSeg frag_load(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ ends,
                                             const uint32_t* __restrict__ cids, const uint32_t* __restrict__ tids,
                                             uint32_t n, uint32_t j, FragRow& r) {
    FragSeg s = {0u, 0u, 0u};
    r.live = j < n;
    r.i = 0;
    r.tid = 0;
    r.cid = QMCP_NO_CONTIG;
    if (!r.live) return s;
    r.i = idx[j];
    r.tid = tids[r.i];
    r.cid = cids[r.i];
    const bool placed = r.cid != QMCP_NO_CONTIG;
    s.head = 1u;
    if (j > 0) {
        const uint32_t ip = idx[j - 1];
        const uint32_t cp = cids[ip];
        s.head = (tids[ip] != r.tid || (cp == QMCP_NO_CONTIG ? 0u : cp) != (placed ? r.cid : 0u)) ? 1u : 0u;
    }
    s.cnt = placed ? 1u : 0u;
    s.val = placed ? ends[r.i] : 0u;
    return s;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, kWave);
    return v;
}

__global__ __launch_bounds__(256) void k_frag_check(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                    const uint32_t* __restrict__ cids, uint32_t n,
                                                    const uint32_t* __restrict__ lengths, uint32_t n_contigs,
                                                    unsigned long long* __restrict__ fstat) {
    __shared__ unsigned long long s_acc[3];
    if (threadIdx.x < 3) s_acc[threadIdx.x] = 0;
    __syncthreads();
    uint32_t err = 0, placed = 0;  // (a thread sees fewer than 2^32 rows)
    unsigned long long bases = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t id = cids[i];
        if (id == QMCP_NO_CONTIG) continue;
        if (id >= n_contigs) {
            err |= 1u;
            continue;
        }
        const uint32_t s = starts[i], e = ends[i];
        if (s > e || e >= lengths[id]) {
            err |= 2u;
            continue;
        }
        placed += 1u;
        bases += (unsigned long long)(e - s) + 1ull;
    }
    const uint32_t lane = threadIdx.x & 63u;
    placed = wave_sum_u32(placed);
    bases = wave_sum_u64(bases);
    const uint32_t e1 = __ballot(err & 1u) != 0ull ? 1u : 0u, e2 = __ballot(err & 2u) != 0ull ? 2u : 0u;
    if (lane == 0) {
        if (placed) atomicAdd(&s_acc[0], (unsigned long long)placed);
        if (bases) atomicAdd(&s_acc[1], bases);
        if (e1 | e2) atomicOr(&s_acc[2], (unsigned long long)(e1 | e2));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_acc[0]) atomicAdd(&fstat[kFragPlaced], s_acc[0]);
        if (s_acc[1]) atomicAdd(&fstat[kFragBasesIn], s_acc[1]);
        if (s_acc[2]) atomicOr(&fstat[kFragErr], s_acc[2]);
    }
}

// idx == nullptr: row j is input row j (the first round); otherwise the order the rounds before it left
__global__ __launch_bounds__(256) void k_frag_keys(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ cids,
                                                   const uint32_t* __restrict__ tids, const uint32_t* __restrict__ idx,
                                                   uint32_t n, uint32_t start_bits, uint32_t contig_bits,
                                                   uint32_t template_bits, uint64_t* __restrict__ keys) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const uint32_t i = idx ? idx[j] : j;
        const uint32_t id = cids[i];
        const bool placed = id != QMCP_NO_CONTIG;
        uint64_t key = 0;
        uint32_t at = 0;
        if (start_bits) {
            key = placed ? starts[i] : 0u;
            at = start_bits;
        }
        if (contig_bits) {
            key |= (uint64_t)(placed ? id : 0u) << at;
            at += contig_bits;
        }
        if (template_bits) key |= (uint64_t)tids[i] << at;  // (at <= 56: the fields of a round fit 64 bits)
        keys[j] = key;
    }
}

__global__ __launch_bounds__(kFragThreads) void k_frag_tiles(const uint32_t* __restrict__ idx,
                                                              const uint32_t* __restrict__ ends,
                                                              const uint32_t* __restrict__ cids,
                                                              const uint32_t* __restrict__ tids, uint32_t n,
                                                              FragSeg* __restrict__ agg) {
    __shared__ FragSeg s_wave[kFragThreads / kWave];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kFragTile + w * (kFragItems * 64u);
    FragSeg x[kFragItems];
    FragRow row;
#pragma unroll
    for (int k = 0; k < kFragItems; ++k) {
        const uint64_t j = base + (uint32_t)k * 64u + lane;
        x[k] = frag_load(idx, ends, cids, tids, n, j < n ? (uint32_t)j : n, row);
    }
    const FragSeg none = {0u, 0u, 0u};
    const FragSeg total = frag_block_excl_scan(x, none, s_wave);
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

__global__ __launch_bounds__(kFragThreads) void k_frag_spine(const FragSeg* __restrict__ agg, uint32_t n_tiles,
                                                              FragSeg* __restrict__ carry) {
    __shared__ FragSeg s_wave[kFragThreads / kWave];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const FragSeg none = {0u, 0u, 0u};
    FragSeg run = none;
    for (uint32_t base = 0; base < n_tiles; base += kFragTile) {  // (n_tiles <= 2^21: base never wraps)
        FragSeg x[kFragItems];
#pragma unroll
        for (int k = 0; k < kFragItems; ++k) {
            const uint32_t t = base + w * (kFragItems * 64u) + (uint32_t)k * 64u + lane;
            x[k] = t < n_tiles ? agg[t] : none;
        }
        const FragSeg total = frag_block_excl_scan(x, run, s_wave);
#pragma unroll
        for (int k = 0; k < kFragItems; ++k) {
            const uint32_t t = base + w * (kFragItems * 64u) + (uint32_t)k * 64u + lane;
            if (t < n_tiles) carry[t] = x[k];
        }
        run = frag_join(run, total);
    }
}

__global__ __launch_bounds__(kFragThreads) void k_frag_apply(const uint32_t* __restrict__ idx,
                                                              const uint32_t* __restrict__ starts,
                                                              const uint32_t* __restrict__ ends,
                                                              const uint32_t* __restrict__ cids,
                                                              const uint32_t* __restrict__ tids, uint32_t n,
                                                              uint32_t n_templates, const FragSeg* __restrict__ carry,
                                                              uint32_t* __restrict__ starts_out,
                                                              uint32_t* __restrict__ cids_out,
                                                              uint32_t* __restrict__ tflags,
                                                              unsigned long long* __restrict__ fstat) {
    __shared__ FragSeg s_wave[kFragThreads / kWave];
    __shared__ unsigned long long s_removed;
    __shared__ uint32_t s_cnt[3];  // clipped, emptied, largest group
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x == 3) s_removed = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kFragTile + w * (kFragItems * 64u);
    FragSeg x[kFragItems];
    FragRow row[kFragItems];
    uint32_t own[kFragItems];  // bit 0 head, bit 1 placed
#pragma unroll
    for (int k = 0; k < kFragItems; ++k) {
        const uint64_t j = base + (uint32_t)k * 64u + lane;
        x[k] = frag_load(idx, ends, cids, tids, n, j < n ? (uint32_t)j : n, row[k]);
        own[k] = x[k].head | (x[k].cnt << 1);
    }
    frag_block_excl_scan(x, carry[blockIdx.x], s_wave);
    uint32_t n_clip = 0, n_empty = 0, group = 0;
    unsigned long long removed = 0;
#pragma unroll
    for (int k = 0; k < kFragItems; ++k) {
        if (!row[k].live) continue;
        const uint32_t i = row[k].i;
        const bool head = (own[k] & 1u) != 0, placed = (own[k] & 2u) != 0;
        const uint32_t earlier = head ? 0u : x[k].cnt;  // placed members of the group before this row
        uint32_t s = starts[i], id = row[k].cid;
        if (placed) {
            group = max(group, earlier + 1u);
            if (earlier) {
                const uint32_t reach = x[k].val, e = ends[i];
                const bool changed = s <= reach;
                if (e <= reach) {
                    removed += (unsigned long long)(e - s) + 1ull;
                    id = QMCP_NO_CONTIG;
                    n_empty += 1u;
                } else if (s <= reach) {  // reach < e: reach + 1 does not wrap
                    removed += (unsigned long long)(reach - s) + 1ull;
                    s = reach + 1u;
                    n_clip += 1u;
                }
                if (changed && row[k].tid < n_templates)  // (ids were checked; the bound keeps a bad one from writing)
                    atomicOr(&tflags[row[k].tid >> 5], 1u << (row[k].tid & 31u));
            }
        }
        starts_out[i] = s;
        cids_out[i] = id;
    }
    n_clip = wave_sum_u32(n_clip);
    n_empty = wave_sum_u32(n_empty);
    group = wave_max_u32(group);
    removed = wave_sum_u64(removed);
    if (lane == 0) {
        if (n_clip) atomicAdd(&s_cnt[0], n_clip);
        if (n_empty) atomicAdd(&s_cnt[1], n_empty);
        if (group) atomicMax(&s_cnt[2], group);
        if (removed) atomicAdd(&s_removed, removed);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_cnt[0]) atomicAdd(&fstat[kFragClipped], (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&fstat[kFragEmptied], (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicMax(&fstat[kFragMaxGroup], (unsigned long long)s_cnt[2]);
        if (s_removed) atomicAdd(&fstat[kFragRemoved], s_removed);
    }
}

uint32_t frag_tile_rows() { return kFragTile; }
uint32_t frag_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kFragTile - 1) / kFragTile); }
size_t frag_spine_bytes(uint32_t n) { return (size_t)2 * (frag_tiles(n) ? frag_tiles(n) : 1u) * sizeof(FragSeg); }

void launch_frag_check(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* cids, uint32_t n,
                       const uint32_t* lengths, uint32_t n_contigs, unsigned long long* fstat) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_frag_check, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, ends, cids, n, lengths, n_contigs,
                       fstat);
}

void launch_frag_keys(hipStream_t st, const uint32_t* starts, const uint32_t* cids, const uint32_t* tids, const uint32_t* idx,
                      uint32_t n, uint32_t start_bytes, uint32_t contig_bytes, uint32_t template_bytes, void* keys) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_frag_keys, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, cids, tids, idx, n, 8u * start_bytes,
                       8u * contig_bytes, 8u * template_bytes, (uint64_t*)keys);
}

void launch_frag_scan_apply(hipStream_t st, const uint32_t* idx, const uint32_t* starts, const uint32_t* ends,
                            const uint32_t* cids, const uint32_t* tids, uint32_t n, uint32_t n_templates, void* spine,
                            uint32_t* starts_out, uint32_t* cids_out, uint32_t* tflags, unsigned long long* fstat) {
    if (n == 0) return;
    const uint32_t n_tiles = frag_tiles(n);
    FragSeg* agg = (FragSeg*)spine;
    FragSeg* carry = agg + n_tiles;
    hipLaunchKernelGGL(k_frag_tiles, dim3(n_tiles), dim3(kFragThreads), 0, st, idx, ends, cids, tids, n, agg);
    hipLaunchKernelGGL(k_frag_spine, dim3(1), dim3(kFragThreads), 0, st, (const FragSeg*)agg, n_tiles, carry);
    hipLaunchKernelGGL(k_frag_apply, dim3(n_tiles), dim3(kFragThreads), 0, st, idx, starts, ends, cids, tids, n, n_templates,
                       (const FragSeg*)carry, starts_out, cids_out, tflags, fstat);
}
