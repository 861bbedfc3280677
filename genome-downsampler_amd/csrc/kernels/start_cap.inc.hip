// start_cap.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after dedup).
// Start cap (qmcp_hip_solve_start_cap_*): every (contig, start, group) cell is reduced to its best K reads before the
// by-contig solve.  dedup_plan.h packs the keys; api/start_cap.inc.hip drives the kernels.  The range pass (k_dd_range
// with the groups as tags and the priorities as qualities), the head flags on packed keys (k_dd_heads), the cell
// statistics (k_dd_family_stats with the cap) and the compaction (k_dd_compact) are dedup's; the cap's own are:
//   k_sc_keys        a round's key of read idx[j] (round 0: read j) from the fields {span_max - span, prio_max - prio,
//                    group - group_min, gstart}, packed as the round's DedupPack says
//   ScCellReads      the head comparator after a sort field by field: contig, start and group -- never the end
//   k_sc_heads       every cell's first sorted position from the scanned head flags
//   k_sc_rank        rank = j - headpos[cell(j)]: the survivor bit below K, the capped bit from K on (32-bit atomicOr,
//                    only set bits touched)
//   k_sc_kept_cells  over the sorted records, with the final mask: the kept members per cell, the cells with one and the
//                    largest count
// Every kernel is a grid-stride loop of 256 threads (four waves of 64) that moves bytes and nothing else.

// key of sorted record j = read idx[j] (idx == NULL: read j); groups / prio may be NULL (every value 0)
template <typename KeyT>
__global__ __launch_bounds__(256) void k_sc_keys(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                 const uint32_t* __restrict__ ids, const uint32_t* __restrict__ groups,
                                                 const uint32_t* __restrict__ prio, const uint32_t* __restrict__ idx,
                                                 const uint64_t* __restrict__ poff, uint64_t ltot, uint32_t n,
                                                 uint32_t span_max, uint32_t prio_max, uint32_t group_min, DedupPack pack,
                                                 KeyT* __restrict__ keys) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const uint32_t i = idx ? idx[j] : j;
        const uint32_t cid = ids[i];
        uint64_t v[kDedupMaxFields] = {0, 0, 0, ltot};
        if (cid != QMCP_NO_CONTIG) {
            const uint32_t s = starts[i];
            v[0] = span_max - (ends[i] - s);
            v[1] = prio ? prio_max - prio[i] : 0u;
            v[2] = groups ? groups[i] - group_min : 0u;
            v[3] = poff[cid] + s;
        }
        keys[j] = (KeyT)dd_pack(pack, v);
    }
}

struct ScCellReads { const uint32_t* v; const uint32_t* starts; const uint32_t* ids; const uint32_t* groups;
                     __device__ bool same(uint32_t j) const {
                         const uint32_t a = v[j], b = v[j - 1];
                         return ids[a] == ids[b] && starts[a] == starts[b] && (!groups || groups[a] == groups[b]);
                     } };

// E: the exclusive scan of the head flags of the n_act placed records (n_act + 1 entries).  headpos[f] = the first record
// of cell f, headpos[cells] = n_act.
__global__ __launch_bounds__(256) void k_sc_heads(const uint32_t* __restrict__ E, uint32_t n_act,
                                                  uint32_t* __restrict__ headpos) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_act; j += gridDim.x * blockDim.x) {
        const uint32_t e0 = E[j], e1 = E[j + 1];
        if (e1 != e0) headpos[e0] = j;
        if (j == n_act - 1) headpos[e1] = n_act;
    }
}

// vals[j * stride]: the read of sorted record j.  surv / capped: zeroed masks in input order, 32-bit words; capped may
// be NULL.
__global__ __launch_bounds__(256) void k_sc_rank(const uint32_t* __restrict__ vals, uint32_t stride,
                                                 const uint32_t* __restrict__ E, const uint32_t* __restrict__ headpos,
                                                 uint32_t n_act, uint32_t cap, uint32_t* __restrict__ surv,
                                                 uint32_t* __restrict__ capped) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_act; j += gridDim.x * blockDim.x) {
        const uint32_t rank = j - headpos[E[j + 1] - 1u];
        const uint32_t u = vals[(size_t)j * stride];
        if (rank < cap)
            atomicOr(&surv[u >> 5], 1u << (u & 31u));
        else if (capped)
            atomicOr(&capped[u >> 5], 1u << (u & 31u));
    }
}

// mask: the final keep mask in input order.  cnt (u32, zeroed, one word per cell): the kept members.  counters (u64,
// zeroed): [0] the cells with a kept member, [1] the largest count.  The first arrival at a cell counts the cell, and the
// largest value any arrival leaves is the largest count: both are the same whatever the order of the atomics.
__global__ __launch_bounds__(256) void k_sc_kept_cells(const uint32_t* __restrict__ vals, uint32_t stride,
                                                       const uint32_t* __restrict__ E, uint32_t n_act,
                                                       const uint64_t* __restrict__ mask, uint32_t* __restrict__ cnt,
                                                       unsigned long long* __restrict__ counters) {
    __shared__ uint32_t s_c[4], s_l[4];
    uint32_t cells = 0, largest = 0;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_act; j += gridDim.x * blockDim.x) {
        const uint32_t u = vals[(size_t)j * stride];
        if ((mask[u >> 6] >> (u & 63u)) & 1ull) {
            const uint32_t before = atomicAdd(&cnt[E[j + 1] - 1u], 1u);
            cells += before == 0u ? 1u : 0u;
            largest = max(largest, before + 1u);
        }
    }
    cells = wave_sum_u32(cells);
    largest = wave_max_u32(largest);
    if ((threadIdx.x & 63) == 0) { s_c[threadIdx.x >> 6] = cells; s_l[threadIdx.x >> 6] = largest; }
    __syncthreads();
    if (threadIdx.x == 0) {
        cells = s_c[0] + s_c[1] + s_c[2] + s_c[3];
        largest = max(max(s_l[0], s_l[1]), max(s_l[2], s_l[3]));
        if (cells) atomicAdd(&counters[0], (unsigned long long)cells);
        if (largest) atomicMax(&counters[1], (unsigned long long)largest);
    }
}

void launch_sc_keys(hipStream_t st, uint32_t key_bytes, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                    const uint32_t* groups, const uint32_t* prio, const uint32_t* idx, const uint64_t* poff, uint64_t ltot,
                    uint32_t n, uint32_t span_max, uint32_t prio_max, uint32_t group_min, const DedupPack& pack,
                    void* keys) {
    if (n == 0) return;
    if (key_bytes == 8)
        hipLaunchKernelGGL(k_sc_keys<uint64_t>, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, ends, ids, groups, prio,
                           idx, poff, ltot, n, span_max, prio_max, group_min, pack, (uint64_t*)keys);
    else
        hipLaunchKernelGGL(k_sc_keys<uint32_t>, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, ends, ids, groups, prio,
                           idx, poff, ltot, n, span_max, prio_max, group_min, pack, (uint32_t*)keys);
}

void launch_sc_cell_flags(hipStream_t st, uint32_t form, const void* sorted, const uint32_t* svals, uint32_t low_bits,
                          uint32_t n_act, const uint32_t* starts, const uint32_t* ids, const uint32_t* groups,
                          uint32_t* flag) {
    if (n_act == 0) return;
    if (form != DEDUP_SORT_FIELDS) {
        launch_dd_heads(st, form, sorted, svals, low_bits, n_act, nullptr, nullptr, nullptr, nullptr, nullptr, flag);
        return;
    }
    hipLaunchKernelGGL(k_dd_heads<ScCellReads>, dim3(grid_for(n_act, 256)), dim3(256), 0, st,
                       ScCellReads{svals, starts, ids, groups}, n_act, flag);
}

void launch_sc_heads(hipStream_t st, const uint32_t* E, uint32_t n_act, uint32_t* headpos) {
    if (n_act == 0) return;
    hipLaunchKernelGGL(k_sc_heads, dim3(grid_for(n_act, 256)), dim3(256), 0, st, E, n_act, headpos);
}

void launch_sc_rank(hipStream_t st, const uint32_t* vals, uint32_t stride, const uint32_t* E, const uint32_t* headpos,
                    uint32_t n_act, uint32_t cap, uint64_t* surv, uint64_t* capped) {
    if (n_act == 0) return;
    hipLaunchKernelGGL(k_sc_rank, dim3(grid_for(n_act, 256)), dim3(256), 0, st, vals, stride, E, headpos, n_act, cap,
                       (uint32_t*)surv, (uint32_t*)capped);
}

void launch_sc_kept_cells(hipStream_t st, const uint32_t* vals, uint32_t stride, const uint32_t* E, uint32_t n_act,
                          const uint64_t* mask, uint32_t* cnt, uint64_t* counters) {
    if (n_act == 0) return;
    hipLaunchKernelGGL(k_sc_kept_cells, dim3(grid_for(n_act, 256)), dim3(256), 0, st, vals, stride, E, n_act, mask, cnt,
                       (unsigned long long*)counters);
}
