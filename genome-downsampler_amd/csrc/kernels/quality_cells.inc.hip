// quality_cells.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after launchers).
// The quality pass of qmcp_hip_solve_quality_*: given the keep mask K of the plain solve, keep in every cell (the reads
// of one call that share (contig, start, end)) the same number of reads, chosen by quality descending, then read index.
//   k_qc_range    min / max quality over the placed reads (one whole-chip reduction; equal -> K is the answer)
//   k_qc_keys     composite key per read: gstart | span - min_span | q_max - q, most significant first; the stable LSD
//                 radix of radix_sort.inc.hip sorts {key, index} (32-bit keys as records, wider ones as split columns)
//   k_qc_marks    over the sorted order: K gathered per record (exclusively scanned into P), every segment's end at
//                 its last record and its start at its head (mirrored, so that the reverse min-scan of
//                 bucket_offsets.inc.hip turns both into per-record bounds)
//   k_qc_choose   a record is kept iff its rank in its segment is < P[end] - P[start]; only the bits that flip are
//                 touched, by integer atomicXor on the mask word (at most 2 x the kept reads of contested cells: one
//                 random byte store per read measured 2.3 ms at 10^8 reads)
// A segment is a run of equal (key >> q_bits): one cell.  The records of a cell arrive in (quality desc, index asc)
// order because the sort is stable and the records enter it in index order.

// range[0] = min, range[1] = max quality over reads with ids == null or ids[i] != QMCP_NO_CONTIG (host sets ~0u, 0)
__global__ __launch_bounds__(256) void k_qc_range(const uint32_t* __restrict__ q, const uint32_t* __restrict__ ids,
                                                  uint32_t n, uint32_t* __restrict__ range) {
    __shared__ uint32_t s_mn[4], s_mx[4];
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (ids && ids[i] == QMCP_NO_CONTIG) continue;
        const uint32_t v = q[i];
        mn = min(mn, v);
        mx = max(mx, v);
    }
    mn = wave_min_u32(mn);
    mx = wave_max_u32(mx);
    if ((threadIdx.x & 63) == 0) { s_mn[threadIdx.x >> 6] = mn; s_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = min(min(s_mn[0], s_mn[1]), min(s_mn[2], s_mn[3]));
        mx = max(max(s_mx[0], s_mx[1]), max(s_mx[2], s_mx[3]));
        if (mn != 0xFFFFFFFFu) atomicMin(&range[0], mn);
        if (mx != 0u) atomicMax(&range[1], mx);
    }
}

// ids != null (by-contig calls): read i lies on contig ids[i]; QMCP_NO_CONTIG reads get gstart = ltot with the span and
// quality fields 0 -- one cell of their own behind every contig, whose K count is 0.  ids == null: read i lies on the
// contig c with roff[c] <= i < roff[c + 1] (binary search over the n_contigs + 1 offsets).
template <typename KeyT>
__global__ __launch_bounds__(256) void k_qc_keys(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
                                                 const uint32_t* __restrict__ q, const uint32_t* __restrict__ ids,
                                                 const uint64_t* __restrict__ roff, const uint64_t* __restrict__ poff,
                                                 uint32_t n_contigs, uint64_t ltot, uint32_t n, uint32_t min_span,
                                                 uint32_t span_bits, uint32_t q_max, uint32_t q_bits,
                                                 KeyT* __restrict__ keys) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t cid;
        if (ids) {
            cid = ids[i];
        } else {
            uint32_t lo = 0, hi = n_contigs - 1;  // largest c with roff[c] <= i
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (roff[mid] <= i) lo = mid; else hi = mid - 1;
            }
            cid = lo;
        }
        KeyT key;
        if (cid == QMCP_NO_CONTIG) {
            key = (KeyT)ltot << (span_bits + q_bits);
        } else {
            const uint32_t s = starts[i];
            const KeyT g = (KeyT)(poff[cid] + s);
            const KeyT sp = (KeyT)(ends[i] - s + 1u - min_span);
            key = (g << (span_bits + q_bits)) | (sp << q_bits) | (KeyT)(q_max - q[i]);
        }
        keys[i] = key;
    }
}

struct QcRec { const Rec* r;
               __device__ uint64_t key(uint32_t j) const { return r[j].key; }
               __device__ uint32_t idx(uint32_t j) const { return r[j].val; } };
struct QcSplit64 { const uint64_t* k; const uint32_t* v;
                   __device__ uint64_t key(uint32_t j) const { return k[j]; }
                   __device__ uint32_t idx(uint32_t j) const { return v[j]; } };

// kb[j] = K bit of sorted record j (scanned in place afterwards); seg_end[j] = j + 1 at a segment's last record, ~0u
// elsewhere; seg_head_rev[n - 1 - j] = n - 1 - j at a segment's first record, ~0u elsewhere.
template <typename Keys>
__global__ __launch_bounds__(256) void k_qc_marks(Keys keys, uint32_t n, uint32_t q_bits,
                                                  const uint64_t* __restrict__ mask, uint32_t* __restrict__ kb,
                                                  uint32_t* __restrict__ seg_end, uint32_t* __restrict__ seg_head_rev) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const uint64_t cell = keys.key(j) >> q_bits;
        const uint32_t i = keys.idx(j);
        const bool head = j == 0 || (keys.key(j - 1) >> q_bits) != cell;
        const bool last = j == n - 1 || (keys.key(j + 1) >> q_bits) != cell;
        kb[j] = (uint32_t)(mask[i >> 6] >> (i & 63)) & 1u;
        seg_end[j] = last ? j + 1 : 0xFFFFFFFFu;
        seg_head_rev[n - 1 - j] = head ? n - 1 - j : 0xFFFFFFFFu;
    }
}

// after the scans: P = exclusive prefix of the K bits (n + 1 entries), seg_end[j] = end of j's segment,
// seg_head_rev[n - 1 - j] = n - 1 - (start of j's segment).  counters[0] += contested cells (0 < c < size),
// counters[1] += reads that left the kept set.  The mask's other bits (past n_reads too) are left as they are.
template <typename Keys>
__global__ __launch_bounds__(256) void k_qc_choose(Keys keys, uint32_t n, const uint32_t* __restrict__ P,
                                                   const uint32_t* __restrict__ seg_end,
                                                   const uint32_t* __restrict__ seg_head_rev,
                                                   unsigned long long* __restrict__ mask,
                                                   unsigned long long* __restrict__ counters) {
    __shared__ uint32_t s_c[4], s_s[4];
    uint32_t contested = 0, swapped = 0;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const uint32_t e = seg_end[j];
        const uint32_t s = n - 1 - seg_head_rev[n - 1 - j];
        const uint32_t c = P[e] - P[s];
        const bool keep = j - s < c;
        const bool was = P[j + 1] != P[j];
        if (keep != was) {
            const uint32_t i = keys.idx(j);
            atomicXor(&mask[i >> 6], 1ull << (i & 63));
        }
        swapped += (was && !keep) ? 1u : 0u;
        contested += (j == s && c != 0 && c < e - s) ? 1u : 0u;
    }
    contested = wave_sum_u32(contested);
    swapped = wave_sum_u32(swapped);
    if ((threadIdx.x & 63) == 0) { s_c[threadIdx.x >> 6] = contested; s_s[threadIdx.x >> 6] = swapped; }
    __syncthreads();
    if (threadIdx.x == 0) {
        contested = s_c[0] + s_c[1] + s_c[2] + s_c[3];
        swapped = s_s[0] + s_s[1] + s_s[2] + s_s[3];
        if (contested) atomicAdd(&counters[0], (unsigned long long)contested);
        if (swapped) atomicAdd(&counters[1], (unsigned long long)swapped);
    }
}

void launch_qc_range(hipStream_t st, const uint32_t* q, const uint32_t* ids, uint32_t n, uint32_t* range) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_qc_range, dim3(grid_for(n, 256)), dim3(256), 0, st, q, ids, n, range);
}

void launch_qc_keys(hipStream_t st, bool wide, const uint32_t* starts, const uint32_t* ends, const uint32_t* q,
                    const uint32_t* ids, const uint64_t* roff, const uint64_t* poff, uint32_t n_contigs, uint64_t ltot,
                    uint32_t n, uint32_t min_span, uint32_t span_bits, uint32_t q_max, uint32_t q_bits, void* keys) {
    if (n == 0) return;
    if (wide)
        hipLaunchKernelGGL(k_qc_keys<uint64_t>, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, ends, q, ids, roff,
                           poff, n_contigs, ltot, n, min_span, span_bits, q_max, q_bits, (uint64_t*)keys);
    else
        hipLaunchKernelGGL(k_qc_keys<uint32_t>, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, ends, q, ids, roff,
                           poff, n_contigs, ltot, n, min_span, span_bits, q_max, q_bits, (uint32_t*)keys);
}

void launch_qc_marks(hipStream_t st, bool wide, const void* sorted, const uint32_t* svals, uint32_t n, uint32_t q_bits,
                     const uint64_t* mask, uint32_t* kb, uint32_t* seg_end, uint32_t* seg_head_rev) {
    if (n == 0) return;
    if (wide)
        hipLaunchKernelGGL(k_qc_marks<QcSplit64>, dim3(grid_for(n, 256)), dim3(256), 0, st,
                           QcSplit64{(const uint64_t*)sorted, svals}, n, q_bits, mask, kb, seg_end, seg_head_rev);
    else
        hipLaunchKernelGGL(k_qc_marks<QcRec>, dim3(grid_for(n, 256)), dim3(256), 0, st, QcRec{(const Rec*)sorted}, n,
                           q_bits, mask, kb, seg_end, seg_head_rev);
}

void launch_qc_choose(hipStream_t st, bool wide, const void* sorted, const uint32_t* svals, uint32_t n,
                      const uint32_t* P, const uint32_t* seg_end, const uint32_t* seg_head_rev, uint64_t* mask,
                      unsigned long long* counters) {
    if (n == 0) return;
    if (wide)
        hipLaunchKernelGGL(k_qc_choose<QcSplit64>, dim3(grid_for(n, 256)), dim3(256), 0, st,
                           QcSplit64{(const uint64_t*)sorted, svals}, n, P, seg_end, seg_head_rev, (unsigned long long*)mask, counters);
    else
        hipLaunchKernelGGL(k_qc_choose<QcRec>, dim3(grid_for(n, 256)), dim3(256), 0, st, QcRec{(const Rec*)sorted}, n,
                           P, seg_end, seg_head_rev, (unsigned long long*)mask, counters);
}
