// depth_report.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after launchers).
// qmcp_hip_depth_report_*: depth before and after a keep mask, summarised per contig and per region, never written per
// position.  One position batch (whole contigs, at most 2^31 - 2 positions, concatenated on one axis of P positions):
//   k_depth_events       one pass over the reads: validation as k_bc_keys, and for every placed read of the batch's contigs
//                        +w at ev[start] and -w at ev[end + 1], w = 1 + 2^32 * kept, as two 64-bit no-return atomics.  The
//                        words are sums modulo 2^64 of a + 2^32 b (a the net count of all reads, b of the kept ones, both
//                        within (-2^31, 2^31)), so a = low word and b = high word + the low word's sign bit whatever order
//                        the atomics arrived in: from there on two independent 32-bit channels.
//   k_depth_chunk_sums   the axis is cut into at most 2 048 chunks of whole tiles (1 024 positions); a workgroup per chunk
//                        sums both channels of its chunk
//   k_depth_spine        one workgroup: exclusive scan of the chunk sums
//   k_depth_consume      a workgroup per chunk walks its tiles carrying the two running sums; a thread owns four
//                        consecutive positions (two 16-byte loads), DPP wave scans give cov and kept per position in
//                        registers.  From them the LDS histograms (one copy per workgroup, flushed once with 64-bit
//                        atomics, non-zero bins only) and the rows: position -> row is monotone for both interval tables
//                        (contigs, merged regions), a thread follows its interval index from a binary search inside the
//                        chunk's range of intervals, and a wave reduces runs of equal rows by a segmented shuffle
//                        reduction, so global accumulators are touched at run heads only.
// Nothing here indexes beyond P: ev has P + 1 words, a valid read has start <= end < its contig's length.

constexpr uint32_t kDepthLdsContigs = 2048;  // contig lengths and offsets staged in LDS (2 x 2 048 words = 16 KiB)
constexpr uint32_t kDepthTile = 1024;        // positions per tile: 256 threads x 4
constexpr uint32_t kDepthMaxChunks = 2048;
constexpr uint32_t kDepthNoRow = 0xFFFFFFFFu;

// kTab: 1 lengths and offsets in LDS (n_contigs <= kDepthLdsContigs), 2 read through L2.  kVec: the three columns are
// 16-byte aligned and a lane loads four consecutive reads of each with one 128-bit load (k_target_project's forms).
// lengths: every contig's; boff: the batch-local position offset of the contigs [c0, c1) (other entries unused).
// counts[0] += placed reads of the batch's contigs, counts[1] += those kept.  mask == NULL: every placed read is kept.
template <int kTab, bool kVec>
__global__ __launch_bounds__(256) void k_depth_events(
    const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends, const uint32_t* __restrict__ ids, uint32_t n,
    const uint64_t* __restrict__ mask, const uint32_t* __restrict__ g_len, const uint32_t* __restrict__ g_boff,
    uint32_t n_contigs, uint32_t c0, uint32_t c1, unsigned long long* __restrict__ ev,
    unsigned long long* __restrict__ counts, uint32_t* __restrict__ err) {
    extern __shared__ uint32_t s_tab[];  // kTab == 1: [n_contigs lengths | n_contigs offsets]
    const uint32_t* len = g_len;
    const uint32_t* boff = g_boff;
    if constexpr (kTab == 1) {
        for (uint32_t i = threadIdx.x; i < n_contigs; i += blockDim.x) {
            s_tab[i] = g_len[i];
            s_tab[n_contigs + i] = g_boff[i];
        }
        __syncthreads();
        len = s_tab;
        boff = s_tab + n_contigs;
    }
    const uint32_t n_chunks = (n + 255u) / 256u;
    const uint32_t wave_global = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t bad = 0, placed = 0, kept_n = 0;
    for (uint32_t ch = wave_global; ch < n_chunks; ch += n_waves) {
        const uint64_t base = (uint64_t)ch * 256u;
        uint32_t s4[4], e4[4], id4[4];
        uint64_t i4[4];
        if constexpr (kVec) {
            const uint64_t i0 = base + 4u * lane;
#pragma unroll
            for (int r = 0; r < 4; ++r) i4[r] = i0 + r;
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
                i4[r] = i;
                s4[r] = in ? starts[i] : 0u;
                e4[r] = in ? ends[i] : 0u;
                id4[r] = in ? ids[i] : QMCP_NO_CONTIG;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t id = id4[r];
            if (id >= n_contigs) {
                if (id != QMCP_NO_CONTIG) bad |= 1u;
                continue;
            }
            if (s4[r] > e4[r] || e4[r] >= len[id]) {
                bad |= 2u;
                continue;
            }
            if (id < c0 || id >= c1) continue;  // another position batch's read
            const uint64_t k = mask ? (mask[i4[r] >> 6] >> (i4[r] & 63u)) & 1ull : 1ull;
            const unsigned long long w = 1ull | (k << 32);
            const uint32_t g = boff[id];
            atomicAdd(&ev[g + s4[r]], w);
            atomicAdd(&ev[g + e4[r] + 1u], 0ull - w);
            placed++;
            kept_n += (uint32_t)k;
        }
    }
    placed = wave_sum_u32(placed);
    kept_n = wave_sum_u32(kept_n);
    if (lane == 0) {
        if (placed) atomicAdd(&counts[0], (unsigned long long)placed);
        if (kept_n) atomicAdd(&counts[1], (unsigned long long)kept_n);
    }
    if (bad) atomicOr(err, bad);
}

// the two channels of one event word (see the head of this file)
__device__ __forceinline__ void depth_decode(unsigned long long w, uint32_t& a, uint32_t& b) {
    a = (uint32_t)w;
    b = (uint32_t)(w >> 32) + (a >> 31);
}

// four consecutive event words of thread-owned positions p0 .. p0 + 3 (p0 a multiple of 4; words at or beyond P read 0)
__device__ __forceinline__ void depth_load4(const unsigned long long* __restrict__ ev, uint32_t p0, uint32_t P,
                                            uint32_t a[4], uint32_t b[4]) {
    unsigned long long w[4] = {0ull, 0ull, 0ull, 0ull};
    if (p0 < P && P - p0 >= 4u) {
        const ulonglong2 x = *(const ulonglong2*)(ev + p0), y = *(const ulonglong2*)(ev + p0 + 2);
        w[0] = x.x; w[1] = x.y; w[2] = y.x; w[3] = y.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 < P && (uint32_t)j < P - p0) w[j] = ev[p0 + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) depth_decode(w[j], a[j], b[j]);
}

// sums[chunk] = (sum of a | sum of b << 32) over the chunk's positions, both modulo 2^32
__global__ __launch_bounds__(256) void k_depth_chunk_sums(const unsigned long long* __restrict__ ev, uint32_t P,
                                                          uint32_t tiles_per_chunk, uint32_t n_tiles,
                                                          unsigned long long* __restrict__ sums) {
    __shared__ uint32_t s_w[4][2];
    const uint32_t t0 = blockIdx.x * tiles_per_chunk;
    const uint32_t t1 = min(n_tiles, t0 + tiles_per_chunk);
    uint32_t sa = 0, sb = 0;
    for (uint32_t t = t0; t < t1; ++t) {
        uint32_t a[4], b[4];
        depth_load4(ev, t * kDepthTile + 4u * threadIdx.x, P, a, b);
        sa += a[0] + a[1] + a[2] + a[3];
        sb += b[0] + b[1] + b[2] + b[3];
    }
    sa = wave_sum_u32(sa);
    sb = wave_sum_u32(sb);
    if ((threadIdx.x & 63u) == 0) {
        s_w[threadIdx.x >> 6][0] = sa;
        s_w[threadIdx.x >> 6][1] = sb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t ta = s_w[0][0] + s_w[1][0] + s_w[2][0] + s_w[3][0];
        const uint32_t tb = s_w[0][1] + s_w[1][1] + s_w[2][1] + s_w[3][1];
        sums[blockIdx.x] = (unsigned long long)ta | ((unsigned long long)tb << 32);
    }
}

// exclusive scan of at most kDepthMaxChunks chunk sums, in place, both channels: one workgroup, a thread per 8 entries
__global__ __launch_bounds__(256) void k_depth_spine(unsigned long long* __restrict__ sums, uint32_t n_chunks) {
    __shared__ uint32_t s_a[256], s_b[256];
    constexpr uint32_t kPer = kDepthMaxChunks / 256;
    uint32_t a[kPer], b[kPer], ta = 0, tb = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        const uint32_t i = threadIdx.x * kPer + j;
        const unsigned long long w = i < n_chunks ? sums[i] : 0ull;
        a[j] = (uint32_t)w;
        b[j] = (uint32_t)(w >> 32);
        ta += a[j];
        tb += b[j];
    }
    s_a[threadIdx.x] = ta;
    s_b[threadIdx.x] = tb;
    __syncthreads();
    uint32_t ra = 0, rb = 0;
    for (uint32_t t = 0; t < threadIdx.x; ++t) {
        ra += s_a[t];
        rb += s_b[t];
    }
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        const uint32_t i = threadIdx.x * kPer + j;
        if (i < n_chunks) sums[i] = (unsigned long long)ra | ((unsigned long long)rb << 32);
        ra += a[j];
        rb += b[j];
    }
}

// sorted, disjoint position intervals of the batch's axis, each feeding one row of the accumulators
struct DepthIntervals {
    const uint32_t* lo;   // inclusive bounds
    const uint32_t* hi;
    const uint32_t* row;
    uint32_t n;
};

// the first interval of [a, b) with hi >= p (b if none)
__device__ __forceinline__ uint32_t depth_first_interval(const uint32_t* __restrict__ hi, uint32_t a, uint32_t b, uint32_t p) {
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (hi[m] < p) a = m + 1;
        else b = m;
    }
    return a;
}

// what a run of positions of one row adds to it
struct DepthPartial {
    unsigned long long sum_in, sum_kept, deficit_sum;
    uint32_t capped, deficit, min_in, max_in, min_kept, max_kept;
};
__device__ __forceinline__ void depth_partial_clear(DepthPartial& q) {
    q.sum_in = q.sum_kept = q.deficit_sum = 0ull;
    q.capped = q.deficit = 0u;
    q.min_in = q.min_kept = 0xFFFFFFFFu;
    q.max_in = q.max_kept = 0u;
}
__device__ __forceinline__ void depth_partial_add(DepthPartial& q, uint32_t cov, uint32_t kept, uint32_t M) {
    const uint32_t need = min(cov, M);
    q.sum_in += cov;
    q.sum_kept += kept;
    q.capped += cov > M ? 1u : 0u;
    if (kept < need) {
        q.deficit++;
        q.deficit_sum += need - kept;
    }
    q.min_in = min(q.min_in, cov);
    q.max_in = max(q.max_in, cov);
    q.min_kept = min(q.min_kept, kept);
    q.max_kept = max(q.max_kept, kept);
}
__device__ __forceinline__ unsigned long long depth_shfl_down_u64(unsigned long long v, int o) {
    return (unsigned long long)__shfl_down((long long)v, o, kWave);
}
// accumulators: acc64[5][n_rows] = sum_in, sum_kept, capped, deficit, deficit_sum; acc32[4][n_rows] = min_in, max_in,
// min_kept, max_kept (the minima preset to ~0u)
__device__ __forceinline__ void depth_flush(const DepthPartial& q, uint32_t row, uint32_t n_rows,
                                            unsigned long long* __restrict__ acc64, uint32_t* __restrict__ acc32) {
    if (q.sum_in) atomicAdd(&acc64[row], q.sum_in);
    if (q.sum_kept) atomicAdd(&acc64[(size_t)n_rows + row], q.sum_kept);
    if (q.capped) atomicAdd(&acc64[2 * (size_t)n_rows + row], (unsigned long long)q.capped);
    if (q.deficit) atomicAdd(&acc64[3 * (size_t)n_rows + row], (unsigned long long)q.deficit);
    if (q.deficit_sum) atomicAdd(&acc64[4 * (size_t)n_rows + row], q.deficit_sum);
    atomicMin(&acc32[row], q.min_in);
    atomicMax(&acc32[(size_t)n_rows + row], q.max_in);
    atomicMin(&acc32[2 * (size_t)n_rows + row], q.min_kept);
    atomicMax(&acc32[3 * (size_t)n_rows + row], q.max_kept);
}

// One table's share of a thread's four positions.  k: the thread's interval index (first interval with hi >= p0, kept
// monotone); runs that end inside the thread are flushed at once, the last one is reduced over the wave's lanes that
// share its row (rows are monotone over the lanes, so equal rows are contiguous) and flushed by the run's first lane.
// in[j]: position j lies in an interval of the table.
__device__ __forceinline__ void depth_rows(const DepthIntervals& tb, uint32_t k, uint32_t p0, uint32_t P,
                                           const uint32_t cov[4], const uint32_t kept[4], uint32_t M, uint32_t n_rows,
                                           unsigned long long* __restrict__ acc64, uint32_t* __restrict__ acc32,
                                           bool in[4]) {
    DepthPartial q;
    depth_partial_clear(q);
    uint32_t row = kDepthNoRow;
    uint32_t lo_k = 0, hi_k = 0, row_k = kDepthNoRow;
    bool have = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        in[j] = false;
        const uint32_t p = p0 + j;
        if (p0 >= P || (uint32_t)j >= P - p0) continue;
        while (k < tb.n) {
            if (!have) {
                lo_k = tb.lo[k];
                hi_k = tb.hi[k];
                row_k = tb.row[k];
                have = true;
            }
            if (hi_k >= p) break;
            ++k;
            have = false;
        }
        const uint32_t r = (k < tb.n && lo_k <= p) ? row_k : kDepthNoRow;
        in[j] = r != kDepthNoRow;
        if (r != row) {
            if (row != kDepthNoRow) depth_flush(q, row, n_rows, acc64, acc32);
            depth_partial_clear(q);
            row = r;
        }
        if (r != kDepthNoRow) depth_partial_add(q, cov[j], kept[j], M);
    }
    const uint32_t lane = threadIdx.x & 63u;
    if (__ballot(row != kDepthNoRow) == 0ull) return;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t orow = (uint32_t)__shfl_down((int)row, o, kWave);
        const unsigned long long si = depth_shfl_down_u64(q.sum_in, o), sk = depth_shfl_down_u64(q.sum_kept, o),
                                 ds = depth_shfl_down_u64(q.deficit_sum, o);
        const uint32_t cp = (uint32_t)__shfl_down((int)q.capped, o, kWave), df = (uint32_t)__shfl_down((int)q.deficit, o, kWave),
                       mi = (uint32_t)__shfl_down((int)q.min_in, o, kWave), xi = (uint32_t)__shfl_down((int)q.max_in, o, kWave),
                       mk = (uint32_t)__shfl_down((int)q.min_kept, o, kWave),
                       xk = (uint32_t)__shfl_down((int)q.max_kept, o, kWave);
        if (lane + o < 64u && orow == row && row != kDepthNoRow) {
            q.sum_in += si;
            q.sum_kept += sk;
            q.deficit_sum += ds;
            q.capped += cp;
            q.deficit += df;
            q.min_in = min(q.min_in, mi);
            q.max_in = max(q.max_in, xi);
            q.min_kept = min(q.min_kept, mk);
            q.max_kept = max(q.max_kept, xk);
        }
    }
    const uint32_t prev = (uint32_t)__shfl_up((int)row, 1, kWave);
    if (row != kDepthNoRow && (lane == 0 || prev != row)) depth_flush(q, row, n_rows, acc64, acc32);
}

// spine: the exclusive chunk sums of k_depth_spine.  regions.n == 0 and !scope_regions: no region table.  Scope of the
// histograms: the positions inside a region when scope_regions, every position otherwise.  hist: [n_bins in | n_bins
// kept] 64-bit words, n_bins == 0: none.  Dynamic LDS: 2 * n_bins words.
__global__ __launch_bounds__(256) void k_depth_consume(const unsigned long long* __restrict__ ev, uint32_t P,
                                                       uint32_t tiles_per_chunk, uint32_t n_tiles,
                                                       const unsigned long long* __restrict__ spine, uint32_t M,
                                                       DepthIntervals contigs, DepthIntervals regions, int scope_regions,
                                                       uint32_t n_rows, unsigned long long* __restrict__ acc64,
                                                       uint32_t* __restrict__ acc32, uint32_t n_bins,
                                                       unsigned long long* __restrict__ hist) {
    extern __shared__ uint32_t s_hist[];  // [n_bins in | n_bins kept]
    __shared__ uint32_t s_w[2][4][2];
    for (uint32_t i = threadIdx.x; i < 2u * n_bins; i += blockDim.x) s_hist[i] = 0u;
    const uint32_t t0 = blockIdx.x * tiles_per_chunk;
    const uint32_t t1 = min(n_tiles, t0 + tiles_per_chunk);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // the chunk's range of intervals of both tables: a thread's searches stay inside it
    const uint32_t p_first = t0 * kDepthTile;
    const uint32_t p_last = min(P, t1 * kDepthTile) - 1u;
    const uint32_t c_lo = depth_first_interval(contigs.hi, 0, contigs.n, p_first);
    const uint32_t c_hi = min(contigs.n, depth_first_interval(contigs.hi, c_lo, contigs.n, p_last) + 1u);
    uint32_t r_lo = 0, r_hi = 0;
    if (regions.n) {
        r_lo = depth_first_interval(regions.hi, 0, regions.n, p_first);
        r_hi = min(regions.n, depth_first_interval(regions.hi, r_lo, regions.n, p_last) + 1u);
    }
    const unsigned long long carry0 = spine[blockIdx.x];
    uint32_t carry_a = (uint32_t)carry0, carry_b = (uint32_t)(carry0 >> 32);
    __syncthreads();  // (the histograms are zero)
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t p0 = t * kDepthTile + 4u * threadIdx.x;
        uint32_t a[4], b[4];
        depth_load4(ev, p0, P, a, b);
        a[1] += a[0]; a[2] += a[1]; a[3] += a[2];
        b[1] += b[0]; b[2] += b[1]; b[3] += b[2];
        const uint32_t ia = wave_incl_scan_add(a[3]), ib = wave_incl_scan_add(b[3]);
        const uint32_t par = t & 1u;
        if (lane == 63u) {
            s_w[par][wave][0] = ia;
            s_w[par][wave][1] = ib;
        }
        __syncthreads();
        uint32_t off_a = carry_a + ia - a[3], off_b = carry_b + ib - b[3];
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            const uint32_t wa = s_w[par][w][0], wb = s_w[par][w][1];
            if (w < wave) {
                off_a += wa;
                off_b += wb;
            }
            carry_a += wa;
            carry_b += wb;
        }
        uint32_t cov[4], kept[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cov[j] = off_a + a[j];
            kept[j] = off_b + b[j];
        }
        bool in_c[4], in_r[4];
        depth_rows(contigs, depth_first_interval(contigs.hi, c_lo, c_hi, p0), p0, P, cov, kept, M, n_rows, acc64, acc32, in_c);
        if (regions.n)
            depth_rows(regions, depth_first_interval(regions.hi, r_lo, r_hi, p0), p0, P, cov, kept, M, n_rows, acc64, acc32,
                       in_r);
        if (n_bins) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool scope = scope_regions ? (regions.n != 0 && in_r[j]) : in_c[j];
                if (scope) {
                    atomicAdd(&s_hist[min(cov[j], n_bins - 1u)], 1u);
                    atomicAdd(&s_hist[n_bins + min(kept[j], n_bins - 1u)], 1u);
                }
            }
        }
    }
    if (n_bins) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < 2u * n_bins; i += blockDim.x) {
            const uint32_t v = s_hist[i];
            if (v) atomicAdd(&hist[i], (unsigned long long)v);
        }
    }
}

void launch_depth_events(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids, uint32_t n,
                         const uint64_t* mask, const uint32_t* lengths, const uint32_t* boff, uint32_t n_contigs,
                         uint32_t c0, uint32_t c1, uint64_t* ev, uint64_t* counts, uint32_t* err) {
    if (n == 0) return;
    const dim3 grid(grid_for(((uint64_t)n + 255) / 256 * 64, 256)), block(256);  // a wave per 256 reads
    const bool vec = (((uintptr_t)starts | (uintptr_t)ends | (uintptr_t)ids) & 15u) == 0;
    const bool lds = n_contigs <= kDepthLdsContigs;
    const size_t shm = lds ? 2 * (size_t)n_contigs * sizeof(uint32_t) : 0;
#define QMCP_DE(TAB, VEC)                                                                                           \
    hipLaunchKernelGGL((k_depth_events<TAB, VEC>), grid, block, shm, st, starts, ends, ids, n, mask, lengths, boff, \
                       n_contigs, c0, c1, (unsigned long long*)ev, (unsigned long long*)counts, err)
    if (lds && vec) QMCP_DE(1, true);
    else if (lds) QMCP_DE(1, false);
    else if (vec) QMCP_DE(2, true);
    else QMCP_DE(2, false);
#undef QMCP_DE
}

uint32_t depth_lds_contigs() { return kDepthLdsContigs; }

uint32_t depth_chunks(uint32_t positions) {
    const uint32_t n_tiles = (positions + kDepthTile - 1) / kDepthTile;
    if (n_tiles == 0) return 0;
    const uint32_t per = (n_tiles + kDepthMaxChunks - 1) / kDepthMaxChunks;
    return (n_tiles + per - 1) / per;
}

void launch_depth_sums(hipStream_t st, const uint64_t* ev, uint32_t positions, uint64_t* sums) {
    if (positions == 0) return;
    const uint32_t n_tiles = (positions + kDepthTile - 1) / kDepthTile;
    const uint32_t per = (n_tiles + kDepthMaxChunks - 1) / kDepthMaxChunks;
    const uint32_t chunks = (n_tiles + per - 1) / per;
    hipLaunchKernelGGL(k_depth_chunk_sums, dim3(chunks), dim3(256), 0, st, (const unsigned long long*)ev, positions, per,
                       n_tiles, (unsigned long long*)sums);
    hipLaunchKernelGGL(k_depth_spine, dim3(1), dim3(256), 0, st, (unsigned long long*)sums, chunks);
}

void launch_depth_consume(hipStream_t st, const uint64_t* ev, uint32_t positions, const uint64_t* sums, uint32_t M,
                          const uint32_t* c_lo, const uint32_t* c_hi, const uint32_t* c_row, uint32_t n_c,
                          const uint32_t* r_lo, const uint32_t* r_hi, const uint32_t* r_row, uint32_t n_r,
                          bool scope_regions, uint32_t n_rows, uint64_t* acc64, uint32_t* acc32, uint32_t n_bins,
                          uint64_t* hist) {
    if (positions == 0) return;
    const uint32_t n_tiles = (positions + kDepthTile - 1) / kDepthTile;
    const uint32_t per = (n_tiles + kDepthMaxChunks - 1) / kDepthMaxChunks;
    const uint32_t chunks = (n_tiles + per - 1) / per;
    const DepthIntervals ct = {c_lo, c_hi, c_row, n_c}, rt = {r_lo, r_hi, r_row, n_r};
    hipLaunchKernelGGL(k_depth_consume, dim3(chunks), dim3(256), 2 * (size_t)n_bins * sizeof(uint32_t), st,
                       (const unsigned long long*)ev, positions, per, n_tiles, (const unsigned long long*)sums, M, ct, rt,
                       scope_regions ? 1 : 0, n_rows, (unsigned long long*)acc64, acc32, n_bins,
                       (unsigned long long*)hist);
}
