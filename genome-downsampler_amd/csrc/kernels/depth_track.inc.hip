// depth_track.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after depth_report).
// qmcp_hip_depth_track_*: the depth report's pipeline with another last stage.  The event words, the chunk sums and the
// spine of depth_report.inc.hip give cov(p) and kept(p) in registers for every position of a batch's axis; here they are
// run-length compacted into records (contig, start, end, depth_in, depth_kept, short), in genome order.
//   k_track_count   a workgroup per chunk, the tile scan of k_depth_consume (depth_load4, wave_incl_scan_add on both
//                   channels, the carry from the spine).  Every position gets its KEY (scope interval or "not emitted",
//                   depth_in, depth_kept, short) and two flags from its own key and the key of the position before it:
//                     head(p)  p is emitted and p - 1 is not emitted, lies in another interval or has another tuple
//                     tail'(p) p - 1 is emitted and p is not emitted, lies in another interval or has another tuple
//                   The key of the position before a thread's first one needs no neighbour: its cov and kept are the
//                   thread's exclusive prefix (off_a, off_b -- for a chunk's first position that is spine[chunk]), its
//                   interval follows from the thread's own interval cursor.  Heads, emitted positions and short positions
//                   are counted per chunk (ballot + popcount per wave, LDS across the four waves).
//   k_track_spine   one workgroup: exclusive scan of the chunks' head counts in place, the three totals of the batch
//   k_track_emit    the same flags again.  A head takes rank = chunk base + heads before it and writes contig, start and
//                   the tuple of record `rank`.  RUN ENDS: tail'(p) says that the run holding p - 1 ends there, and that
//                   run is the last one begun before p, so tail'(p) writes end = p - 1 of record (heads before p) - 1 --
//                   one scan serves both flags and no look-ahead word is read.  The position after the axis' last one is
//                   never emitted; it lies in the last tile unless P is a multiple of the tile, and then the last chunk's
//                   first thread closes the open run after its loop.
// No global atomics, no inline assembly.  Records are written by the thread that owns the position; nothing is indexed
// beyond P (ev) or beyond the batch's run count (every rank is below the total that k_track_spine returned for the same
// flags, and a tail' has a head before it).

constexpr uint32_t kTrackNone = 0xFFFFFFFFu;

// depth_cap == 0 arrives as cap = ~0u
struct TrackParams {
    uint32_t M, flags, cap;
};

// iv: index of the scope interval, kTrackNone when the position is not emitted
struct TrackKey {
    uint32_t iv, din, dk, sh;
};

// the key of a position with depths (cov, kept) inside scope interval iv (kTrackNone: outside the scope); in_scope_short:
// the position counts for short_positions whatever the flags say
__device__ __forceinline__ TrackKey track_key(uint32_t cov, uint32_t kept, uint32_t iv, const TrackParams& tp,
                                              uint32_t& in_scope_short) {
    TrackKey k;
    k.sh = (iv != kTrackNone && kept < min(cov, tp.M)) ? 1u : 0u;
    in_scope_short = k.sh;
    k.din = (tp.flags & QMCP_TRACK_IN) ? min(cov, tp.cap) : 0u;
    k.dk = (tp.flags & QMCP_TRACK_KEPT) ? min(kept, tp.cap) : 0u;
    bool em = iv != kTrackNone;
    if ((tp.flags & QMCP_TRACK_SHORT_ONLY) && !k.sh) em = false;
    if ((tp.flags & QMCP_TRACK_SKIP_ZERO) && (k.din | k.dk) == 0u) em = false;
    k.iv = em ? iv : kTrackNone;
    return k;
}
__device__ __forceinline__ bool track_same(const TrackKey& a, const TrackKey& b) {
    return a.iv == b.iv && a.din == b.din && a.dk == b.dk && a.sh == b.sh;
}
__device__ __forceinline__ bool track_head(const TrackKey& prev, const TrackKey& cur) {
    return cur.iv != kTrackNone && !(prev.iv != kTrackNone && track_same(prev, cur));
}
__device__ __forceinline__ bool track_tail_before(const TrackKey& prev, const TrackKey& cur) {
    return prev.iv != kTrackNone && !(cur.iv != kTrackNone && track_same(prev, cur));
}

// a thread's place in a table of sorted disjoint intervals: k is the first interval with hi >= the position last sought
// (k == n: none), lo / hi its bounds
struct TrackCursor {
    uint32_t k, lo, hi;
};
__device__ __forceinline__ void track_cursor_load(const DepthIntervals& tb, TrackCursor& c) {
    if (c.k < tb.n) {
        c.lo = tb.lo[c.k];
        c.hi = tb.hi[c.k];
    }
}
// a, b: the chunk's range of intervals (the search of k_depth_consume)
__device__ __forceinline__ TrackCursor track_cursor_at(const DepthIntervals& tb, uint32_t a, uint32_t b, uint32_t p) {
    TrackCursor c;
    c.k = depth_first_interval(tb.hi, a, b, p);
    c.lo = c.hi = 0u;
    track_cursor_load(tb, c);
    return c;
}
__device__ __forceinline__ void track_cursor_seek(const DepthIntervals& tb, TrackCursor& c, uint32_t p) {
    while (c.k < tb.n && c.hi < p) {
        ++c.k;
        track_cursor_load(tb, c);
    }
}
// the interval of p, the cursor sought to p
__device__ __forceinline__ uint32_t track_interval(const DepthIntervals& tb, const TrackCursor& c, uint32_t p) {
    return (c.k < tb.n && c.lo <= p) ? c.k : kTrackNone;
}
// the interval of p - 1, the cursor sought to p: the same one when it began before p, else the one before it when that
// ends at p - 1 (p == 0: k == 0, none)
__device__ __forceinline__ uint32_t track_interval_before(const DepthIntervals& tb, const TrackCursor& c, uint32_t p) {
    if (c.k < tb.n && c.lo < p) return c.k;
    if (c.k > 0u && tb.hi[c.k - 1u] + 1u == p) return c.k - 1u;
    return kTrackNone;
}

// scope: the table whose intervals bound the runs (the merged regions when the call has any, the contigs otherwise).
// contigs: read by kEmit only, for a record's contig and coordinates.  cnt: [heads | emitted | short] per chunk, the heads
// scanned by k_track_spine before kEmit reads them.
template <bool kEmit>
__device__ __forceinline__ void track_chunk(const unsigned long long* __restrict__ ev, uint32_t P, uint32_t tiles_per_chunk,
                                            uint32_t n_tiles, const unsigned long long* __restrict__ spine,
                                            const TrackParams tp, const DepthIntervals scope, const DepthIntervals contigs,
                                            uint32_t* __restrict__ cnt, uint32_t n_chunks,
                                            qmcp_hip_track_run* __restrict__ runs) {
    __shared__ uint32_t s_w[2][4][2];
    __shared__ uint32_t s_h[2][4];
    __shared__ uint32_t s_c[4][3];
    const uint32_t t0 = blockIdx.x * tiles_per_chunk;
    const uint32_t t1 = min(n_tiles, t0 + tiles_per_chunk);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t p_first = t0 * kDepthTile;
    const uint32_t p_last = min(P, t1 * kDepthTile) - 1u;
    const uint32_t s_lo = depth_first_interval(scope.hi, 0, scope.n, p_first);
    const uint32_t s_hi = min(scope.n, depth_first_interval(scope.hi, s_lo, scope.n, p_last) + 1u);
    uint32_t c_lo = 0, c_hi = 0;
    if constexpr (kEmit) {
        c_lo = depth_first_interval(contigs.hi, 0, contigs.n, p_first);
        c_hi = min(contigs.n, depth_first_interval(contigs.hi, c_lo, contigs.n, p_last) + 1u);
    }
    const unsigned long long carry0 = spine[blockIdx.x];
    uint32_t carry_a = (uint32_t)carry0, carry_b = (uint32_t)(carry0 >> 32);
    uint32_t n_heads = 0, n_em = 0, n_short = 0;     // !kEmit: this thread's counts
    uint32_t rank_carry = kEmit ? cnt[blockIdx.x] : 0u;  // kEmit: heads before the tile
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
        // keys and flags: the position before p0 has depths (off_a, off_b)
        TrackCursor sc = track_cursor_at(scope, s_lo, s_hi, p0);
        uint32_t sh_bit;
        TrackKey prev = track_key(off_a, off_b, track_interval_before(scope, sc, p0), tp, sh_bit);
        uint32_t heads = 0, tails = 0, h_thread = 0;  // bit j: position p0 + j
        uint32_t din[4], dk[4], shj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t p = p0 + j;
            track_cursor_seek(scope, sc, p);
            const TrackKey cur = track_key(off_a + a[j], off_b + b[j], track_interval(scope, sc, p), tp, sh_bit);
            const bool h = track_head(prev, cur);
            heads |= (h ? 1u : 0u) << j;
            tails |= (track_tail_before(prev, cur) ? 1u : 0u) << j;
            h_thread += h ? 1u : 0u;
            if constexpr (kEmit) {
                din[j] = cur.din;
                dk[j] = cur.dk;
                shj[j] = cur.sh;
            } else {
                n_em += cur.iv != kTrackNone ? 1u : 0u;
                n_short += sh_bit;
            }
            prev = cur;
        }
        if constexpr (!kEmit) {
            n_heads += h_thread;
        } else {
            const uint32_t ih = wave_incl_scan_add(h_thread);
            if (lane == 63u) s_h[par][wave] = ih;
            __syncthreads();
            uint32_t rank = rank_carry + ih - h_thread;
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) {
                const uint32_t wh = s_h[par][w];
                if (w < wave) rank += wh;
                rank_carry += wh;
            }
            if (heads | tails) {
                TrackCursor cc = track_cursor_at(contigs, c_lo, c_hi, p0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t p = p0 + j;
                    if (((heads | tails) >> j) == 0u) break;
                    track_cursor_seek(contigs, cc, p);
                    if ((tails >> j) & 1u) {
                        // p - 1 lies in the contig of p when that began before p, else on the last position of the one before
                        const uint32_t end = (cc.k < contigs.n && cc.lo < p) ? p - 1u - cc.lo
                                                                              : contigs.hi[cc.k - 1u] - contigs.lo[cc.k - 1u];
                        runs[rank - 1u].end = end;
                    }
                    if ((heads >> j) & 1u) {
                        qmcp_hip_track_run* r = runs + rank;
                        r->contig = contigs.row[cc.k];
                        r->start = p - cc.lo;
                        r->depth_in = din[j];
                        r->depth_kept = dk[j];
                        r->flags = shj[j];
                        ++rank;
                    }
                }
            }
        }
    }
    if constexpr (kEmit) {
        // P a multiple of the tile: the position after the last one lies in no tile, and a run open at P - 1 ends there
        if (blockIdx.x + 1u == gridDim.x && P == n_tiles * kDepthTile && threadIdx.x == 0) {
            uint32_t sh_bit;
            const uint32_t iv = (scope.n && scope.hi[scope.n - 1u] + 1u == P) ? scope.n - 1u : kTrackNone;
            const TrackKey last = track_key(carry_a, carry_b, iv, tp, sh_bit);
            if (last.iv != kTrackNone) runs[rank_carry - 1u].end = contigs.hi[contigs.n - 1u] - contigs.lo[contigs.n - 1u];
        }
    } else {
        const uint32_t wh = wave_sum_u32(n_heads), we = wave_sum_u32(n_em), ws = wave_sum_u32(n_short);
        __syncthreads();
        if (lane == 0) {
            s_c[wave][0] = wh;
            s_c[wave][1] = we;
            s_c[wave][2] = ws;
        }
        __syncthreads();
        if (threadIdx.x < 3u)
            cnt[threadIdx.x * n_chunks + blockIdx.x] =
                s_c[0][threadIdx.x] + s_c[1][threadIdx.x] + s_c[2][threadIdx.x] + s_c[3][threadIdx.x];
    }
}

__global__ __launch_bounds__(256) void k_track_count(const unsigned long long* __restrict__ ev, uint32_t P,
                                                     uint32_t tiles_per_chunk, uint32_t n_tiles,
                                                     const unsigned long long* __restrict__ spine, TrackParams tp,
                                                     DepthIntervals scope, uint32_t* __restrict__ cnt, uint32_t n_chunks) {
    track_chunk<false>(ev, P, tiles_per_chunk, n_tiles, spine, tp, scope, scope, cnt, n_chunks, nullptr);
}

__global__ __launch_bounds__(256) void k_track_emit(const unsigned long long* __restrict__ ev, uint32_t P,
                                                    uint32_t tiles_per_chunk, uint32_t n_tiles,
                                                    const unsigned long long* __restrict__ spine, TrackParams tp,
                                                    DepthIntervals scope, DepthIntervals contigs,
                                                    const uint32_t* __restrict__ cnt, uint32_t n_chunks,
                                                    qmcp_hip_track_run* __restrict__ runs) {
    track_chunk<true>(ev, P, tiles_per_chunk, n_tiles, spine, tp, scope, contigs, const_cast<uint32_t*>(cnt), n_chunks,
                      runs);
}

// cnt: [heads | emitted | short] x n_chunks (n_chunks <= kDepthMaxChunks).  The heads are scanned in place (exclusive);
// totals[0 .. 2] = the batch's heads, emitted positions and short positions.  One workgroup, a thread per 8 chunks.
__global__ __launch_bounds__(256) void k_track_spine(uint32_t* __restrict__ cnt, uint32_t n_chunks,
                                                     unsigned long long* __restrict__ totals) {
    __shared__ uint32_t s_t[3][256];
    constexpr uint32_t kPer = kDepthMaxChunks / 256;
    uint32_t h[kPer], th = 0, te = 0, ts = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        const uint32_t i = threadIdx.x * kPer + j;
        h[j] = i < n_chunks ? cnt[i] : 0u;
        th += h[j];
        te += i < n_chunks ? cnt[n_chunks + i] : 0u;
        ts += i < n_chunks ? cnt[2u * n_chunks + i] : 0u;
    }
    s_t[0][threadIdx.x] = th;
    s_t[1][threadIdx.x] = te;
    s_t[2][threadIdx.x] = ts;
    __syncthreads();
    uint32_t r = 0;
    for (uint32_t t = 0; t < threadIdx.x; ++t) r += s_t[0][t];
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        const uint32_t i = threadIdx.x * kPer + j;
        if (i < n_chunks) cnt[i] = r;
        r += h[j];
    }
    if (threadIdx.x < 3u) {
        unsigned long long tot = 0ull;
        for (uint32_t t = 0; t < 256u; ++t) tot += s_t[threadIdx.x][t];
        totals[threadIdx.x] = tot;
    }
}

namespace {
struct TrackGrid {
    uint32_t n_tiles, per, chunks;
};
TrackGrid track_grid(uint32_t positions) {  // the chunks of launch_depth_sums
    TrackGrid g;
    g.n_tiles = (positions + kDepthTile - 1) / kDepthTile;
    g.per = (g.n_tiles + kDepthMaxChunks - 1) / kDepthMaxChunks;
    g.chunks = (g.n_tiles + g.per - 1) / g.per;
    return g;
}
}  // namespace

void launch_track_count(hipStream_t st, const uint64_t* ev, uint32_t positions, const uint64_t* sums, uint32_t M,
                        uint32_t flags, uint32_t depth_cap, const uint32_t* s_lo, const uint32_t* s_hi, uint32_t n_s,
                        uint32_t* cnt, uint64_t* totals) {
    if (positions == 0) return;
    const TrackGrid g = track_grid(positions);
    const TrackParams tp = {M, flags, depth_cap ? depth_cap : 0xFFFFFFFFu};
    const DepthIntervals sc = {s_lo, s_hi, nullptr, n_s};
    hipLaunchKernelGGL(k_track_count, dim3(g.chunks), dim3(256), 0, st, (const unsigned long long*)ev, positions, g.per,
                       g.n_tiles, (const unsigned long long*)sums, tp, sc, cnt, g.chunks);
    hipLaunchKernelGGL(k_track_spine, dim3(1), dim3(256), 0, st, cnt, g.chunks, (unsigned long long*)totals);
}

void launch_track_emit(hipStream_t st, const uint64_t* ev, uint32_t positions, const uint64_t* sums, uint32_t M,
                       uint32_t flags, uint32_t depth_cap, const uint32_t* s_lo, const uint32_t* s_hi, uint32_t n_s,
                       const uint32_t* c_lo, const uint32_t* c_hi, const uint32_t* c_row, uint32_t n_c,
                       const uint32_t* cnt, qmcp_hip_track_run* runs) {
    if (positions == 0) return;
    const TrackGrid g = track_grid(positions);
    const TrackParams tp = {M, flags, depth_cap ? depth_cap : 0xFFFFFFFFu};
    const DepthIntervals sc = {s_lo, s_hi, nullptr, n_s}, ct = {c_lo, c_hi, c_row, n_c};
    hipLaunchKernelGGL(k_track_emit, dim3(g.chunks), dim3(256), 0, st, (const unsigned long long*)ev, positions, g.per,
                       g.n_tiles, (const unsigned long long*)sums, tp, sc, ct, cnt, g.chunks, runs);
}
