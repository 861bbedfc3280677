// amplicon_clip.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp, after
// amplicon_by_contig).  The assign step of qmcp_hip_solve_amplicons_*: one streaming pass over the units (pairs of reads
// 2q, 2q + 1, or single reads) that validates every read, applies the length / MAPQ filters, assigns the unit to one
// amplicon of its contig (amplicon_assign.h's rule and walk) and clips its reads to that amplicon's insert.  It moves
// bytes and little else: a grid-stride loop of 256 threads, capped at grid_for's 2048 blocks, one 64-unit keep word per
// wave by ballot, uint2 loads and stores per pair, no atomics except the error word -- the counters leave each block as
// one row of partial sums, and k_ac_totals adds the rows.

// Amplicons staged in LDS: 6 words each, 2 560 x 24 B = 60 KiB.  That stays under the 64 KiB a launch gets without
// asking for more, and two workgroups (120 KiB and their 512 B of counters) fit the 160 KiB of a CU.  At the full
// table that is two workgroups, 8 waves, a CU: enough for a pass that streams; a panel's table (a few KiB) leaves the
// residency to the registers.
constexpr uint32_t kAcLdsMax = 2560;

// kPairs: a unit is the reads 2q, 2q + 1 (columns read and written as uint2), else the read q.  kLds: the table
// (amplicon_assign.h: AssignTable::words, n_amp x 6) staged in LDS, else read from global memory.
// Every read is validated as k_amplicon_filter_by_contig does, those of dropped units included (err bit 0 an id that is
// neither < n_contigs nor QMCP_NO_CONTIG, bit 1 a placed read with start > end or end >= its contig's length).
// Per unit: label (index in the caller's table or QMCP_NO_AMPLICON) and one keep bit.  Per read: the solve columns cs /
// ce / ci -- pooled: the clipped read in genome coordinates and its contig; per_amplicon: the clipped read rebased to
// the insert and the amplicon's index -- and, when rs is given, the rebased columns rs / re / ri as well.  A read of an
// unassigned unit, and a read clipped away, get {0, 0, QMCP_NO_CONTIG}.  used[k] = 1 for every assigned amplicon k (the
// same plain store from every unit of k).
template <bool kPairs, bool kLds>
__global__ __launch_bounds__(256) void k_amplicon_clip(
    const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends, const uint32_t* __restrict__ ids,
    const uint32_t* __restrict__ seq_lengths, const uint32_t* __restrict__ qualities, uint64_t n_units,
    const uint32_t* __restrict__ lengths, uint32_t n_contigs, const uint32_t* __restrict__ amp_offs,
    const uint32_t* __restrict__ tab_g, uint32_t n_amp, uint32_t min_length, uint32_t min_mapq, uint32_t per_amplicon,
    uint32_t* __restrict__ label, uint64_t* __restrict__ unit_keep, uint32_t* __restrict__ cs, uint32_t* __restrict__ ce,
    uint32_t* __restrict__ ci, uint32_t* __restrict__ rs, uint32_t* __restrict__ re, uint32_t* __restrict__ ri,
    uint32_t* __restrict__ used, uint64_t* __restrict__ partials, uint32_t* __restrict__ err) {
    extern __shared__ uint32_t s_tab[];  // kLds: the six columns
    __shared__ uint64_t s_part[4][kAcCounts];
    const uint32_t* tab = tab_g;
    if constexpr (kLds) {
        for (uint32_t i = threadIdx.x; i < 6 * n_amp; i += blockDim.x) s_tab[i] = tab_g[i];
        __syncthreads();
        tab = s_tab;
    }
    const uint32_t* t_start = tab;
    const uint32_t* t_end = tab + n_amp;
    const uint32_t* t_pmax = tab + 2 * (size_t)n_amp;
    const uint32_t* t_index = tab + 3 * (size_t)n_amp;
    const uint32_t* t_is = tab + 4 * (size_t)n_amp;
    const uint32_t* t_ie = tab + 5 * (size_t)n_amp;
    constexpr int kReads = kPairs ? 2 : 1;
    const uint64_t n_words = (n_units + 63) / 64;
    const uint64_t wave_global = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t bad = 0;
    uint32_t n_assigned = 0, n_filtered = 0, n_none = 0, n_several = 0, n_short = 0, n_away = 0;
    uint64_t bases = 0;
    for (uint64_t w = wave_global; w < n_words; w += n_waves) {
        const uint64_t q = w * 64 + lane;
        bool ok = false;
        if (q < n_units) {
            uint32_t s[kReads], e[kReads], id[kReads];
            if constexpr (kPairs) {
                const uint2 s2 = ((const uint2*)starts)[q], e2 = ((const uint2*)ends)[q], i2 = ((const uint2*)ids)[q];
                s[0] = s2.x, s[1] = s2.y, e[0] = e2.x, e[1] = e2.y, id[0] = i2.x, id[1] = i2.y;
            } else {
                s[0] = starts[q], e[0] = ends[q], id[0] = ids[q];
            }
            bool placed = true;
            for (int r = 0; r < kReads; ++r) {
                if (id[r] < n_contigs) {
                    if (s[r] > e[r] || e[r] >= lengths[id[r]]) bad |= 2u;
                } else {
                    placed = false;
                    if (id[r] != QMCP_NO_CONTIG) bad |= 1u;
                }
            }
            bool pass = true;
            if (qualities) {
                if constexpr (kPairs) {
                    const uint2 mq = ((const uint2*)qualities)[q];
                    pass = mq.x >= min_mapq && mq.y >= min_mapq;
                } else {
                    pass = qualities[q] >= min_mapq;
                }
            }
            if (seq_lengths) {
                if constexpr (kPairs) {
                    const uint2 ln = ((const uint2*)seq_lengths)[q];
                    pass = pass && ln.x >= min_length && ln.y >= min_length;
                } else {
                    pass = pass && seq_lengths[q] >= min_length;
                }
            }
            uint32_t found = QMCP_NO_AMPLICON;
            bool several = false;
            if (!pass) {
                n_filtered++;
            } else {
                if (placed && id[0] == id[kReads - 1]) {
                    const uint32_t lo = amp_offs[id[0]], hi = amp_offs[id[0] + 1];
                    const uint32_t m = min(s[0], s[kReads - 1]), x = max(e[0], e[kReads - 1]);
                    uint32_t a = lo, b = hi;  // first amplicon of the contig with start > m lies in [a, b]
                    while (a < b) {
                        const uint32_t mid = a + ((b - a) >> 1);
                        if (t_start[mid] <= m) a = mid + 1;
                        else b = mid;
                    }
                    // backwards from the last amplicon starting at or before m (amplicon_assign.h: assign_amplicon)
                    for (uint32_t k = a; k > lo;) {
                        --k;
                        if (t_pmax[k] < x) break;
                        if (t_end[k] >= x) {
                            if (found == QMCP_NO_AMPLICON) {
                                found = k;
                            } else {
                                several = true;
                                break;
                            }
                        }
                    }
                }
                if (found == QMCP_NO_AMPLICON) n_none++;
            }
            uint32_t os[kReads], oe[kReads], oc[kReads], bs[kReads], be[kReads], bc[kReads];
            uint32_t lab = QMCP_NO_AMPLICON;
            for (int r = 0; r < kReads; ++r) {
                os[r] = oe[r] = bs[r] = be[r] = 0;
                oc[r] = bc[r] = QMCP_NO_CONTIG;
            }
            if (found != QMCP_NO_AMPLICON) {
                ok = true;
                n_assigned++;
                n_several += several ? 1u : 0u;
                lab = t_index[found];
                used[lab] = 1u;
                const uint32_t is = t_is[found], ie = t_ie[found];
                for (int r = 0; r < kReads; ++r) {
                    const uint32_t a = max(s[r], is), b = min(e[r], ie);
                    if (a > b) {
                        n_away++;
                        bases += (uint64_t)(e[r] - s[r]) + 1;
                        continue;
                    }
                    if (a != s[r] || b != e[r]) {
                        n_short++;
                        bases += (uint64_t)(a - s[r]) + (e[r] - b);
                    }
                    bs[r] = a - is, be[r] = b - is, bc[r] = lab;
                    if (per_amplicon) os[r] = bs[r], oe[r] = be[r], oc[r] = lab;
                    else os[r] = a, oe[r] = b, oc[r] = id[r];
                }
            }
            label[q] = lab;
            if constexpr (kPairs) {
                ((uint2*)cs)[q] = make_uint2(os[0], os[1]);
                ((uint2*)ce)[q] = make_uint2(oe[0], oe[1]);
                ((uint2*)ci)[q] = make_uint2(oc[0], oc[1]);
                if (rs) {
                    ((uint2*)rs)[q] = make_uint2(bs[0], bs[1]);
                    ((uint2*)re)[q] = make_uint2(be[0], be[1]);
                    ((uint2*)ri)[q] = make_uint2(bc[0], bc[1]);
                }
            } else {
                cs[q] = os[0], ce[q] = oe[0], ci[q] = oc[0];
                if (rs) rs[q] = bs[0], re[q] = be[0], ri[q] = bc[0];
            }
        }
        const uint64_t word = __ballot(ok);
        if (lane == 0) unit_keep[w] = word;
    }
    if (bad) atomicOr(err, bad);
    // the block's row of partial sums: wave by wave through shuffles, then the four waves through LDS
    uint64_t v[kAcCounts] = {n_assigned, n_filtered, n_none, n_several, n_short, n_away, bases, 0};
    for (uint32_t i = 0; i < kAcCounts; ++i)
        for (int d = 32; d > 0; d >>= 1) v[i] += __shfl_down(v[i], d, 64);
    if (lane == 0)
        for (uint32_t i = 0; i < kAcCounts; ++i) s_part[threadIdx.x >> 6][i] = v[i];
    __syncthreads();
    if (threadIdx.x < kAcCounts)
        partials[(size_t)blockIdx.x * kAcCounts + threadIdx.x] =
            s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
}

// the rows of partial sums added up, and the amplicons no unit was assigned to counted into totals[kAcUnused]: one block
__global__ __launch_bounds__(256) void k_ac_totals(const uint64_t* __restrict__ partials, uint32_t n_rows,
                                                   const uint32_t* __restrict__ used, uint32_t n_amp,
                                                   uint64_t* __restrict__ totals) {
    __shared__ uint64_t s_sum[256];
    const uint32_t col = threadIdx.x % kAcCounts, first = threadIdx.x / kAcCounts, step = 256 / kAcCounts;
    uint64_t sum = 0;
    for (uint32_t r = first; r < n_rows; r += step) sum += partials[(size_t)r * kAcCounts + col];
    if (col == kAcUnused)
        for (uint32_t k = first; k < n_amp; k += step) sum += used[k] ? 0u : 1u;
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x < kAcCounts) {
        uint64_t t = 0;
        for (uint32_t r = 0; r < step; ++r) t += s_sum[r * kAcCounts + threadIdx.x];
        totals[threadIdx.x] = t;
    }
}

// cs .. ri: one word per read (n_units, or 2 n_units with pairs); rs / re / ri all NULL or all given; used: n_amp zeroed
// words; totals: kAcCounts words; partials: ac_partial_rows() rows.  With pairs every column must be 8-byte aligned.
uint32_t ac_partial_rows() { return 2048; }
void launch_amplicon_clip(hipStream_t st, bool pairs, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                          const uint32_t* seq_lengths, const uint32_t* qualities, uint64_t n_units,
                          const uint32_t* lengths, uint32_t n_contigs, const uint32_t* amp_offs, const uint32_t* tab,
                          uint32_t n_amp, uint32_t min_length, uint32_t min_mapq, bool per_amplicon, uint32_t* label,
                          uint64_t* unit_keep, uint32_t* cs, uint32_t* ce, uint32_t* ci, uint32_t* rs, uint32_t* re,
                          uint32_t* ri, uint32_t* used, uint64_t* partials, uint64_t* totals, uint32_t* err) {
    uint32_t n_blocks = 0;
    if (n_units) {
        n_blocks = grid_for(((n_units + 63) / 64) * 64, 256);
        const dim3 grid(n_blocks), block(256);
        const bool lds = n_amp <= kAcLdsMax;
        const size_t shm = lds ? 6 * (size_t)n_amp * sizeof(uint32_t) : 0;
        const uint32_t pa = per_amplicon ? 1u : 0u;
#define QMCP_AC_LAUNCH(P, L)                                                                                           \
    hipLaunchKernelGGL((k_amplicon_clip<P, L>), grid, block, shm, st, starts, ends, ids, seq_lengths, qualities, n_units, \
                       lengths, n_contigs, amp_offs, tab, n_amp, min_length, min_mapq, pa, label, unit_keep, cs, ce, ci, \
                       rs, re, ri, used, partials, err)
        if (pairs && lds) QMCP_AC_LAUNCH(true, true);
        else if (pairs) QMCP_AC_LAUNCH(true, false);
        else if (lds) QMCP_AC_LAUNCH(false, true);
        else QMCP_AC_LAUNCH(false, false);
#undef QMCP_AC_LAUNCH
    }
    hipLaunchKernelGGL(k_ac_totals, dim3(1), dim3(256), 0, st, partials, n_blocks, used, n_amp, totals);
}
