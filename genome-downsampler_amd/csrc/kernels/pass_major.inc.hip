// pass_major.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp).
// ------------------------------------------------------------------ range-ranked route, pass-major layout
// The range-ranked route (ranked_route.inc.hip) needs the reads grouped by position range, in read-index order
// inside a range.  Its first form reads the reads twice before it can write them -- k_prepare (histogram of every
// pass of 8 192 reads), a scan of the histograms, k_range_partition (re-reads the starts, writes 6 B per read to
// where the scan says) -- because a range-major array needs every pass's counts before the first record can be
// placed.  Here the grouped array is never materialised (host model with every index asserted in bounds:
// tests/pass_major_model.py, tests/test_pass_major_model.py):
//   k_pm_prepare_sort   ONE pass over the reads (8 B per read in): validate, span statistics, clear the keep mask,
//                       sort every pass of 8 192 reads by range; the pass's records of range d -- its SLICE (d, P) --
//                       leave as two 16-bit streams (position inside the range, read index inside the pass: 4 B per
//                       read) at a slot that is a multiple of 64: pass P owns the slots [P stride, (P + 1) stride),
//                       stride = 8192 + 64 n_ranges, the slices follow each other padded to whole groups of 64 slots.
//                       Two tables laid out [range][pass]: the slice's record count rounded up to a multiple of 64, and
//                       (first slot - P stride) / 64 | true count << 16.  The stable rank inside a pass comes from per-lane
//                       counts where the pass's digits span at most 32 ranges (pm_lane_rank.inc.hip; every pass of
//                       cfg4), from part_rank_rounds' ballots otherwise: the same ranks, so the same buffers.
//                       Such a pass of the unfiltered producer (at most 32 slices, whichever form ranked it) is staged in
//                       LDS in the padded layout it has in memory -- a record at its slice's padded base plus its rank --
//                       and the stage's words [0, padded total) leave as ONE flat run to the slots from P stride on: two
//                       16-byte LDS reads and one 16-byte store a stream per thread and step, a wave's store 1 KB, no
//                       compare, no readlane, no loop over slices; the padding inside a group receives whatever the
//                       stage held (the consumers mask by the record count), nothing beyond the padded total is written
//                       (tests/pm_flat_writeout_model.py restates it on the host).  Other passes and the filtered
//                       producer stage unpadded and go out slice by slice, two slices a wave at a time.
//   k_pm_row_sums,      exclusive scan over the padded count table in two launches (partial sums of the rows' parts, then
//   k_pm_tables         every part scanned from a base it derives itself): Tp[d][P] = the PADDED FLAT position of the slice --
//                       range d's records in read-index order are its slices in pass order, each padded to whole
//                       groups, so a group of 64 padded flat positions (a WAVE-SLOT) lies in exactly one slice.
//   k_pm_tables         the same launch, one thread per table entry: one descriptor word per wave-slot -- pass << 15 |
//                       slot group inside the pass << 6 | (records in the group - 1) --; from the rows' true record counts
//                       the ranges' true flat starts -- the bucket offsets' bases -- and the heaviest load.
//   k_pm_offsets        per range: LDS histogram of its wave-slots' positions -> bucket offsets (k_range_offsets' job);
//                       eight position requests a wave in flight, the next round's descriptors asked for behind them.
//   k_pm_walk           per range: k_rank_mark's ordered walk, a chunk of sixteen wave-slots per step, each wave's
//                       records found through ONE descriptor word (round 3 searched the table's row with a cursor in
//                       LDS: 57 vector instructions per wave and chunk against the range-major walk's 21).  Kept
//                       records' read indices collect in a ring in LDS, per wave, and are marked 64 at a time.
//                       The (chunk, position) groups whose quota ran out inside a chunk are listed and settled in the
//                       kernel's tail, one wave per group, by the workgroup that listed them.
// THE RANGE GRID (pm_grid_plan.h; the host decides before anything is queued).  A range is 2^shift positions of an axis
// the starts are laid on.  On the genome's global axis every contig border falls inside a range, and a range that
// straddles one gets two slices per pass pair, each padded to whole groups of 64: the same records in more wave-slots.
// k_pm_offsets and k_pm_walk run one workgroup per range, a single wave of workgroups on the chip, so they take as long
// as their heaviest range: at cfg4 (8 contigs of 10^6, 245 ranges of 32 768) the seven straddling ranges, 8 506
// wave-slots against a median near 7 300.  The ALIGNED grid lays contig c at (rbase[c] << shift), rbase[c] = the ranges
// of the contigs before it: no range straddles a border -- 248 ranges, the heaviest 7 322 wave-slots (-14 %), k_pm_walk
// 0.275 -> 0.250 ms.  It is taken where its ranges still fit the 256 digits and the heaviest range's expected wave-slots
// come out strictly lighter (options.pm_grid forces either).  To the kernels both grids are the same tables: the
// producer adds vbase[c] in place of the contig's global offset; the per-range kernels take the real position of key 0
// (pos0), the positions that exist (live) and the range's contig from the table.  boff[ltot], the grand total, is no
// range's position and is written apart.
// A range's records in read-index order are its slices in pass order, so nothing about the selection changes: the
// kept set is bit for bit the first form's, under either grid.  One-level genomes only (<= 256 ranges); longer ones keep the two-level
// partition, and so do calls whose slices would be short (narrow ranges: the padding would be most of a group).
static constexpr int kPmPass = 8192;             // reads per pass
// slots between the beginnings of two passes: the pass's records and up to 63 slots of padding per range
__host__ __device__ inline uint32_t pm_stride_of(uint32_t n_ranges) { return (uint32_t)kPmPass + 64u * n_ranges; }
static constexpr int kPmThreads = 512;           // 8 waves: wave w owns records [1024 w, 1024 (w + 1)) of the pass
static constexpr int kPmWaves = kPmThreads / 64;
static constexpr int kPmPassesPerWg = 4;         // a workgroup's passes leave their table entries as 16-byte runs
static constexpr size_t kPmSortLds = ((size_t)kPmPass + kPmWaves * 256 + 2 * 256 + 16 + 2 * kPmPassesPerWg * 256 + kPmWaves * 3 * 128) * sizeof(uint32_t);
static constexpr uint32_t kPmExcPerWave = 128;  // list slots per wave and pass: an eighth of the wave's 1 024 reads

// The flat write-out (below): a pass of at most kPmFlatDigits slices is staged padded and leaves as one run.
static constexpr uint32_t kPmFlatDigits = 32;
static constexpr uint32_t kPmStageWords = 10240;
static constexpr uint32_t kPmFlatSlots = 8;   // slots a thread copies per step: 16 bytes a stream (8-byte stores of 4 slots: 0.280 against 0.277 ms)
static_assert(kPmStageWords >= (uint32_t)kPmPass + kPmFlatDigits * 63u, "a padded pass of 32 slices fits the stage");
static_assert(kPmStageWords <= (uint32_t)kPmPass + kPmWaves * 3u * kPmExcPerWave, "the stage's tail aliases s_exc and nothing else");
static_assert(kPmFlatDigits == 1u << kPmLaneFormBits, "a pass the lane counts rank is a pass the flat write-out takes");

#ifndef QMCP_PM_MIN_WAVES
#define QMCP_PM_MIN_WAVES 4  // waves per SIMD the register allocation aims at (6 -- three workgroups per CU -- spills: 0.42 against 0.29 ms)
#endif
__global__ __launch_bounds__(kPmThreads, QMCP_PM_MIN_WAVES) void k_pm_prepare_sort(
    const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends, uint32_t n,
    const uint64_t* __restrict__ contig_read_off, const uint64_t* __restrict__ contig_pos_off, uint32_t n_contigs,
    const uint32_t* __restrict__ vbase /* [n_contigs + 1] where a contig begins on the grid's axis (pm_grid_plan.h) */,
    uint32_t shift, uint32_t stride /* pm_stride_of(ranges of the grid) */,
    uint16_t* __restrict__ keys16, uint16_t* __restrict__ idx16,
    uint32_t* __restrict__ cnt_tab, uint32_t* __restrict__ lst_tab, uint32_t pitch /* multiple of 4 */,
    uint32_t* __restrict__ stats, unsigned long long* __restrict__ zero_mask,
    // near-uniform route (kernels/near_uniform.inc.hip): reads whose span is not ell_reg are left out of the sorted
    // passes and listed instead -- {global start, global end, read index}, three arrays of exc_cap words.  Every wave
    // of every pass owns kPmExcPerWave slots of the list (pass P, wave w: from (8 P + w) * 128) and says how many it
    // filled in exc_cnt[8 P + w]: no counter is shared (24 k same-address atomics, one per wave, took longer than
    // the whole kernel: 0.32 -> 0.69 ms); k_nu_count_groups adds the groups up into stats[4] afterwards.  stats[5]
    // is set if a wave met more than its slots hold (the list is then incomplete).  ell_reg == 0: every read is regular.
    uint32_t ell_reg, uint32_t* __restrict__ exc, uint32_t exc_cap, uint32_t* __restrict__ exc_cnt) {
    extern __shared__ uint32_t s_pm[];
    // A pass's records, sorted: key | index in pass << 16.  Back to back where the pass leaves slice by slice (8 192
    // words); in the padded layout it has in memory -- every slice from a multiple of 64 -- where it leaves as one flat
    // run (at most 32 slices: up to 63 words of padding each).  The words past 8 192 are the filtered producer's
    // exception corner: the filter never takes the flat form, so the two never meet.
    uint32_t* s_stage = s_pm;                           // [10240], the last 2 048 aliased by s_exc
    uint32_t* s_exc = s_stage + kPmPass;                // [8][128][3] every wave's exceptions of the pass, until the pass is written out
    uint32_t* s_cnt = s_exc + kPmWaves * 3 * kPmExcPerWave;  // [8][256] per-wave digit counts, then offsets
    uint32_t* s_gbase = s_cnt + kPmWaves * 256;         // [256] where a digit's records begin inside the sorted pass
    uint32_t* s_pbase = s_gbase + 256;                  // [256] ... and where its slice begins inside the pass's slots (padded)
    uint32_t* s_wave = s_pbase + 256;                   // [16]
    uint32_t* s_tabc = s_wave + 16;                     // [4][256] the workgroup's table entries
    uint32_t* s_tabl = s_tabc + kPmPassesPerWg * 256;   // [4][256]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t mn = 0xFFFFFFFFu, mx = 0, bad = 0;
    auto contig_of = [&](uint32_t i) {
        uint32_t lo = 0, hi = n_contigs;  // last c with roff[c] <= i
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (contig_read_off[mid] <= i) lo = mid; else hi = mid;
        }
        return lo;
    };
    // A pass's contigs and the digits they span.  Which lane owns which read (below) follows from them, so they are
    // worked out a pass ahead, behind the loads of the pass before; only the workgroup's first pass waits for them.
    struct PassForm { uint32_t c_first, c_last, match_bits, d_lo, d_hi; };
    auto form_of = [&](uint32_t base, uint32_t count) {
        PassForm f;
        f.c_first = n_contigs > 1 ? contig_of(base) : 0u;
        f.c_last = n_contigs > 1 ? contig_of(base + count - 1) : 0u;
        // the pass's digits lie in the ranges its contigs span on the grid's axis: from the first contig's first
        // position to the last one's last
        const uint32_t len_last = (uint32_t)(contig_pos_off[f.c_last + 1] - contig_pos_off[f.c_last]);
        f.d_lo = (vbase[f.c_first] >> shift) & 255u;
        f.d_hi = ((vbase[f.c_last] + (len_last ? len_last - 1u : 0u)) >> shift) & 255u;
        f.match_bits = f.d_hi >= f.d_lo ? 32u - (uint32_t)__builtin_clz((f.d_hi - f.d_lo) | 1u) : 8u;
        if (f.d_hi == f.d_lo) f.match_bits = 0;
        // (uniform by construction; carried from pass to pass in scalar registers)
        f.c_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)f.c_first);
        f.c_last = (uint32_t)__builtin_amdgcn_readfirstlane((int)f.c_last);
        f.d_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)f.d_lo);
        f.d_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)f.d_hi);
        f.match_bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)f.match_bits);
        return f;
    };
    // Ranking by per-lane counts (pm_lane_rank.inc.hip) serves the unfiltered producer -- the filter's exception lists
    // are in read-index order per wave under the strided ownership -- and loads 16 bytes a lane.
    const bool lane_form_ok = ell_reg == 0u && (((uintptr_t)starts | (uintptr_t)ends) & 15u) == 0u;
    PassForm next_form = {0u, 0u, 0u, 0u, 0u};
    {
        const uint64_t base0 = (uint64_t)blockIdx.x * kPmPassesPerWg * kPmPass;
        if (base0 < n) next_form = form_of((uint32_t)base0, min((uint32_t)kPmPass, n - (uint32_t)base0));
    }
    for (int g = 0; g < kPmPassesPerWg; ++g) {
        const uint32_t P = blockIdx.x * kPmPassesPerWg + g;
        const uint64_t base64 = (uint64_t)P * kPmPass;
        if (base64 >= n) {  // (uniform) a pass beyond the reads: zero table entries, the scan runs over the padding too
            if (threadIdx.x < 256) { s_tabc[g * 256 + threadIdx.x] = 0; s_tabl[g * 256 + threadIdx.x] = 0; }
            if (ell_reg != 0u && lane == 0 && P < pitch) exc_cnt[P * kPmWaves + w] = 0;
            continue;
        }
        const uint32_t base = (uint32_t)base64;
        const uint32_t count = min((uint32_t)kPmPass, n - base);
        const uint32_t wbase = base + w * (kSortItems * 64);
        const PassForm form = next_form;
        const uint32_t c_first = form.c_first, c_last = form.c_last, match_bits = form.match_bits;
        // (uniform) who owns which read of the wave's 1 024: lane l the sixteen consecutive reads from 16 l on, where the
        // pass is ranked by per-lane counts; otherwise the reads l, l + 64, ...: the thread's k-th read is lane0 + k kstep
        const bool blocked = lane_form_ok && match_bits <= kPmLaneFormBits;
        const uint32_t lane0 = wbase + (blocked ? 16u * (uint32_t)lane : (uint32_t)lane);
        const uint32_t kstep = blocked ? 1u : 64u;
        // (uniform) the pass is staged padded and leaves as one flat run: at most 32 slices (match_bits <= 5 is
        // d_lo <= d_hi <= d_lo + 31), whichever form ranks it; the filter keeps its corner of the stage
#ifdef QMCP_PM_LAB_SLICE_WRITEOUT
        const bool flat = false;  // (lab build only: the slice-by-slice write-out for every pass, to time against)
#else
        const bool flat = ell_reg == 0u && match_bits <= kPmLaneFormBits;
#endif
        // all of the pass's loads first (32 in flight per thread; eight of 16 bytes under the blocked ownership, where
        // a lane's reads are 64 contiguous bytes of each array -- they read at the rate of the coalesced dwords)
        Rec rec[kSortItems];  // key: start, then global start; val: end
        if (blocked && count == (uint32_t)kPmPass) {  // (uniform)
            // (a vector type of the language, not uint4: that one is a struct, its load is split into four words
            //  before the two branches meet, and the branches' word loads are then merged into one run of 32)
            const PmQuad* const s4 = reinterpret_cast<const PmQuad*>(starts + lane0);
            const PmQuad* const e4 = reinterpret_cast<const PmQuad*>(ends + lane0);
#pragma unroll
            for (int q = 0; q < kSortItems / 4; ++q) {
                const PmQuad s = s4[q], e = e4[q];
                rec[4 * q].key = s.x; rec[4 * q + 1].key = s.y; rec[4 * q + 2].key = s.z; rec[4 * q + 3].key = s.w;
                rec[4 * q].val = e.x; rec[4 * q + 1].val = e.y; rec[4 * q + 2].val = e.z; rec[4 * q + 3].val = e.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kSortItems; ++k) {
                const uint32_t i = min(lane0 + k * kstep, n - 1);  // clamped: every lane loads
                rec[k].key = starts[i];
                rec[k].val = ends[i];
            }
        }
        for (int i = threadIdx.x; i < kPmWaves * 256; i += kPmThreads) s_cnt[i] = 0;
        // the pass's 128 words of the keep mask are cleared here (saves a memset launch)
        if (zero_mask && threadIdx.x < 128 && P * 128u + threadIdx.x < (n + 63u) / 64u) zero_mask[P * 128u + threadIdx.x] = 0ull;
        if (g + 1 < kPmPassesPerWg && base64 + kPmPass < n)
            next_form = form_of(base + kPmPass, min((uint32_t)kPmPass, n - base - (uint32_t)kPmPass));
        uint32_t skip = 0;  // bit k: the thread's k-th read is an exception (near-uniform route)
        uint32_t filled = 0;  // (uniform) exceptions of the pass this wave has met
        // An exception is put aside the moment it is recognised (its end is then dead: kept until later, the sixteen
        // ends cost sixteen registers and the kernel spilled), in the wave's own corner of LDS, and goes to the list
        // when the pass is written out -- a store to memory here would have to be drained at the next barrier.
        // (an LDS-qualified pointer: through a generic one the three stores become flat_ stores, which wait for the
        //  pass's thirty-two loads in flight -- 1 us per wave-round that holds an exception, 0.32 -> 0.69 ms)
        typedef __attribute__((address_space(3))) uint32_t LdsWord;
        LdsWord* const mine = (LdsWord*)(s_exc + w * (3 * kPmExcPerWave));
        auto put_aside = [&, mine](int k, bool isx, uint32_t gs, uint32_t ge, uint32_t i) {
            const uint64_t m = __ballot(isx);
            if (m != 0ull) {  // (uniform)
                const uint32_t slot = filled + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (isx) {
                    skip |= 1u << k;
                    if (slot < kPmExcPerWave) { mine[3u * slot] = gs; mine[3u * slot + 1u] = ge; mine[3u * slot + 2u] = i; }
                    else nu_overflow_put(exc, exc_cap, stats, gs, ge, i);  // (more than the wave's slots hold: the overflow region)
                }
                filled += (uint32_t)__popcll(m);
            }
        };
        // validate, span range, start on the grid's axis (a start beyond its contig -- the call fails -- is taken as
        // the contig's last position, so that its digit lies inside the pass's digit interval)
        if (c_first == c_last) {
            const uint32_t p0 = (uint32_t)contig_pos_off[c_first];
            const uint32_t len = (uint32_t)contig_pos_off[c_first + 1] - p0;
            const uint32_t v0 = vbase[c_first];
            const uint32_t last = len ? len - 1u : 0u;
#pragma unroll
            for (int k = 0; k < kSortItems; ++k) {
                const uint32_t i = lane0 + k * kstep;
                const uint32_t s = rec[k].key, e = rec[k].val;
                bool isx = false;
                if (i < n) {
                    bad |= (s > e || e >= len) ? 1u : 0u;
                    const uint32_t span = e - s + 1;
                    mn = min(mn, span);
                    mx = max(mx, span);
                    isx = span != ell_reg;
                }
                rec[k].key = v0 + min(s, last);
                if (ell_reg != 0u) put_aside(k, isx, p0 + min(s, last), p0 + min(e, last), i);  // (the list holds global positions)
            }
        } else {
#pragma unroll
            for (int k = 0; k < kSortItems; ++k) {
                const uint32_t i = lane0 + k * kstep;
                bool isx = false;
                uint32_t gs = 0, ge = 0;
                if (i < n) {
                    const uint32_t cc = contig_of(i);
                    const uint32_t p0 = (uint32_t)contig_pos_off[cc];
                    const uint32_t len = (uint32_t)contig_pos_off[cc + 1] - p0;
                    const uint32_t s = rec[k].key, e = rec[k].val;
                    bad |= (s > e || e >= len) ? 1u : 0u;
                    const uint32_t span = e - s + 1;
                    mn = min(mn, span);
                    mx = max(mx, span);
                    rec[k].key = vbase[cc] + min(s, len ? len - 1u : 0u);
                    isx = span != ell_reg;
                    gs = p0 + min(s, len ? len - 1u : 0u);
                    ge = p0 + min(e, len ? len - 1u : 0u);
                }
                if (ell_reg != 0u) put_aside(k, isx, gs, ge, i);
            }
        }
        __syncthreads();  // (counters cleared)
        uint32_t rank[kSortItems];
        {
            uint32_t* const s_cnt_w = s_cnt + w * 256;
            const uint32_t bound = base + count;
#ifdef QMCP_PM_LAB_NO_RANK
            // (lab build only: the producer without its ranking, to time against.  A record's rank is its lane's own
            //  index, every digit of the interval is said to hold 32 records a wave: every index stays inside the
            //  stage and the pass's slots, the buffers are not the model's and only the producer may run on them)
            if (blocked) {
#pragma unroll
                for (int k = 0; k < kSortItems; ++k) rank[k] = (uint32_t)lane & 31u;
                if (lane < 32 && form.d_lo + (uint32_t)lane < 256u) s_cnt_w[form.d_lo + (uint32_t)lane] = 32u;
            } else
#endif
            if (blocked) {  // uniform
                PmLdsWord* const s_w = (PmLdsWord*)(s_stage + w * (kSortItems * 64));
                const uint32_t n_pairs = (form.d_hi - form.d_lo) / 2u + 1u;
                if (count == (uint32_t)kPmPass) pm_rank_lane_counts<true>(rec, rank, lane0, bound, shift, form.d_lo, n_pairs, lane, s_w, s_cnt_w);
                else pm_rank_lane_counts<false>(rec, rank, lane0, bound, shift, form.d_lo, n_pairs, lane, s_w, s_cnt_w);
            } else switch (match_bits) {  // uniform
                case 0: part_rank_rounds<0>(rec, rank, wbase, bound, shift, lane, s_cnt_w, skip); break;
                case 1: part_rank_rounds<1>(rec, rank, wbase, bound, shift, lane, s_cnt_w, skip); break;
                case 2: part_rank_rounds<2>(rec, rank, wbase, bound, shift, lane, s_cnt_w, skip); break;
                case 3: part_rank_rounds<3>(rec, rank, wbase, bound, shift, lane, s_cnt_w, skip); break;
                case 4: part_rank_rounds<4>(rec, rank, wbase, bound, shift, lane, s_cnt_w, skip); break;
                case 5: part_rank_rounds<5>(rec, rank, wbase, bound, shift, lane, s_cnt_w, skip); break;
                case 6: part_rank_rounds<6>(rec, rank, wbase, bound, shift, lane, s_cnt_w, skip); break;
                case 7: part_rank_rounds<7>(rec, rank, wbase, bound, shift, lane, s_cnt_w, skip); break;
                default: part_rank_rounds<8>(rec, rank, wbase, bound, shift, lane, s_cnt_w, skip); break;
            }
        }
        __syncthreads();
        if (threadIdx.x < 256) {
            // digit d = threadIdx.x: its total over the waves, then (below) where it begins inside the sorted pass and
            // where its slice -- padded to whole groups of 64 slots -- begins inside the pass's slots
            const uint32_t d = threadIdx.x;
            uint32_t tot = 0;
#pragma unroll
            for (int x = 0; x < kPmWaves; ++x) tot += s_cnt[x * 256 + d];
            const uint32_t ptot = (tot + 63u) & ~63u;
            const uint32_t inc = wave_incl_scan_add(tot);
            const uint32_t pinc = wave_incl_scan_add(ptot);
            if (lane == 63) { s_wave[w] = inc; s_wave[8 + w] = pinc; }
            s_gbase[d] = inc - tot;  // exclusive inside the wave; completed after the barrier
            s_pbase[d] = pinc - ptot;
            s_tabc[g * 256 + d] = ptot;
            s_tabl[g * 256 + d] = tot << 16;
        }
        __syncthreads();
        if (threadIdx.x < 256) {
            const uint32_t d = threadIdx.x;
            uint32_t wave_base = 0, pwave_base = 0;
            for (int x = 0; x < w; ++x) { wave_base += s_wave[x]; pwave_base += s_wave[8 + x]; }
            const uint32_t tile_off = s_gbase[d] + wave_base;
            const uint32_t ptile_off = s_pbase[d] + pwave_base;
            uint32_t run = flat ? ptile_off : tile_off;  // (the stage is padded where the pass leaves flat)
#pragma unroll
            for (int x = 0; x < kPmWaves; ++x) { const uint32_t cx = s_cnt[x * 256 + d]; s_cnt[x * 256 + d] = run; run += cx; }
            s_gbase[d] = tile_off;
            s_pbase[d] = ptile_off;
            s_tabl[g * 256 + d] |= ptile_off >> 6;   // (< 2^16: a pass has at most 8192 / 64 + 256 slot groups)
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kSortItems; ++k) {
            const uint32_t i = lane0 + k * kstep;
            if (i < n && !((skip >> k) & 1u)) {
                const uint32_t d = (rec[k].key >> shift) & 255u;
                const uint32_t local = i - base;  // < 8192
                s_stage[s_cnt[w * 256 + d] + rank[k]] = (rec[k].key & ((1u << shift) - 1u)) | (local << 16);
            }
        }
        __syncthreads();
        // out, slice by slice: wave w takes the digits w, w + 8, ..., two at a time -- one per half-wave --, four records
        // per lane and store (8 bytes of positions, 8 of indices: slices begin at multiples of 64 slots, so every store is
        // aligned and a half-wave's store is one 256-byte run)
        if (flat) {  // uniform
            // ... or flat: the stage already is the pass's slots [P stride, P stride + ptot), padding and all, so every
            // thread copies runs of eight consecutive slots -- two aligned 16-byte LDS reads, the low halves to the
            // positions, the high halves to the indices, 16 bytes a stream: a wave's store is one 1 KB run.  ptot, the
            // pass's padded total, is a multiple of 64 and P stride one too: nothing at or beyond ptot is written.  The
            // padding inside a group receives what the stage held (the consumers mask by the record count).
            const uint32_t ptot = s_wave[8] + s_wave[9] + s_wave[10] + s_wave[11];  // (the digit threads' four waves)
            const PmLdsQuad* const st4 = (const PmLdsQuad*)s_stage;
            uint16_t* const kout = keys16 + (size_t)P * stride;
            uint16_t* const iout = idx16 + (size_t)P * stride;
            for (uint32_t s = kPmFlatSlots * threadIdx.x; s < ptot; s += kPmFlatSlots * kPmThreads) {
                const PmQuad a = st4[s >> 2], b = st4[(s >> 2) + 1u];
                const PmQuad kq = {(a.x & 0xFFFFu) | (a.y << 16), (a.z & 0xFFFFu) | (a.w << 16), (b.x & 0xFFFFu) | (b.y << 16), (b.z & 0xFFFFu) | (b.w << 16)};
                const PmQuad iq = {(a.x >> 16) | (a.y & 0xFFFF0000u), (a.z >> 16) | (a.w & 0xFFFF0000u), (b.x >> 16) | (b.y & 0xFFFF0000u), (b.z >> 16) | (b.w & 0xFFFF0000u)};
#ifndef QMCP_PM_LAB_NO_STORE  // (lab build only: the producer without its stores, to time against)
                *reinterpret_cast<PmQuad*>(kout + s) = kq;
                *reinterpret_cast<PmQuad*>(iout + s) = iq;
#else
                (void)kout; (void)iout; (void)kq; (void)iq;
#endif
            }
        } else {
            const uint32_t my_d = (uint32_t)w + 8u * ((uint32_t)lane & 31u);
            const uint32_t my_tot = lane < 32 ? s_tabl[g * 256 + my_d] >> 16 : 0u;
            const uint32_t my_gb = s_gbase[my_d], my_pb = s_pbase[my_d];
            const bool upper = lane >= 32;
            const uint32_t hl = (uint32_t)lane & 31u;
            uint64_t todo = __ballot(my_tot != 0u);
            while (todo != 0ull) {  // uniform
                const int l0 = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                int l1 = l0;
                bool two = false;
                if (todo != 0ull) { l1 = __builtin_ctzll(todo); todo &= todo - 1ull; two = true; }
                const uint32_t cnt0 = (uint32_t)__builtin_amdgcn_readlane((int)my_tot, l0);
                const uint32_t cnt1 = two ? (uint32_t)__builtin_amdgcn_readlane((int)my_tot, l1) : 0u;
                const uint32_t cnt = upper ? cnt1 : cnt0;
                const uint32_t gb = upper ? (uint32_t)__builtin_amdgcn_readlane((int)my_gb, l1) : (uint32_t)__builtin_amdgcn_readlane((int)my_gb, l0);
                const uint32_t pb = upper ? (uint32_t)__builtin_amdgcn_readlane((int)my_pb, l1) : (uint32_t)__builtin_amdgcn_readlane((int)my_pb, l0);
                const size_t out0 = (size_t)P * stride + pb;
                const uint32_t most = max(cnt0, cnt1);
                for (uint32_t j0 = 0; j0 < most; j0 += 128u) {  // uniform
                    const uint32_t j = j0 + 4u * hl;
                    if (j < cnt) {
                        const uint32_t v0 = s_stage[gb + j];
                        const uint32_t v1 = j + 1 < cnt ? s_stage[gb + j + 1] : 0u;
                        const uint32_t v2 = j + 2 < cnt ? s_stage[gb + j + 2] : 0u;
                        const uint32_t v3 = j + 3 < cnt ? s_stage[gb + j + 3] : 0u;
#ifndef QMCP_PM_LAB_NO_STORE  // (lab build only: the producer without its stores, to time against)
                        *reinterpret_cast<uint2*>(keys16 + out0 + j) = make_uint2((v0 & 0xFFFFu) | (v1 << 16), (v2 & 0xFFFFu) | (v3 << 16));
                        *reinterpret_cast<uint2*>(idx16 + out0 + j) = make_uint2((v0 >> 16) | (v1 & 0xFFFF0000u), (v2 >> 16) | (v3 & 0xFFFF0000u));
#endif
                    }
                }
            }
        }
        if (ell_reg != 0u) {
            const size_t slot0 = ((size_t)P * kPmWaves + w) * kPmExcPerWave;
            for (uint32_t r = (uint32_t)lane; r < min(filled, kPmExcPerWave); r += 64u) {
                exc[slot0 + r] = mine[3u * r];
                exc[exc_cap + slot0 + r] = mine[3u * r + 1u];
                exc[2 * (size_t)exc_cap + slot0 + r] = mine[3u * r + 2u];
            }
            if (lane == 0) {
                exc_cnt[P * kPmWaves + w] = min(filled, kPmExcPerWave);
            }
        }
        __syncthreads();  // (the next pass clears the counters and re-fills the stage)
    }
    __syncthreads();
    if (threadIdx.x < 256) {
        // [digit][pass] tables: the workgroup's four passes are one aligned 16-byte run of the digit's row
        const uint32_t P0 = blockIdx.x * kPmPassesPerWg;
        if (P0 < pitch) {
            uint4 a, b;
            a.x = s_tabc[threadIdx.x]; a.y = s_tabc[256 + threadIdx.x]; a.z = s_tabc[512 + threadIdx.x]; a.w = s_tabc[768 + threadIdx.x];
            b.x = s_tabl[threadIdx.x]; b.y = s_tabl[256 + threadIdx.x]; b.z = s_tabl[512 + threadIdx.x]; b.w = s_tabl[768 + threadIdx.x];
            *reinterpret_cast<uint4*>(cnt_tab + (size_t)threadIdx.x * pitch + P0) = a;
            *reinterpret_cast<uint4*>(lst_tab + (size_t)threadIdx.x * pitch + P0) = b;
        }
    }

    // statistics: block reduction, at most one atomic per statistic per workgroup (k_prepare)
    __shared__ uint32_t s_red[3][kPmWaves];
    mn = wave_min_u32(mn);
    mx = wave_max_u32(mx);
    bad = wave_max_u32(bad);
    if (lane == 0) { s_red[0][w] = mn; s_red[1][w] = mx; s_red[2][w] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int x = 1; x < kPmWaves; ++x) { mn = min(mn, s_red[0][x]); mx = max(mx, s_red[1][x]); bad |= s_red[2][x]; }
        if (mn < __hip_atomic_load(&stats[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&stats[0], mn);
        if (mx > __hip_atomic_load(&stats[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&stats[1], mx);
        if (bad) atomicOr(&stats[2], 1u);
    }
}

// The table stage's working words: per (range, part of the row) the part's padded and true record counts -- written by
// k_pm_row_sums with plain stores (every word every call: nothing to clear), read whole by every k_pm_tables workgroup.
static constexpr uint32_t kPmDescrY = 8;  // workgroups per range
static constexpr uint32_t kPmWorkWords = 256u * kPmDescrY * 2u;

// A wave-slot's descriptor: pass << 15 | slot group inside the pass << 6 | (records - 1).  (2^17 passes: 2^30 reads; 512
// slot groups: a pass holds at most 8192 / 64 + 256.)
struct PmSlot { uint32_t slot0, nv, pass; };
// (kVector: the descriptor sits in a vector register -- the 24-bit multiply is the full-rate one there; a uniform
//  descriptor goes through the scalar unit, which has the plain multiply only)
template <bool kVector>
__device__ __forceinline__ PmSlot pm_unpack(uint32_t dsc, bool has, uint32_t stride) {
    PmSlot s;
    s.pass = dsc >> 15;
    s.slot0 = has ? (kVector ? __umul24(s.pass, stride) : s.pass * stride) + (((dsc >> 6) & 511u) << 6) : 0u;
    s.nv = has ? (dsc & 63u) + 1u : 0u;
    return s;
}

// The table stage in two launches (the launches are the only synchronisation: no flags, no look-back).  A row of the
// [range][pass] tables is cut into kPmDescrY parts; workgroup (d, y) owns part y of row d in both kernels.
__device__ __forceinline__ void pm_row_part(uint32_t pitch, uint32_t& P_beg, uint32_t& P_end) {
    const uint32_t per = (pitch + kPmDescrY - 1u) / kPmDescrY;
    P_beg = min(pitch, blockIdx.y * per);
    P_end = min(pitch, (blockIdx.y + 1u) * per);
}

// k_pm_row_sums: the part's padded record count (cnt_tab) and true record count (lst_tab >> 16) -> work[(d Y + y) 2 ..].
__global__ __launch_bounds__(256) void k_pm_row_sums(const uint32_t* __restrict__ cnt_tab, const uint32_t* __restrict__ lstw,
                                                     uint32_t pitch, uint32_t* __restrict__ work) {
    __shared__ uint32_t s_red[2][4];
    const uint32_t d = blockIdx.x;
    uint32_t P_beg, P_end;
    pm_row_part(pitch, P_beg, P_end);
    uint32_t pad = 0, tru = 0;
    for (uint32_t P0 = P_beg + threadIdx.x; P0 < P_end; P0 += 4u * 256u) {
        uint32_t c[4], w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t P = min(P0 + (uint32_t)u * 256u, P_end - 1u);  // clamped: every load is issued
            c[u] = cnt_tab[(size_t)d * pitch + P];
            w[u] = lstw[(size_t)d * pitch + P];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (P0 + (uint32_t)u * 256u < P_end) { pad += c[u]; tru += w[u] >> 16; }
    }
    pad = wave_sum_u32(pad);
    tru = wave_sum_u32(tru);
    if ((threadIdx.x & 63u) == 0u) { s_red[0][threadIdx.x >> 6] = pad; s_red[1][threadIdx.x >> 6] = tru; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t* const out = work + ((size_t)d * kPmDescrY + blockIdx.y) * 2u;
        out[0] = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
        out[1] = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
    }
}

// k_pm_tables: everything else of the stage.  Every workgroup reads all 256 x Y partial pairs (16 KB; thread t takes row
// t) and derives what it needs itself: the padded flat start of its part -- the rows before d, the parts before y --, and
// workgroup (0, 0) the ranges' true flat starts (257 entries), the heaviest range's load and the scan's grand total (and
// it clears the sixteen words of clear16: the stream orders that ahead of everything the solve's tail queues).  It
// then scans its part of the padded count table IN PLACE (tab: cnt_tab in, Tp out -- absolute padded flat coordinates,
// what an exclusive scan over the whole table gives; a thread overwrites only the entries it has read itself) and
// writes the slices' wave-slot descriptors, a thread per (range, pass) table entry.  (First forms of the descriptor
// kernel: a workgroup per 256 entries, every one ending in an atomic on one ticket word: 12 288 same-address atomics,
// 0.49 ms; one workgroup per range walking its row serially: 0.044 ms.)
__global__ __launch_bounds__(256) void k_pm_tables(uint32_t* tab, const uint32_t* __restrict__ lstw, uint32_t pitch,
                                                   uint32_t n_groups /* total padded flat / 64 bound */,
                                                   uint32_t* __restrict__ desc, const uint32_t* __restrict__ work,
                                                   uint32_t* __restrict__ range_start,
                                                   uint32_t* __restrict__ max_load /* [0] records, [1] wave-slots of the heaviest range */,
                                                   uint32_t* __restrict__ clear16 /* or null */) {
    __shared__ uint32_t s_red[4], s_red2[4], s_base, s_tile[2][4][4];
    const uint32_t d = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wv = tid >> 6;
    const bool first = d == 0u && y == 0u;  // (uniform)
    uint32_t rp = 0, rt = 0, before = 0;  // row tid: padded total, true total, padded total of its parts before y
    {
        const uint4* const src = reinterpret_cast<const uint4*>(work + (size_t)tid * kPmDescrY * 2u);
        uint4 q[kPmDescrY / 2u];
#pragma unroll
        for (uint32_t k = 0; k < kPmDescrY / 2u; ++k) q[k] = src[k];
#pragma unroll
        for (uint32_t k = 0; k < kPmDescrY / 2u; ++k) {
            if (2u * k < y) before += q[k].x;
            if (2u * k + 1u < y) before += q[k].z;
            rp += q[k].x + q[k].z;
            rt += q[k].y + q[k].w;
        }
    }
    {
        const uint32_t inc = wave_incl_scan_add(rp);
        if (lane == 63u) s_red[wv] = inc;
        __syncthreads();
        uint32_t base = 0;
        for (uint32_t x = 0; x < wv; ++x) base += s_red[x];
        if (tid == d) s_base = base + inc - rp + before;
        if (first && tid == 255u) tab[(size_t)256u * pitch] = base + inc;  // the scan's total
        __syncthreads();
    }
    if (first) {  // the ranges' true flat starts and the heaviest range's load, from the rows' true counts
        if (clear16 != nullptr && tid < 16u) clear16[tid] = 0u;  // (the solve's result scalars: saves the tail a memset launch)
        const uint32_t inc = wave_incl_scan_add(rt);
        const uint32_t mx = wave_max_u32(rt), mxp = wave_max_u32(rp);
        if (lane == 63u) s_red[wv] = inc;
        __syncthreads();
        uint32_t base = 0;
        for (uint32_t x = 0; x < wv; ++x) base += s_red[x];
        range_start[tid] = base + inc - rt;
        if (tid == 255u) range_start[256] = base + inc;
        __syncthreads();
        if (lane == 0u) { s_red[wv] = mx; s_red2[wv] = mxp; }
        __syncthreads();
        if (tid == 0) {
            max_load[0] = max(max(s_red[0], s_red[1]), max(s_red[2], s_red[3]));
            max_load[1] = max(max(s_red2[0], s_red2[1]), max(s_red2[2], s_red2[3])) >> 6;  // (a row's padded total is its wave-slots x 64)
        }
    }
    uint32_t P_beg, P_end;
    pm_row_part(pitch, P_beg, P_end);
    uint32_t carry = s_base;  // padded flat position of entry P0 of the round (uniform)
    uint32_t round = 0;
    for (uint32_t P0 = P_beg; P0 < P_end; P0 += 4u * 256u, round ^= 1u) {
        uint32_t c[4], w[4], inc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t P = P0 + (uint32_t)u * 256u + tid;
            const bool in = P < P_end;
            const size_t at = (size_t)d * pitch + min(P, P_end - 1u);  // clamped: every load is issued
            c[u] = tab[at];
            w[u] = lstw[at];
            if (!in) { c[u] = 0u; w[u] = 0u; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            inc[u] = wave_incl_scan_add(c[u]);
            if (lane == 63u) s_tile[round][u][wv] = inc[u];
        }
        __syncthreads();  // (one barrier a round: the next round writes the other half of s_tile)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            uint32_t base = carry;
            for (uint32_t x = 0; x < wv; ++x) base += s_tile[round][u][x];
            carry += s_tile[round][u][0] + s_tile[round][u][1] + s_tile[round][u][2] + s_tile[round][u][3];
            const uint32_t P = P0 + (uint32_t)u * 256u + tid;
            if (P >= P_end) continue;
            const uint32_t t = base + inc[u] - c[u];
            tab[(size_t)d * pitch + P] = t;
            const uint32_t cnt = w[u] >> 16;
            if (cnt == 0u) continue;
            const uint32_t g = t >> 6;
            const uint32_t n_ws = (cnt + 63u) >> 6;
            for (uint32_t j = 0; j < n_ws; ++j)
                if (g + j < n_groups)  // (always: the bound is the buffer's size)
                    desc[g + j] = (P << 15) | (((w[u] & 0xFFFFu) + j) << 6) | (min(64u, cnt - 64u * j) - 1u);
        }
    }
}

// The grid's per-range tables (pm_grid_plan.h), one buffer: where key 0 of range r lies in the genome, how many of the
// range's positions exist, and the range's contig (kPmNoContig where the range straddles a border).
__device__ __forceinline__ uint32_t pm_grid_pos0(const uint32_t* __restrict__ grid, uint32_t r) { return grid[r]; }
__device__ __forceinline__ uint32_t pm_grid_live(const uint32_t* __restrict__ grid, uint32_t r) { return grid[kPmGridRows + r]; }
__device__ __forceinline__ uint32_t pm_grid_contig(const uint32_t* __restrict__ grid, uint32_t r) { return grid[2u * kPmGridRows + r]; }

// Lab build only (-DQMCP_PM_STAMP, lab/build_variant.sh; read back by lab/pm_range_stamps.py): the two per-range
// kernels stamp the shader clock at their phase borders, wave 0 of every workgroup, into a buffer of their own that no
// kernel reads.  [kernel: 0 offsets, 1 walk][range][0..4 the clock at the borders, 5 set once the row is written,
// 6..7 the 100 MHz clock at entry and end: what a tick is worth].  The product build contains no stamp.
#ifdef QMCP_PM_STAMP
__device__ unsigned long long g_pm_stamps[2][kPmGridRows][8];
__device__ __forceinline__ unsigned long long pm_stamp() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    return t;
}
// ... once `dep` (a register a load writes) is there: the wait for that load comes before the stamp
__device__ __forceinline__ unsigned long long pm_stamp_after(uint32_t dep) {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "v"(dep) : "memory");
    return t;
}
__device__ __forceinline__ unsigned long long pm_stamp_real() {
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    return t;
}
#define QMCP_PM_STAMPS unsigned long long pm_t[5] = {0, 0, 0, 0, 0}; const unsigned long long pm_r0 = pm_stamp_real();
#define QMCP_PM_STAMP_AT(i) pm_t[i] = pm_stamp();
#define QMCP_PM_STAMP_AFTER(i, dep) pm_t[i] = pm_stamp_after(dep);
#define QMCP_PM_STAMPS_OUT(kernel)                                                                         \
    if (threadIdx.x == 0) {                                                                                \
        unsigned long long* const row = g_pm_stamps[kernel][blockIdx.x];                                   \
        for (int i = 0; i < 5; ++i) row[i] = pm_t[i];                                                      \
        row[5] = 1ull; row[6] = pm_r0; row[7] = pm_stamp_real();                                           \
    }
#else
#define QMCP_PM_STAMPS
#define QMCP_PM_STAMP_AT(i)
#define QMCP_PM_STAMP_AFTER(i, dep)
#define QMCP_PM_STAMPS_OUT(kernel)
#endif

#ifndef QMCP_PM_OFFSETS_REC
#define QMCP_PM_OFFSETS_REC 8  // records a lane loads at a time: 8 (16 bytes) or 4 (8 bytes)
#endif
#ifndef QMCP_PM_OFFSETS_U
#define QMCP_PM_OFFSETS_U 4  // position requests a wave keeps in flight
#endif
// k_range_offsets for the pass-major layout: the range's positions come as wave-slots, in any order.  A wave takes
// eight wave-slots at a time -- eight lanes each, eight records (16 bytes) per lane: one 1 024-byte request -- and keeps
// kU such requests in flight.  The descriptors of a round are asked for one round ahead, a word per eighth of the wave
// in one vector load, right behind the round's position requests: by the time the positions have been counted they
// are there.  The first round's descriptors are asked for before the counters are cleared and its positions half way
// through the clear (16 bytes a lane and store): the clear runs behind those two trips to memory.
// (History, cfg4, one solve alone, aligned grid.  Sixteen scalar descriptor loads by uniform index, waited for before
// the first position could be asked for: 0.086 ms.  A vector load a round ahead: 0.078.  16-byte position loads, four
// requests of eight wave-slots instead of eight of four, and the clear behind the first requests: 0.075 -> 0.070
// beside the parent on one box.  A second register set, round r + 1 asked for before round r is counted, bought
// nothing -- the sixteen waves of the workgroup run through the loop without a barrier and overlap each other's
// loads and atomics already -- and was removed: profiles/pm_range_trips.md.)
// One workgroup per range of the grid (gridDim.x); the last one also writes the grand total, boff[ltot].
__global__ __launch_bounds__(1024) void k_pm_offsets(const uint16_t* __restrict__ keys16, const uint32_t* __restrict__ desc,
                                                     const uint32_t* __restrict__ Tp, uint32_t pitch,
                                                     const uint32_t* __restrict__ range_start /* true flat starts */,
                                                     const uint32_t* __restrict__ grid,
                                                     uint32_t shift, uint32_t stride, uint32_t ltot, uint32_t* __restrict__ boff,
                                                     uint32_t* __restrict__ empty_positions) {
    extern __shared__ __align__(16) uint32_t s_cnt32[];  // [(1 << shift) padded] counters
#define PADDED(i) ((i) + ((i) >> 5))
    __shared__ uint32_t s_wsum[16], s_esum[16];
    const uint32_t range = blockIdx.x, width = 1u << shift;
    QMCP_PM_STAMPS
    QMCP_PM_STAMP_AT(0)
    const uint32_t pos0 = pm_grid_pos0(grid, range), live = pm_grid_live(grid, range);
    const uint32_t lo_p = Tp[(size_t)range * pitch], hi_p = Tp[(size_t)(range + 1) * pitch];
    const uint32_t g0 = lo_p >> 6, n_ws = (hi_p - lo_p) >> 6;
    const uint32_t lo = range_start[range];
    const uint32_t lane = threadIdx.x & 63u, nw = blockDim.x >> 6;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    constexpr int kU = QMCP_PM_OFFSETS_U;
    constexpr uint32_t kRec = QMCP_PM_OFFSETS_REC;  // 64 / kRec lanes a wave-slot, kRec wave-slots (a GROUP) a request
    static_assert(kRec == 4 || kRec == 8, "a lane loads 8 or 16 bytes");
    const uint32_t sub = lane / (64u / kRec), l_in = lane % (64u / kRec);
    const uint32_t n_groups = (n_ws + kRec - 1u) / kRec, step = (uint32_t)kU * nw;
    // the lane's wave-slots of the kU groups from q0 on: their descriptors (beyond the range's last: that one's, never used)
    uint32_t dsc[kU];
    auto ask_descriptors = [&](uint32_t q0) {
#pragma unroll
        for (int u = 0; u < kU; ++u) dsc[u] = desc[g0 + min(kRec * (q0 + (uint32_t)u * nw) + sub, n_ws - 1u)];
    };
    uint32_t v[kU][kRec / 2], nv[kU];  // a round's positions (in flight) and its wave-slots' record counts
    // round q0's positions through dsc[], then the next round's descriptors into dsc[], behind them
    auto ask_round = [&](uint32_t q0) {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const PmSlot at = pm_unpack<true>(dsc[u], kRec * (q0 + (uint32_t)u * nw) + sub < n_ws, stride);
            nv[u] = at.nv;
            const uint16_t* const src = keys16 + at.slot0 + kRec * l_in;   // (inside the slice's padded group: always readable)
            if constexpr (kRec == 4) {
                const uint2 x = *reinterpret_cast<const uint2*>(src);
                v[u][0] = x.x; v[u][1] = x.y;
            } else {
                const uint4 x = *reinterpret_cast<const uint4*>(src);
                v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w;
            }
        }
        ask_descriptors(q0 + step);  // (the last round's too: clamped, a line already read)
    };
    if (n_ws != 0u) ask_descriptors(w);
    // the clear: every word of the padded array (PADDED(width - 1) < width + width / 32, the array is one word longer)
    const uint32_t n_words = width + (width >> 5), n_vec = n_words >> 2, half = (n_vec + 1u) >> 1;
    uint4* const cnt4 = reinterpret_cast<uint4*>(s_cnt32);
    for (uint32_t i = threadIdx.x; i < half; i += blockDim.x) cnt4[i] = make_uint4(0u, 0u, 0u, 0u);
    if (w < n_groups) ask_round(w);  // (uniform)
    for (uint32_t i = half + threadIdx.x; i < n_vec; i += blockDim.x) cnt4[i] = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t i = 4u * n_vec + threadIdx.x; i < n_words; i += blockDim.x) s_cnt32[i] = 0u;
    __syncthreads();
    // v[] holds round q0, asked for; dsc[] round q0 + step's descriptors
    for (uint32_t q0 = w; q0 < n_groups; q0 += step) {
#ifdef QMCP_PM_STAMP
        if (q0 == w) QMCP_PM_STAMP_AFTER(1, v[kU - 1][kRec / 2 - 1])
#endif
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const uint32_t e = kRec * l_in;
#pragma unroll
            for (uint32_t x = 0; x < kRec / 2; ++x) {
                if (e + 2u * x < nv[u]) atomicAdd(&s_cnt32[PADDED(v[u][x] & 0xFFFFu)], 1u);
                if (e + 2u * x + 1u < nv[u]) atomicAdd(&s_cnt32[PADDED(v[u][x] >> 16)], 1u);
            }
        }
        if (q0 + step < n_groups) ask_round(q0 + step);  // (uniform)
    }
    __syncthreads();
    QMCP_PM_STAMP_AT(2)
    // counts -> bucket offsets, in place (k_range_offsets)
    const uint32_t per = width >= 1024u ? width >> 10 : 1u;  // positions per thread
    const uint32_t firstp = threadIdx.x * per;
    uint32_t sum = 0, empties = 0;
    if (firstp < width)
        for (uint32_t qq = 0; qq < per; ++qq) {
            const uint32_t cq = s_cnt32[PADDED(firstp + qq)];
            sum += cq;
            empties += (cq == 0 && firstp + qq < live) ? 1u : 0u;
        }
    const uint32_t inc = wave_incl_scan_add(sum);
    const uint32_t wv = threadIdx.x >> 6;
    if (lane == 63) s_wsum[wv] = inc;
    if (empty_positions != nullptr) {
        empties = wave_sum_u32(empties);
        if (lane == 0) s_esum[wv] = empties;
    }
    __syncthreads();
    if (empty_positions != nullptr && threadIdx.x == 0) {
        uint32_t total = 0;
        for (uint32_t x = 0; x < nw; ++x) total += s_esum[x];
        if (total != 0) atomicAdd(empty_positions, total);
    }
    uint32_t run = lo + inc - sum;
    for (uint32_t x = 0; x < wv; ++x) run += s_wsum[x];
    if (firstp < width)
        for (uint32_t qq = 0; qq < per; ++qq) {
            const uint32_t cq = s_cnt32[PADDED(firstp + qq)];
            s_cnt32[PADDED(firstp + qq)] = run;
            run += cq;
        }
    __syncthreads();
    QMCP_PM_STAMP_AT(3)
    for (uint32_t i = threadIdx.x; i < live; i += blockDim.x) boff[pos0 + i] = s_cnt32[PADDED(i)];
    // (the grand total: the ranges of the grid end where the genome does, so no range has a position ltot of its own)
    if (range == gridDim.x - 1u && threadIdx.x == 0) boff[ltot] = range_start[kPmGridRows];
    QMCP_PM_STAMP_AT(4)
    QMCP_PM_STAMPS_OUT(0)
#undef PADDED
}

// Where the quotas come from when the event-driven sweep ran whole contigs (no stretch table): the kept count of
// position p is sev[p - (k - lastns[k]) * ell], k its block -- what k_sweep_expand would write into selend[] for the
// ranking to read back (30 us and 100 MB a solve; here the ranking reads the sweep's own output).
// (div: ell's multiply-and-shift constants, computed by the launcher -- pm_div.h)
struct EvQuota { const uint32_t* sev; const uint32_t* lastns; const uint64_t* poff; uint32_t n_contigs, ell; PmDiv div; };

// The walk's quotas straight from the event-driven sweep's output: two dependent loads per position -- the block's
// distance to the block that holds its value (lastns), then the value (sev) -- kQ positions of a thread in flight: at
// kQ = 16 a range of 32 Ki positions takes two rounds (eight in flight and a divide per position: 16.5 us from the
// kernel's entry to its first draw at cfg4; sixteen and the multiply: 8.1 - 9.7; all 32 in one round: no better --
// profiles/pm_range_trips.md).  The block of a position, (p - base) / ell, is a multiply and a shift by the
// launcher's constants (pm_div.h).  kOne: the range lies in contig c_range, whose base and
// row of lastns[] are uniform; else every position's contig is looked up.
template <int kQ, bool kOne>
__device__ __forceinline__ void pm_event_quotas(const EvQuota& evq, uint32_t c_range, uint32_t pos0, uint32_t live, uint32_t tid,
                                                uint32_t nthreads, int32_t* s_q) {
    uint32_t base_u = 0, row_u = 0;
    if (kOne) {
        base_u = (uint32_t)evq.poff[c_range];
        row_u = (pm_div(base_u, evq.div) >> 2) + c_range;  // base / (4 ell) + c
    }
    for (uint32_t i0 = tid; i0 < live; i0 += kQ * nthreads) {
        uint32_t val[kQ];  // the distance in blocks, then the quota
#pragma unroll
        for (int u = 0; u < kQ; ++u) {
            const uint32_t p = pos0 + min(i0 + u * nthreads, live - 1);  // clamped: every load is issued
            uint32_t base = base_u, row = row_u;
            if (!kOne) {
                uint32_t c_lo = 0, c_hi = evq.n_contigs;  // last contig with poff[c] <= p
                while (c_hi - c_lo > 1) {
                    const uint32_t mid = (c_lo + c_hi) >> 1;
                    if ((uint32_t)evq.poff[mid] <= p) c_lo = mid; else c_hi = mid;
                }
                base = (uint32_t)evq.poff[c_lo];
                row = (pm_div(base, evq.div) >> 2) + c_lo;
            }
            const uint32_t k = pm_div(p - base, evq.div);
            val[u] = k - evq.lastns[(size_t)row * 4u + k];
        }
#pragma unroll
        for (int u = 0; u < kQ; ++u) val[u] = evq.sev[pos0 + min(i0 + u * nthreads, live - 1) - val[u] * evq.ell];
#pragma unroll
        for (int u = 0; u < kQ; ++u)
            if (i0 + u * nthreads < live) s_q[i0 + u * nthreads] = (int32_t)val[u];
    }
}

// Settling, in the walk's own tail: the listed (chunk, position) groups of the range.  The position's `skip` LAST records
// of that chunk are the ones the quota did not reach, so a wave walks the chunk's sixteen wave-slots backwards, passes
// over that many matches and keeps the rest.  The workgroup's sixteen waves deal the groups out (a few dozen per range
// at cfg4: 20 000 in all).  A group is four dependent trips to memory -- list entry, descriptors, positions, read
// indices -- and a walk of sixteen steps, so a wave overlaps them: the list entries of all its groups come in one load
// (lane j: the wave's group j), and while group j is walked the positions of group j + 1 and the descriptors of group
// j + 2 are on their way.  The read indices of a group's kept records are asked for step by step during its walk and
// marked after the NEXT group's walk: no trip per step that holds a match, none per group.  -> records kept by this
// wave (uniform).
// (This was a kernel of its own, k_pm_settle -- a second launch that loaded Tp, the range's start and a per-range group
// count again; then two groups at a time, nothing of the next two asked for: profiles/pm_range_trips.md.)
__device__ __forceinline__ uint32_t pm_settle_groups(const uint16_t* __restrict__ keys16, const uint16_t* __restrict__ idx16,
                                                     const uint32_t* __restrict__ desc, uint32_t g0, uint32_t n_ws,
                                                     uint32_t stride, const uint2* amb, uint32_t namb, uint32_t w,
                                                     uint32_t lane, unsigned long long* __restrict__ mask) {
    const uint64_t gt_mask = lane == 63 ? 0ull : ~((2ull << lane) - 1ull);  // lanes above this one
    uint32_t kept = 0;
    constexpr int kSteps = 16;
    constexpr uint32_t stride_k = 16;  // waves of the workgroup
    struct Group {
        uint32_t key[kSteps];  // lane l: the position in slot l of the chunk's wave-slot t
        uint32_t dscv;         // lane t < 16: the descriptor of the chunk's wave-slot t
        uint32_t c, p, skip;   // (uniform) the chunk, the position, matches to be passed over from the chunk's end
    };
    struct Kept {              // of a walked group: what is still to be marked
        uint32_t idx[kSteps];  // lane l: the read index inside its pass of the record in slot l of wave-slot t (asked for)
        uint32_t marked;       // steps t whose record this lane keeps
        uint32_t dscv;         // the group's descriptors (their passes)
    };
    const uint32_t mine = namb > w ? (namb - w + stride_k - 1u) / stride_k : 0u;  // (uniform) groups w, w + 16, ...
    for (uint32_t j0 = 0; j0 < mine; j0 += 64u) {
        const uint32_t nj = min(64u, mine - j0);
        const uint32_t k_lane = w + stride_k * (j0 + lane);
        const uint2 ent = k_lane < namb ? amb[k_lane] : make_uint2(0u, 0u);
        uint32_t dsc_next;  // descriptors on their way
        // (every request below is made without a condition, for the last group again where there is no further one:
        //  under a condition the compiler loads into other registers and copies, and waits for the copy's sake)
        auto ask_descriptors = [&](uint32_t j) {
            const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)ent.x, (int)min(j, nj - 1u)) >> 15;
            const uint32_t ws = 16u * c + (lane & 15u);
            dsc_next = desc[g0 + min(ws, n_ws - 1u)];  // (beyond the range's last: that one's, never used)
        };
        auto ask_positions = [&](Group& G, uint32_t j) {  // through dsc_next
            const int jj = (int)min(j, nj - 1u);
            const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)ent.x, jj);
            G.c = e >> 15;
            G.p = e & 0x7FFFu;
            G.skip = (uint32_t)__builtin_amdgcn_readlane((int)ent.y, jj);
            G.dscv = dsc_next;
#pragma unroll
            for (int t = 0; t < kSteps; ++t) {
                const uint32_t dsc = (uint32_t)__builtin_amdgcn_readlane((int)G.dscv, t);
                G.key[t] = keys16[pm_unpack<false>(dsc, 16u * G.c + (uint32_t)t < n_ws, stride).slot0 + lane];
            }
        };
        // the walk of one group: passes over `skip` matches from the chunk's end, asks for the read indices of the rest
        auto walk = [&](const Group& G, Kept& K) {
            uint32_t skip = G.skip;
            K.marked = 0u;
            K.dscv = G.dscv;
#pragma unroll
            for (int t = kSteps - 1; t >= 0; --t) {
                const uint32_t dsc = (uint32_t)__builtin_amdgcn_readlane((int)G.dscv, t);
                const PmSlot at = pm_unpack<false>(dsc, 16u * G.c + (uint32_t)t < n_ws, stride);
                const bool member = lane < at.nv && G.key[t] == G.p;
                const uint64_t m = __ballot(member);
                K.idx[t] = 0u;
                if (m == 0) continue;
                const uint32_t above = (uint32_t)__popcll(m & gt_mask);  // matches after this one in the step
                if (member && above >= skip) {
                    K.idx[t] = idx16[at.slot0 + lane];
                    K.marked |= 1u << t;
                }
                const uint32_t in_step = (uint32_t)__popcll(m);
                kept += in_step > skip ? in_step - skip : 0u;
                skip = skip > in_step ? skip - in_step : 0u;
            }
        };
        // ... and their marking, one group later: the read indices have had a walk's time to arrive
        auto mark = [&](Kept& K) {
            if (__ballot(K.marked != 0u) != 0) {
#pragma unroll
                for (int t = 0; t < kSteps; ++t)
                    if ((K.marked >> t) & 1u) {
                        const uint32_t v = ((uint32_t)__builtin_amdgcn_readlane((int)K.dscv, t) >> 15) * (uint32_t)kPmPass + K.idx[t];
                        atomicOr(&mask[v >> 6], 1ull << (v & 63u));
                    }
            }
            K.marked = 0u;
        };
        Group A, B;
        Kept KA, KB;
        KA.marked = KB.marked = 0u;
        KA.dscv = KB.dscv = 0u;
#pragma unroll
        for (int t = 0; t < kSteps; ++t) KA.idx[t] = KB.idx[t] = 0u;
        ask_descriptors(0u);
        ask_positions(A, 0u);
        ask_descriptors(1u);
        for (uint32_t j = 0; j < nj; j += 2u) {
            ask_positions(B, j + 1u);
            ask_descriptors(j + 2u);
            walk(A, KA);
            mark(KB);  // group j - 1's
            if (j + 1u >= nj) break;
            ask_positions(A, j + 2u);
            ask_descriptors(j + 3u);
            walk(B, KB);
            mark(KA);
        }
        mark(KA);
        mark(KB);
    }
    return kept;
}

// k_rank_mark's ordered walk for the pass-major layout: one workgroup (16 waves) per range, quota array q[p] = S(p) in
// LDS, the range's wave-slots in order, sixteen (a CHUNK: one per wave) per step: `old = q[p]--`, barrier, `aft = q[p]`,
// barrier; kept iff old > 0 -- except where the quota runs out inside the chunk (old > 0 but aft < 0: the draws of one
// chunk come in no particular order): those groups are listed (chunk, position, -aft) by the record that drew
// old == 1 and settled after the last chunk by the same workgroup (pm_settle_groups).  A wave's records are the 64 slots its descriptor names -- one word, asked for
// fifteen chunks ahead -- and their positions and read indices are asked for seven chunks ahead, issued and waited for by
// hand.  Kept records: the wave collects their read indices in a ring of 128 words in LDS and marks them 64 at a time --
// one atomic instruction every ~20 chunks instead of one per chunk: atomics and stores share the loads' counter, and a
// counted wait also waits for everything of theirs that is still on its way.
__global__ __launch_bounds__(1024) void k_pm_walk(const uint16_t* __restrict__ keys16, const uint16_t* __restrict__ idx16,
                                                  const uint32_t* __restrict__ desc,
                                                  const uint32_t* __restrict__ Tp, uint32_t pitch,
                                                  const uint32_t* __restrict__ range_start /* true flat starts */,
                                                  const uint32_t* __restrict__ grid,
                                                  uint32_t shift, uint32_t stride,
                                                  const uint32_t* __restrict__ boff, const uint32_t* __restrict__ selend,
                                                  EvQuota evq,
                                                  unsigned long long* __restrict__ mask,
                                                  uint2* __restrict__ amb_lists, int lists_by_records,
                                                  unsigned long long* __restrict__ kept_total) {
    extern __shared__ int32_t s_q[];  // [(1 << shift) + 1] quotas
    __shared__ uint32_t s_namb, s_kept;
    __shared__ uint32_t s_ring[16][128];  // per wave: kept records' read indices on their way to the mask
    const uint32_t range = blockIdx.x, width = 1u << shift;
    const uint32_t pos0 = pm_grid_pos0(grid, range), live = pm_grid_live(grid, range);
    const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
    const uint32_t lane = tid & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    QMCP_PM_STAMPS
    QMCP_PM_STAMP_AT(0)
    const uint32_t lo_p = Tp[(size_t)range * pitch];
    const uint32_t hi_p = Tp[(size_t)(range + 1) * pitch];  // (range 255: the scan's total)
    if (lo_p >= hi_p) return;  // uniform: a range without reads needs no quotas either
    const uint32_t g0 = lo_p >> 6, n_ws = (hi_p - lo_p) >> 6;
    const uint32_t n_chunks = (n_ws + 15u) >> 4;
    const uint32_t lo_true = range_start[range];
    uint2* const amb = amb_lists + (lists_by_records ? (size_t)lo_true : (size_t)range * width);
    // the wave's descriptors of chunks 0..6, the plain way (compiler registers), asked for here: they are on their way
    // while the quotas are fetched, not a trip of their own after them
    uint32_t d0[kRankDepth - 1];
#pragma unroll
    for (int k = 0; k < kRankDepth - 1; ++k) d0[k] = desc[g0 + min(16u * (uint32_t)k + w, n_ws - 1u)];
    if (evq.sev != nullptr) {
        // straight from the event-driven sweep's output.  On the aligned grid the range lies in one contig; a range of
        // the global grid that straddles a border looks every position's contig up.
        const uint32_t c_range = pm_grid_contig(grid, range);  // (uniform)
        if (c_range != kPmNoContig) pm_event_quotas<16, true>(evq, c_range, pos0, live, tid, nthreads, s_q);
        else pm_event_quotas<8, false>(evq, c_range, pos0, live, tid, nthreads, s_q);
    } else
    for (uint32_t i0 = tid; i0 < live; i0 += 8 * nthreads) {
        uint32_t a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t i = min(i0 + u * nthreads, live - 1);  // clamped: every load is issued
            a[u] = selend[pos0 + i];
            b[u] = boff[pos0 + i];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u * nthreads < live) s_q[i0 + u * nthreads] = (int32_t)(a[u] - b[u]);
    }
    if (tid == 0) { s_namb = 0; s_kept = 0; }
    __syncthreads();

    // The loads in flight -- positions and descriptors of the chunks ahead -- land in registers the COMPILER NEVER SEES:
    // v96..v103 (positions of the chunk consumed at slot k of the unrolled loop), v104..v111 (descriptors), v112..v119 (read
    // indices inside the pass).  They are named in the assembly, issued and waited for by hand, and every
    // assembly statement of the kernel lists all of them as clobbered, so the compiler keeps nothing of its own there.
    // The first form of this kernel held them in compiler-allocated registers, as k_rank_mark does: the compiler then
    // kept a loop-carried descriptor in another register than the one its load writes and COPIED it at the loop's end --
    // a copy of a register whose load is still in flight, i.e. of what was there before: cfg4 came out different from
    // run to run, one run ended in a memory access fault (a stale descriptor's slots); small inputs never showed it.
    // tools/isa_hazards.py checks the assembly for such reads and that v96..v119 occur in hand-written assembly only
    // (tests/test_isa_hazards.py).
#define QMCP_PM_RING "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119"
#define QMCP_PM_KEYREG(k) "v" QMCP_PM_STR(QMCP_PM_CAT(QMCP_PM_KEY_, k))
#define QMCP_PM_DSCREG(k) "v" QMCP_PM_STR(QMCP_PM_CAT(QMCP_PM_DSC_, k))
#define QMCP_PM_IDXREG(k) "v" QMCP_PM_STR(QMCP_PM_CAT(QMCP_PM_IDX_, k))
#define QMCP_PM_STR(x) QMCP_PM_STR2(x)
#define QMCP_PM_STR2(x) #x
#define QMCP_PM_CAT(a, b) QMCP_PM_CAT2(a, b)
#define QMCP_PM_CAT2(a, b) a##b
#define QMCP_PM_KEY_0 96
#define QMCP_PM_KEY_1 97
#define QMCP_PM_KEY_2 98
#define QMCP_PM_KEY_3 99
#define QMCP_PM_KEY_4 100
#define QMCP_PM_KEY_5 101
#define QMCP_PM_KEY_6 102
#define QMCP_PM_KEY_7 103
#define QMCP_PM_DSC_0 104
#define QMCP_PM_DSC_1 105
#define QMCP_PM_DSC_2 106
#define QMCP_PM_DSC_3 107
#define QMCP_PM_DSC_4 108
#define QMCP_PM_DSC_5 109
#define QMCP_PM_DSC_6 110
#define QMCP_PM_DSC_7 111
#define QMCP_PM_IDX_0 112
#define QMCP_PM_IDX_1 113
#define QMCP_PM_IDX_2 114
#define QMCP_PM_IDX_3 115
#define QMCP_PM_IDX_4 116
#define QMCP_PM_IDX_5 117
#define QMCP_PM_IDX_6 118
#define QMCP_PM_IDX_7 119
    static_assert(kRankDepth == 8, "the ring registers are named for eight slots");
    struct Slot { uint32_t slot0, nv, read0; bool has; };  // of a chunk whose records are in flight or being consumed (uniform; the compiler's)
    auto desc_offset = [&](uint32_t c) -> uint32_t {  // byte offset of the wave's descriptor of chunk c (the range's last beyond it: never used)
        return (g0 + min(16u * c + w, n_ws - 1u)) * 4u;
    };
    auto slot_of = [&](uint32_t dsc, uint32_t c) -> Slot {
        const bool has = 16u * c + w < n_ws;  // uniform
        // (on the vector unit, although every lane holds the same word: through v_readfirstlane and the scalar unit --
        //  fewer vector instructions -- the walk took 0.285 instead of 0.255 ms at cfg4: the scalar chain's dependent
        //  multi-cycle instructions sit in front of the requests for the chunk seven steps ahead)
        const PmSlot at = pm_unpack<true>(dsc, has, stride);
        Slot s;
        s.slot0 = at.slot0;
        s.nv = at.nv;
        s.read0 = at.pass * (uint32_t)kPmPass;  // the pass's first read
        s.has = has;
        return s;
    };
    uint32_t kept = 0;  // (set from `cur` after the walk)
    // kept read indices collected / marked so far (uniform)
    uint32_t cur = 0, flushed = 0;
    uint32_t* const ring = s_ring[w];
    // One slot of the walk (K: its place in the unrolled loop, KF = (K + 7) % 8): chunk c is consumed from ring slot K;
    // chunk c + 7's positions are asked for into slot KF through slot K's descriptor (asked for eight slots ago), and
    // slot K's descriptor is asked for again, for chunk c + 15.
    // Loads complete in issue order.  Per slot three are issued: positions, read indices, a descriptor.  The read indices
    // of chunk c were asked for seven slots ago and 19 loads have been issued since; its positions and the descriptor read
    // with them are older.  (Younger stores and atomics only make the wait longer.)
#define QMCP_PM_STEP(K, KF)                                                                                                   \
    {                                                                                                                         \
        const uint32_t c = c0 + (uint32_t)(K);                                                                                \
        uint32_t key, dsc, idx;                                                                                               \
        asm volatile("s_waitcnt vmcnt(19)\n\tv_mov_b32 %0, " QMCP_PM_KEYREG(K) "\n\tv_mov_b32 %1, " QMCP_PM_DSCREG(K)          \
                     "\n\tv_mov_b32 %2, " QMCP_PM_IDXREG(K)                                                                   \
                     : "=v"(key), "=v"(dsc), "=v"(idx) : : QMCP_PM_RING, "memory");                                                      \
        const Slot at = S[K];                                                                                                 \
        const bool valid = lane < at.nv;                                                                                      \
        int32_t old = 0;                                                                                                      \
        if (valid) old = atomicSub(&s_q[key], 1); /* (the 16-bit load zero-extends) */                                        \
        S[KF] = slot_of(dsc, c + 7u);                                                                                         \
        asm volatile("global_load_ushort " QMCP_PM_KEYREG(KF) ", %0, %1\n\tglobal_load_ushort " QMCP_PM_IDXREG(KF) ", %0, %2"   \
                     "\n\tglobal_load_dword " QMCP_PM_DSCREG(K) ", %3, %4"                                                    \
                     : : "v"((S[KF].slot0 + lane) * 2u), "s"(keys16), "s"(idx16), "v"(desc_offset(c + 15u)), "s"(desc)        \
                     : QMCP_PM_RING, "memory");                                                                               \
        __syncthreads();                                                                                                      \
        int32_t aft = 0;                                                                                                      \
        if (valid) aft = s_q[key];                                                                                            \
        const bool keep = valid && old > 0 && aft >= 0;                                                                       \
        if (valid && old == 1 && aft < 0) {                                                                                   \
            const uint32_t k = atomicAdd(&s_namb, 1u);                                                                        \
            amb[k] = make_uint2((c << 15) | key, (uint32_t)(-aft)); /* c < 2^17, key < 2^15 */                                \
        }                                                                                                                     \
        __syncthreads(); /* every q_after is read before the next chunk draws */                                              \
        if (at.has) { /* uniform: the wave has a wave-slot in this chunk */                                                   \
            const uint64_t kb = __ballot(keep);                                                                               \
            const uint32_t cw = (uint32_t)__popcll(kb);                                                                       \
            if (keep) ring[(cur + __builtin_amdgcn_mbcnt_hi((uint32_t)(kb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kb, 0u))) & 127u] = at.read0 + idx; \
            cur += cw;                                                                                                        \
            if (cur - flushed >= 64u) { /* uniform */                                                                         \
                const uint32_t v = ring[(flushed + lane) & 127u];                                                             \
                atomicOr(&mask[v >> 6], 1ull << (v & 63u));                                                                   \
                flushed += 64u;                                                                                               \
            }                                                                                                                 \
        }                                                                                                                     \
    }
    Slot S[kRankDepth];
    {
        // chunks 0..6: descriptors the plain way (d0[]: asked for ahead of the quotas), their positions into the ring;
        // descriptors of chunks 7..14 into the ring; then everything is waited for once -- the loop's counted wait
        // assumes its own issue order (positions, descriptor, positions, ...), which these requests do not have
#pragma unroll
        for (int k = 0; k < kRankDepth - 1; ++k) S[k] = slot_of(d0[k], (uint32_t)k);
        S[kRankDepth - 1] = Slot{0u, 0u, 0u, false};
#define QMCP_PM_ASK_KEYS(K) asm volatile("global_load_ushort " QMCP_PM_KEYREG(K) ", %0, %1\n\tglobal_load_ushort " QMCP_PM_IDXREG(K) ", %0, %2" : : "v"((S[K].slot0 + lane) * 2u), "s"(keys16), "s"(idx16) : QMCP_PM_RING, "memory");
#define QMCP_PM_ASK_DSC(K) asm volatile("global_load_dword " QMCP_PM_DSCREG(K) ", %0, %1" : : "v"(desc_offset(7u + (uint32_t)(K))), "s"(desc) : QMCP_PM_RING, "memory");
        QMCP_PM_ASK_KEYS(0) QMCP_PM_ASK_KEYS(1) QMCP_PM_ASK_KEYS(2) QMCP_PM_ASK_KEYS(3) QMCP_PM_ASK_KEYS(4) QMCP_PM_ASK_KEYS(5) QMCP_PM_ASK_KEYS(6)
        QMCP_PM_ASK_DSC(0) QMCP_PM_ASK_DSC(1) QMCP_PM_ASK_DSC(2) QMCP_PM_ASK_DSC(3) QMCP_PM_ASK_DSC(4) QMCP_PM_ASK_DSC(5) QMCP_PM_ASK_DSC(6) QMCP_PM_ASK_DSC(7)
        asm volatile("s_waitcnt vmcnt(0)" : : : QMCP_PM_RING, "memory");
#undef QMCP_PM_ASK_KEYS
#undef QMCP_PM_ASK_DSC
    }
    QMCP_PM_STAMP_AT(1)
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += kRankDepth) {
        QMCP_PM_STEP(0, 7) QMCP_PM_STEP(1, 0) QMCP_PM_STEP(2, 1) QMCP_PM_STEP(3, 2)
        QMCP_PM_STEP(4, 3) QMCP_PM_STEP(5, 4) QMCP_PM_STEP(6, 5) QMCP_PM_STEP(7, 6)
    }
#undef QMCP_PM_STEP
    asm volatile("s_waitcnt vmcnt(0)" : : : QMCP_PM_RING, "memory");  // (the loads asked for beyond the last chunk)
    QMCP_PM_STAMP_AT(2)
    if (lane < cur - flushed) {
        const uint32_t v = ring[(flushed + lane) & 127u];
        atomicOr(&mask[v >> 6], 1ull << (v & 63u));
    }
    kept = cur;
    // The groups this workgroup listed, settled where they were produced: the barrier makes its amb[] stores (and
    // s_namb) visible to its own waves -- workgroup scope is all that is needed, nobody else reads the list.  Plain C++
    // from here on: the ring registers are dead.
    __syncthreads();
    kept += pm_settle_groups(keys16, idx16, desc, g0, n_ws, stride, amb, s_namb, w, lane, mask);
    if (lane == 0 && kept) atomicAdd(&s_kept, kept);
    __syncthreads();
    QMCP_PM_STAMP_AT(3)
    QMCP_PM_STAMPS_OUT(1)
    if (tid == 0 && s_kept) atomicAdd(kept_total, (unsigned long long)s_kept);
}

// ---- launchers
#ifdef QMCP_PM_STAMP
// (lab build only) the stamps of the last k_pm_offsets and k_pm_walk launches -> out[2 * 256 * 8]
extern "C" int qmcp_lab_pm_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pm_stamps), sizeof(g_pm_stamps));
}
#endif
uint32_t pm_pitch(uint32_t n) { return part_pass_pitch(n); }  // passes of the call, rounded up to a multiple of 4
uint32_t pm_pass() { return (uint32_t)kPmPass; }
uint32_t pm_stride(uint32_t n_ranges) { return pm_stride_of(n_ranges); }
size_t pm_slots(uint32_t n, uint32_t n_ranges) { return (size_t)pm_pitch(n) * pm_stride(n_ranges); }  // slots of keys16 / idx16
uint32_t pm_work_words() { return kPmWorkWords; }
uint32_t pm_exc_slots(uint32_t n) { return pm_pitch(n) * kPmWaves * kPmExcPerWave + kNuOverflow; }  // the exception list's slots: 128 per wave and pass, and the overflow region
// the walk's lists of quota-crossing groups: a slot per position of every range of the grid, or per read
bool pm_rank_scratch_by_records(uint32_t shift, uint32_t n_ranges, uint32_t n) { return (size_t)n < ((size_t)n_ranges << shift); }
size_t pm_rank_scratch_bytes(uint32_t shift, uint32_t n_ranges, uint32_t n) {
    const size_t by_pos = (size_t)n_ranges << shift;
    return (by_pos < (size_t)n ? by_pos : (size_t)n) * sizeof(uint2) + 64;
}
void launch_pm_prepare_sort(hipStream_t st, const uint32_t* starts, const uint32_t* ends, uint32_t n,
                            const uint64_t* d_roff, const uint64_t* d_poff, uint32_t n_contigs, uint32_t shift,
                            uint32_t n_ranges, const uint32_t* d_grid,
                            uint16_t* keys16, uint16_t* idx16, uint32_t* cnt_tab, uint32_t* lst_tab,
                            uint32_t* stats, unsigned long long* zero_mask, uint32_t ell_reg, uint32_t* exc,
                            uint32_t exc_cap, uint32_t* exc_cnt) {
    const uint32_t pitch = pm_pitch(n);
    if (pitch == 0) return;
    (void)hipFuncSetAttribute((const void*)k_pm_prepare_sort, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPmSortLds);
    hipLaunchKernelGGL(k_pm_prepare_sort, dim3(pitch / kPmPassesPerWg), dim3(kPmThreads), kPmSortLds, st, starts, ends, n,
                       d_roff, d_poff, n_contigs, d_grid + 3u * kPmGridRows, shift, pm_stride(n_ranges), keys16, idx16,
                       cnt_tab, lst_tab, pitch, stats, zero_mask, exc != nullptr ? ell_reg : 0u, exc, exc_cap, exc_cnt);
    if (exc != nullptr && ell_reg != 0u)
        hipLaunchKernelGGL(k_nu_count_groups, dim3(32), dim3(256), 0, st, exc_cnt, pitch * kPmWaves, stats);
}
// The table stage: the padded count table scanned in place (tab: counts in, Tp out, the total at tab[256 pitch]), the
// wave-slot descriptors, the ranges' true flat starts and the heaviest load (records, and wave-slots) -- two launches.
// All 256 rows, whatever the grid's ranges: the rows beyond them hold zeros and scan to the total.
void launch_pm_row_sums(hipStream_t st, const uint32_t* cnt_tab, const uint32_t* lstw, uint32_t n, uint32_t* work) {
    const uint32_t pitch = pm_pitch(n);
    if (pitch == 0) return;
    hipLaunchKernelGGL(k_pm_row_sums, dim3(256, kPmDescrY), dim3(256), 0, st, cnt_tab, lstw, pitch, work);
}
void launch_pm_tables(hipStream_t st, uint32_t* tab, const uint32_t* lstw, uint32_t n, uint32_t n_ranges,
                      uint32_t* desc, const uint32_t* work, uint32_t* range_start, uint32_t* max_load, uint32_t* clear16) {
    const uint32_t pitch = pm_pitch(n);
    if (pitch == 0) return;
    const uint32_t s64 = pm_stride(n_ranges) / 64u;
    hipLaunchKernelGGL(k_pm_tables, dim3(256, kPmDescrY), dim3(256), 0, st, tab, lstw, pitch, pitch * s64, desc, work,
                       range_start, max_load, clear16);
}
void launch_pm_offsets(hipStream_t st, const uint16_t* keys16, const uint32_t* desc, const uint32_t* Tp, uint32_t n,
                       const uint32_t* range_start, uint32_t shift, uint32_t n_ranges, const uint32_t* d_grid, uint32_t ltot,
                       uint32_t* boff, uint32_t* empty_positions) {
    const size_t width = (size_t)1 << shift;
    const size_t lds = (width + width / 32 + 1) * sizeof(uint32_t);
    (void)hipFuncSetAttribute((const void*)k_pm_offsets, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_pm_offsets, dim3(n_ranges), dim3(1024), lds, st, keys16, desc, Tp, pm_pitch(n), range_start, d_grid,
                       shift, pm_stride(n_ranges), ltot, boff, empty_positions);
}
// The ranking: the ordered walk, with the settling of the groups it listed in its tail -- one launch.
void launch_pm_walk(hipStream_t st, const uint16_t* keys16, const uint16_t* idx16, const uint32_t* desc, const uint32_t* Tp,
                    uint32_t n, const uint32_t* range_start, uint32_t shift, uint32_t n_ranges, const uint32_t* d_grid,
                    const uint32_t* boff, const uint32_t* selend, unsigned long long* mask, unsigned long long* kept_total, void* scratch,
                    bool scratch_by_records, const uint32_t* ev_sev, const uint32_t* ev_lastns,
                    const uint64_t* d_poff, uint32_t n_contigs, uint32_t ell) {
    const EvQuota evq{ev_sev, ev_lastns, d_poff, n_contigs, ell, pm_div_make(ell)};
    const size_t lds = (((size_t)1 << shift) + 1) * sizeof(uint32_t);
    (void)hipFuncSetAttribute((const void*)k_pm_walk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_pm_walk, dim3(n_ranges), dim3(1024), lds, st, keys16, idx16, desc, Tp, pm_pitch(n), range_start, d_grid, shift,
                       pm_stride(n_ranges), boff, selend, evq, mask, (uint2*)scratch, scratch_by_records ? 1 : 0,
                       kept_total);
}
