// Launchers of the gfx950 kernels in qmcp_kernels.hip (internal to the library; the public
// surface is include/qmcp_hip.h).
#ifndef QMCP_KERNELS_H
#define QMCP_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmcp_hip.h"    // qmcp_hip_track_run
#include "sweep_plan.h"  // the shape predicates and window counts the host decides with
#include "dedup_plan.h"  // DedupPack, DedupSortForm: how a round's key is packed, which form the sort takes
#include "thresholds_plan.h"  // thresholds_word: one mask word folded into the reads seen so far
#include "pm_grid_plan.h"  // PmGridPlan: where the pass-major form cuts its ranges, and the tables that say so

namespace qmcp {

static constexpr uint32_t kMaxLdsRingSpan = 16383;   // two LDS rings of 16384 u32 = 128 KiB
static constexpr uint32_t kMaxGeneralSpan = (1u << 24) - 1;  // beyond kMaxLdsRingSpan the rings live in global memory
static constexpr uint32_t kMaxUniformSpan = 512;    // 8 positions per lane in the block sweep
static constexpr uint32_t kMaxCachedSpan = 4032;    // LDS-cached mixed-span sweep: 8 words x 4096 slots,
                                                    // ring >= max_span + 64 (a chunk enters 64 buckets at once)

void launch_prepare(hipStream_t st, const uint32_t* starts, const uint32_t* ends, uint32_t n,
                    const uint64_t* d_roff, const uint64_t* d_poff, uint32_t n_contigs,
                    const uint64_t* keep_mask, uint32_t* gstart, uint32_t* cstart,
                    uint32_t* stats, uint32_t part_shift,
                    uint32_t* part_hist /* digit-major [256][tiles] of (gstart >> part_shift), or null */,
                    uint32_t* digit0_hist /* same shape, low byte of gstart; needs part_hist; or null */,
                    uint32_t* global_digit_hist /* [4][256] whole-call digit counts of gstart, or null */,
                    unsigned long long* zero_mask /* keep mask to clear (ceil(n/64) words), or null */,
                    uint32_t ell_reg = 0, uint32_t* exc = nullptr, uint32_t exc_cap = 0, uint32_t* exc_cnt = nullptr
                    /* near-uniform route on the range-major form: see k_prepare */,
                    uint32_t tiles_per_block = 0 /* tiles a workgroup takes (at most 8; even with part_hist); 0: chosen by the
                                                    tile count (the stage tests run the wider forms on a few tiles) */);
uint32_t prepare_exc_slots(uint32_t n);  // slots of the exception list when k_prepare fills it (groups of 128 per wave and tile)
void launch_general_keys(hipStream_t st, bool wide, const uint32_t* gstart, const uint32_t* starts,
                         const uint32_t* ends, uint32_t n, uint32_t span_bits, uint32_t max_span,
                         const uint64_t* keep_mask, void* keys, uint32_t* ecnt,
                         uint32_t ecnt_len /* entries of ecnt (positions + 1), 0: unknown */);
uint32_t scan_spine_entries(uint32_t n);
void launch_exclusive_scan(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out,
                           uint32_t* spine, bool write_total);
uint32_t sort_tiles(uint32_t n);
void launch_radix_hist(hipStream_t st, bool wide, const void* keys_in, uint32_t n, uint32_t shift,
                       uint32_t* hist);
void launch_radix_scatter(hipStream_t st, bool wide, const void* keys_in, const uint32_t* vals_in,
                          uint32_t n, uint32_t shift, const uint32_t* offs, void* keys_out,
                          uint32_t* vals_out);
// row pitch, in partition passes (pairs of 4096-read tiles), of the range partition's [digit][pass]
// table (k_prepare writes it, one plain scan over 256 * pitch entries turns it into offsets, the
// partition reads it)
uint32_t part_pass_pitch(uint32_t n);

// ------------------------------------------------------------------ the sweeps
// Where a sweep runs: the stream, the bucket offsets of the reads it sweeps, the contigs on the global axis, and the
// stretch table -- null: one workgroup per contig; else launch_sweep_segments' (or a speculative tier's), with a
// workgroup for each of its n_seg_max = n_contigs + windows candidate stretches.  Built once per solve; every
// launch_sweep_* and launch_spec_* takes it first, then what is its own.
struct SweepAxis {
    hipStream_t st;
    const uint32_t* boff;
    const uint64_t* poff;
    uint32_t n_contigs, ltot;
    const uint32_t* seg = nullptr;
    uint32_t n_seg_max = 0;
    uint32_t workgroups() const { return seg ? n_seg_max : n_contigs; }
    // the same axis under another table of the same windows (the speculative tiers)
    SweepAxis with_table(const uint32_t* table) const {
        SweepAxis a = *this;
        a.seg = table;
        return a;
    }
};
// The sorted reads a mixed-span sweep walks: Rec{key, val} records (wide == false) or u64 keys, the run lengths where
// the walk reads them (launch_group_heads; null otherwise), and the key's span field.
struct SortedSpans {
    bool wide;
    const void* sorted;
    const uint32_t* next_head;
    uint32_t span_bits, max_span;
};
// What a mixed-span sweep holds the coverage against, per position: eoff, the prefix counts of read ends (coverage =
// starts - ends) under the scalar cap M; or, capped, a profile's need[] (M is not read).
struct SweepDemand {
    const uint32_t* per_position;
    bool capped;
};

// Cut points (coverage <= M) split a contig's sweep exactly.  sweep_segment_windows (sweep_plan.h): how many
// windows to look for cuts in (0: not worth it); launch_sweep_segments fills `seg_words` (sweep_segment_words()
// uint32: [windows' cuts | count, stretches]) and returns the axis under that table.
// eoff: prefix counts of read ends for mixed spans; null for one span ell
SweepAxis launch_sweep_segments(const SweepAxis& ax, const uint32_t* eoff, uint32_t ell, uint32_t M, uint32_t n_windows,
                                uint32_t* seg_words,
                                const uint32_t* other_cov = nullptr /* reads outside boff covering position q - 1:
                                    other_cov[q] (the near-uniform route's exceptions) */);
// Speculative boundaries (kernels/sweep_segments.inc.hip): further tables of the same windows (tier 1, 2
// behind the exact one in seg_words), with a boundary `burn` positions of run-in wide wherever a window has no
// cut (call launch_sweep_segments first; *n_speculative receives how many; burn == 0: the exact table again),
// and the check + merge of the two outputs behind a sweep of the axis' table (a disagreement marks its exact stretch in
// redo_out; a later tier passes the previous tier's marks as redo_in).
const uint32_t* launch_sweep_segments_speculative(const SweepAxis& ax, uint32_t n_windows, uint32_t burn,
                                                  uint32_t* seg_words, uint32_t* n_speculative,
                                                  uint32_t run_ins_apart, uint32_t tier);
void launch_spec_verify(const SweepAxis& ax, uint32_t ell, const uint32_t* owned, const uint32_t* run_in,
                        uint32_t* mismatches, const uint32_t* redo_in, uint32_t* redo_out,
                        const uint32_t* own_marks = nullptr /* per stretch of the table: which were swept this time */);
void launch_spec_verify_merge_mixed(const SweepAxis& ax, uint32_t max_span, uint32_t* out_even, const uint32_t* out_odd,
                                    const uint32_t* snap, uint32_t* mismatches, const uint32_t* redo_in,
                                    uint32_t* redo_out);
// One span ell: the seven-wave pipelines (fast form with checked fallback; every block in the general form -- sparse
// data: the fast form rarely holds) and the single-wave kernel.  false: the span is not one the form takes.
bool launch_sweep_uniform_mw(const SweepAxis& ax, uint32_t ell, uint32_t M, uint32_t* selend, uint32_t* iter_stats);
// selend_run_in (or null): speculative tables -- a stretch's run-in is stored there, what it owns in selend;
// redo_in (or null): a later tier -- only stretches whose exact stretch is marked there do anything
bool launch_sweep_uniform_gen(const SweepAxis& ax, uint32_t ell, uint32_t M, uint32_t* selend, uint32_t* iter_stats,
                              uint32_t* selend_run_in = nullptr, const uint32_t* redo_in = nullptr,
                              const int32_t* nadj = nullptr /* near-uniform route: need(p) += nadj[p], capped at the
                                                               swept reads' coverage (ltot + 1 entries) */,
                              const uint32_t* own_marks = nullptr /* per stretch of the table: 0 = leave its output alone */);
bool launch_sweep_uniform(const SweepAxis& ax, uint32_t ell, uint32_t M, uint32_t* selend, uint32_t* iter_stats);
// event-driven form for deep data (kernels/sweep_uniform_events.inc.hip): pack, chain, expand -- three launches, apart,
// so that the host can bracket each.  pk / lastns are scratch of sweep_ev_pack_bytes / sweep_ev_last_bytes
// (sweep_plan.h); sev has ltot + 8 words.
bool launch_sweep_ev_pack(const SweepAxis& ax, uint32_t ell, uint32_t M, uint32_t* pk, const int32_t* nadj = nullptr,
                          const uint32_t* from = nullptr);
bool launch_sweep_ev_chain(const SweepAxis& ax, uint32_t ell, uint32_t M, const uint32_t* pk, uint32_t* sev,
                           uint32_t* lastns, uint32_t* iter_stats, const int32_t* nadj = nullptr,
                           uint32_t* ckpt = nullptr /* sweep_ev_ckpt_bytes */,
                           const uint32_t* restart = nullptr /* per stretch: first block to sweep (multiple of 64) */);
bool launch_sweep_ev_expand(const SweepAxis& ax, uint32_t ell, uint32_t M, const uint32_t* sev, const uint32_t* lastns,
                            uint32_t* selend, const uint32_t* from = nullptr);
// Mixed spans: the plain walk (any span; rings of ring_size words in LDS, or in g_rings -- 2 * ring_size words per
// workgroup -- when they do not fit), the LDS-cached walk, and the register-resident one (buckets per lane
// ceil((max_span + 64) / 64), up to 8: false beyond) with its speculative outputs.
void launch_sweep_general(const SweepAxis& ax, const SortedSpans& reads, SweepDemand demand, uint32_t M, uint32_t* selend,
                          uint32_t ring_size, uint32_t* g_rings);
void launch_group_heads(hipStream_t st, bool wide, const void* sorted, uint32_t n,
                        uint32_t* next_head /* n + 1 entries; reverse-min-scan it afterwards */);
void launch_sweep_general_cached(const SweepAxis& ax, const SortedSpans& reads, const uint32_t* eoff, uint32_t M,
                                 uint32_t* selend, uint32_t ring);
bool launch_sweep_general_reg(const SweepAxis& ax, const SortedSpans& reads, SweepDemand demand, uint32_t M,
                              uint32_t* selend, uint32_t* selend_odd = nullptr, const uint32_t* redo_in = nullptr,
                              uint32_t* snap = nullptr /* speculative tables: spec_snap_bytes(n_seg_max) */);
// `sorted` is a Rec{key,val} array (wide == false) or u64 keys with `svals` beside them
void launch_mark(hipStream_t st, bool wide, const void* sorted, const uint32_t* svals, uint32_t ltot,
                 const uint32_t* boff, const uint32_t* selend, uint64_t* mask,
                 unsigned long long* n_kept);
// Coverage profile (kernels/profile.inc.hip): need[p] = min(cov(p), cap(p)) with the top bit set where cov(p) <= cap(p),
// from a batch's sorted, disjoint regions in global positions (rs / re / cap, n_regions of them; default_cap elsewhere);
// pstat[0] += positions with cov > cap, pstat[1] += the sum of need.  launch_profile_segments is launch_sweep_segments
// reading that bit; the mixed-span sweeps take need[] as a capped SweepDemand.
void launch_profile_need(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, uint32_t ltot, const uint32_t* rs,
                         const uint32_t* re, const uint32_t* cap, uint32_t n_regions, uint32_t default_cap, uint32_t* need,
                         unsigned long long* pstat);
SweepAxis launch_profile_segments(const SweepAxis& ax, const uint32_t* need, uint32_t n_windows, uint32_t* seg_words);
void launch_bucket_heads(hipStream_t st, bool wide, const void* sorted, const uint32_t* svals,
                         uint32_t n, uint32_t span_bits, uint32_t ltot, uint32_t* boff);
void launch_reverse_min_scan(hipStream_t st, uint32_t* data, uint32_t n, uint32_t* spine);
void launch_radix_hist_rec(hipStream_t st, bool first, const uint32_t* keys, const void* recs,
                           uint32_t n, uint32_t shift, uint32_t* hist);
void launch_radix_scatter_rec(hipStream_t st, bool first, const uint32_t* keys, const void* recs_in,
                              uint32_t n, uint32_t shift, const uint32_t* offs, void* recs_out);
void launch_coverage(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, uint32_t ltot,
                     uint32_t* cov);
void launch_b_and_demand(hipStream_t st, const uint32_t* cov, uint32_t n, uint32_t M, int32_t* b, int32_t* d);
void launch_complete_pairs(hipStream_t st, uint64_t* mask, uint32_t n_words, uint64_t n_reads);
void launch_word_popcounts(hipStream_t st, const uint64_t* words, uint32_t n_words, uint32_t* counts);
void launch_mask_to_indices(hipStream_t st, const uint64_t* mask, uint32_t n_words, const uint32_t* word_base,
                            unsigned long long* out);
void launch_compact_pairs(hipStream_t st, const uint32_t* starts, const uint32_t* ends,
                          const uint64_t* pair_keep, const uint32_t* word_base, uint64_t n_pairs,
                          uint32_t* starts_c, uint32_t* ends_c, uint32_t* orig_pair);
void launch_expand_mask(hipStream_t st, const uint64_t* mask_c, const uint32_t* orig_pair,
                        uint32_t n_reads_c, uint64_t* mask);
void launch_amplicon_filter(hipStream_t st, const uint32_t* starts, const uint32_t* ends,
                            const uint32_t* seq_lengths, const uint32_t* qualities,
                            uint64_t n_pairs, const uint32_t* amp_starts, const uint32_t* amp_ends,
                            uint32_t n_amp, uint32_t min_length, uint32_t min_mapq,
                            uint64_t* pair_keep);

// range-ranked uniform path: one stable partition of {start, index} records by position range,
// then per-range LDS histograms (counts) and per-range ordered ranking against S(p) (keep mask)
uint32_t range_shift_for(uint32_t ltot);
bool range_path_supported(uint32_t ltot);
bool range_path_two_level(uint32_t ltot);  // more than 256 ranges: two partition levels
uint32_t seg_tile_bound(uint32_t n);
void launch_partition_level1(hipStream_t st, const uint32_t* starts, const uint64_t* d_roff,
                             const uint64_t* d_poff, uint32_t n_contigs, uint32_t n, uint32_t shift_hi,
                             const uint32_t* offs, void* recs_out, uint32_t* super_start,
                             uint32_t* max_super_load, const uint32_t* ends = nullptr, uint32_t ell_reg = 0);
void launch_partition_level2(hipStream_t st, const void* recs_in, uint32_t n, uint32_t shift,
                             uint32_t* tables /* 771 words */, uint32_t* hist, uint32_t* spine,
                             uint16_t* keys16_out, uint32_t* idx_out, uint32_t* range_start /* 65537 */,
                             uint32_t* max_load);
void launch_range_partition(hipStream_t st, const uint32_t* gstart_or_null, const uint32_t* starts,
                            const uint64_t* d_roff, const uint64_t* d_poff, uint32_t n_contigs,
                            uint32_t n, uint32_t shift, const uint32_t* offs, uint16_t* keys16_out,
                            uint32_t* idx_out, uint32_t* range_start /* [257] */, uint32_t* max_load,
                            const uint32_t* ends = nullptr, uint32_t ell_reg = 0 /* near-uniform route: leave out other spans */);
void launch_gstart(hipStream_t st, const uint32_t* starts, uint32_t n, const uint64_t* d_roff,
                   const uint64_t* d_poff, uint32_t n_contigs, uint32_t* gstart);
void launch_fill_ends(hipStream_t st, const uint32_t* starts, uint32_t n, uint32_t span_minus_1, uint32_t* ends);
void launch_range_offsets(hipStream_t st, const uint16_t* keys16, const uint32_t* range_start,
                          uint32_t shift, uint32_t ltot, uint32_t* boff,
                          uint32_t* empty_positions /* zeroed counter: positions that start no read; or null */);
size_t rank_scratch_bytes(uint32_t shift, uint32_t ltot, uint32_t n);  // list slots: per position or per read
bool rank_scratch_by_records(uint32_t shift, uint32_t ltot, uint32_t n);
void launch_rank_mark(hipStream_t st, const uint16_t* keys16, const uint32_t* idx,
                      const uint32_t* range_start, uint32_t shift, uint32_t ltot, const uint32_t* boff,
                      const uint32_t* selend, unsigned long long* mask, unsigned long long* kept_total,
                      void* scratch, bool scratch_by_records);

// range-ranked route, pass-major layout (kernels/pass_major.inc.hip): one-level genomes
uint32_t pm_pitch(uint32_t n);     // row pitch of the [range][pass] tables
uint32_t pm_pass();                // reads per pass
// (n_ranges, d_grid: the grid pm_grid_plan.h cut -- its range count and its tables on the device, pos0 | live | contig |
//  vbase in one buffer)
uint32_t pm_stride(uint32_t n_ranges);                          // slots between the beginnings of two passes
size_t pm_slots(uint32_t n, uint32_t n_ranges);                 // slots of the two 16-bit record streams
size_t pm_rank_scratch_bytes(uint32_t shift, uint32_t n_ranges, uint32_t n);  // the walk's list slots: per position of the grid or per read
bool pm_rank_scratch_by_records(uint32_t shift, uint32_t n_ranges, uint32_t n);
uint32_t pm_work_words();          // words of the table stage's working buffer (k_pm_row_sums -> k_pm_tables)
void launch_pm_prepare_sort(hipStream_t st, const uint32_t* starts, const uint32_t* ends, uint32_t n,
                            const uint64_t* d_roff, const uint64_t* d_poff, uint32_t n_contigs, uint32_t shift,
                            uint32_t n_ranges, const uint32_t* d_grid, uint16_t* keys16, uint16_t* idx16, uint32_t* cnt_tab, uint32_t* lst_tab,
                            uint32_t* stats, unsigned long long* zero_mask, uint32_t ell_reg = 0, uint32_t* exc = nullptr,
                            uint32_t exc_cap = 0, uint32_t* exc_cnt = nullptr);
uint32_t pm_exc_slots(uint32_t n);  // slots of the near-uniform route's exception list (groups of 64, one per wave and pass)
// the table stage, two launches in this order on one stream: the parts' sums of the two tables (work: pm_work_words());
// then the padded count table scanned in place (tab: counts in, padded flat positions out, the total at
// tab[256 pitch]), wave-slot descriptors (pm_slots / 64 words), the ranges' true flat starts (257 words), the heaviest
// range's records and wave-slots (max_load: two words).  clear16: sixteen words the second launch also sets to zero (or null)
void launch_pm_row_sums(hipStream_t st, const uint32_t* cnt_tab, const uint32_t* lstw, uint32_t n, uint32_t* work);
void launch_pm_tables(hipStream_t st, uint32_t* tab, const uint32_t* lstw, uint32_t n, uint32_t n_ranges,
                      uint32_t* desc, const uint32_t* work, uint32_t* range_start, uint32_t* max_load, uint32_t* clear16);
void launch_pm_offsets(hipStream_t st, const uint16_t* keys16, const uint32_t* desc, const uint32_t* Tp, uint32_t n,
                       const uint32_t* range_start, uint32_t shift, uint32_t n_ranges, const uint32_t* d_grid, uint32_t ltot,
                       uint32_t* boff, uint32_t* empty_positions);
// the ranking: ordered walk (kept reads marked 64 at a time); the quota-crossing groups it lists are settled in its tail
void launch_pm_walk(hipStream_t st, const uint16_t* keys16, const uint16_t* idx16, const uint32_t* desc, const uint32_t* Tp,
                    uint32_t n, const uint32_t* range_start, uint32_t shift, uint32_t n_ranges, const uint32_t* d_grid,
                    const uint32_t* boff, const uint32_t* selend, unsigned long long* mask, unsigned long long* kept_total, void* scratch,
                    bool scratch_by_records,
                    // quotas straight from the event-driven sweep's output (whole contigs, no stretch table), instead
                    // of selend[] - boff[]: the changed blocks' kept counts, the last changed block per block
                    const uint32_t* ev_sev = nullptr, const uint32_t* ev_lastns = nullptr,
                    const uint64_t* d_poff = nullptr, uint32_t n_contigs = 0, uint32_t ell = 0);


// near-uniform route (kernels/near_uniform.inc.hip): one dominant span, a few shorter reads as listed exceptions
void launch_span_mode_share(hipStream_t st, const uint32_t* starts, const uint32_t* ends, uint32_t n, uint32_t* out /* 3 words: sampled, in the fullest bin, its span */);
size_t nu_exc_bytes(uint32_t cap);
uint32_t nu_overflow_slots();  // the overflow region: the list's last slots
uint32_t* nu_exc_counts(uint32_t* exc, uint32_t cap);  // the groups' counts inside the list's buffer  // the exception list: start, end, index (k_pm_prepare_sort), selection time, event key, group counts
void launch_nu_count_span(hipStream_t st, const uint32_t* starts, const uint32_t* ends, uint32_t n, uint32_t span, uint32_t* out);
void launch_nu_setup(hipStream_t st, uint32_t* exc, uint32_t cap, uint32_t n_exc, const uint32_t* n_over /* the producer's stats[6] */,
                     const uint32_t* boff, uint32_t ltot, uint32_t ell, uint32_t M, uint32_t* ce /* ltot + 3 words */,
                     uint32_t* spine, int32_t* nadj /* ltot + 1 */, uint32_t* state /* 8 words */);
void launch_nu_round(hipStream_t st, uint32_t* exc, uint32_t cap, uint32_t n_exc, const uint32_t* n_over, bool first_round,
                     const uint32_t* boff, const uint32_t* selend, int32_t* nadj, const uint32_t* ce /* launch_nu_setup's */,
                     const uint64_t* d_poff, uint32_t n_contigs,
                     uint32_t ell, uint32_t M, uint2* suspects, uint32_t suspects_cap, uint32_t* state,
                     unsigned long long* viol_key, uint32_t* viol_idx,
                     const uint32_t* swept_from /* per contig: first block the round's sweep covered (0xFFFFFFFF: none) */,
                     uint32_t* sweep_from_next /* per contig, out: where the next round's sweep starts (0xFFFFFFFF: settled) */,
                     uint32_t ltot, uint32_t* spine /* scan_spine_entries(2^17 + 2) words */,
                     const uint32_t* seg_exact /* sweeps in stretches: launch_sweep_segments' table; or null */, uint32_t n_cand,
                     uint32_t* marks_next /* n_cand words, out: the exact stretches the next round's sweep must cover */,
                     uint32_t* selend_prev /* sweeps in stretches: ltot words, the round before's selend (kept here); or null:
                                              every listed exception is replayed */,
                     uint32_t* dirty /* nu_cells_bytes(): cells that changed since the round before (the last round's
                                        dirty_next) */,
                     uint32_t* dirty_next,
                     const uint32_t* seg_fine = nullptr /* sweeps in speculative stretches: the first tier's table */,
                     uint32_t* fine_next = nullptr /* n_cand words, out: the stretches of that table the next round's sweep
                                                      must cover */);
size_t nu_cells_bytes();
size_t nu_suspect_bytes(uint32_t suspects_cap);  // `suspects`: the list and, behind it, its bins by start position
void launch_nu_mark_selected(hipStream_t st, uint32_t* exc, uint32_t cap, uint32_t n_exc, const uint32_t* n_over,
                             unsigned long long* mask, unsigned long long* kept_total);

// reads in any order with a contig id each (kernels/by_contig.inc.hip; api/by_contig.inc.hip drives them): sort keys
// (contig id, n_contigs for QMCP_NO_CONTIG) and the validation flags (err: bit 0 bad id, bit 1 bad read), the contigs'
// bounds in grouped order from the sorted Rec{key, index} array (offs: n_groups + 1 words), a batch's columns gathered
// in grouped order, and a batch's grouped keep mask ORed into the input-order mask
void launch_bc_keys(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids, uint32_t n,
                    const uint32_t* lengths, uint32_t n_contigs, uint32_t* keys, uint32_t* err);
void launch_bc_bounds(hipStream_t st, const void* sorted, uint32_t n, uint32_t n_groups, uint32_t* offs);
void launch_bc_gather(hipStream_t st, const void* sorted, uint32_t n, const uint32_t* starts, const uint32_t* ends,
                      uint32_t* starts_out, uint32_t* ends_out);
void launch_bc_scatter_mask(hipStream_t st, const uint64_t* batch_mask, const void* sorted, uint32_t n, uint64_t* mask);

// the coverage ladder between two levels of a batch (kernels/ladder.inc.hip; api/ladder.inc.hip drives them): the stable
// compaction of the reads `mask` keeps (word_base: its scanned word popcounts, the total behind the last word) with an
// origin column -- origin_in is the grouping's Rec{key, index} array when `first`, the previous origin column otherwise
// --, the kept rank at each of the n_contigs + 1 contig offsets (the next level's offsets), and levels[origin] = level
// for the kept reads of a level
void launch_ladder_compact(hipStream_t st, bool first, const uint32_t* starts, const uint32_t* ends,
                           const void* origin_in, const uint64_t* mask, const uint32_t* word_base, uint32_t n,
                           uint32_t* starts_c, uint32_t* ends_c, uint32_t* origin_c);
void launch_ladder_offsets(hipStream_t st, const uint32_t* offs, uint32_t n_contigs, const uint64_t* mask,
                           const uint32_t* word_base, uint32_t* next);
void launch_ladder_levels(hipStream_t st, bool first, const uint64_t* mask, const void* origin_in, uint32_t n,
                          uint32_t level, uint8_t* levels);

// stratified downsampling (kernels/stratified.inc.hip; api/stratified.inc.hip drives them): validation (err: bits 0 and 1
// as launch_bc_keys, bit 2 a bad stratum id) and the stratum-major sort keys stratum * n_contigs + contig (n_strata *
// n_contigs for a read without contig or stratum), and the per-stratum rows -- rows[4 * s ..] = {reads, kept reads, bases,
// kept bases}, zeroed by the caller -- from the n_placed grouped Rec{key, index} records and the input-order keep mask.
// kStratumTallyTile: the grouped records one workgroup of k_st_tally reduces.
static constexpr uint32_t kStratumTallyTile = 1024;
void launch_st_keys(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                    const uint32_t* strata, uint32_t n, const uint32_t* lengths, uint32_t n_contigs, uint32_t n_strata,
                    uint32_t* keys, uint32_t* err, unsigned long long* none_count = nullptr);
void launch_st_tally(hipStream_t st, const void* sorted, uint32_t n_placed, uint32_t n_contigs, const uint32_t* starts,
                     const uint32_t* ends, const uint64_t* mask, uint64_t* rows);

// pairs of several contigs against the amplicons of their own contig (kernels/amplicon_by_contig.inc.hip; api/
// amplicon_by_contig.inc.hip drives them): the FILTER (amp_offs == NULL: no amplicon predicate; the table of
// amplicon_table.h otherwise, n_amp entries; err as launch_bc_keys) into one bit per pair, and the compaction of the
// surviving pairs with their contig ids.  Every column holds whole pairs and is 8-byte aligned.
void launch_amplicon_filter_by_contig(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                                      const uint32_t* seq_lengths, const uint32_t* qualities, uint64_t n_pairs,
                                      const uint32_t* lengths, uint32_t n_contigs, const uint32_t* amp_offs,
                                      const uint32_t* amp_starts, const uint32_t* amp_pmax, uint32_t n_amp,
                                      uint32_t min_length, uint32_t min_mapq, uint64_t* pair_keep, uint32_t* err);
void launch_compact_pairs_ids(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                              const uint64_t* pair_keep, const uint32_t* word_base, uint64_t n_pairs, uint32_t* starts_c,
                              uint32_t* ends_c, uint32_t* ids_c, uint32_t* orig_pair);

// the quality pass of qmcp_hip_solve_quality_* (kernels/quality_cells.inc.hip; api/quality.inc.hip drives it): the
// quality range of the placed reads (range: {min, max}, preset to {~0u, 0}), composite keys gstart | span - min_span |
// q_max - q (u64 when `wide`, u32 otherwise; ids == NULL: contigs by roff, else by id with QMCP_NO_CONTIG reads in a cell
// of their own), the segment marks and choice over the sorted {key, index} order (records, or split keys + svals when
// `wide`), which flips the bits of the keep mask that change
void launch_qc_range(hipStream_t st, const uint32_t* q, const uint32_t* ids, uint32_t n, uint32_t* range);
void launch_qc_keys(hipStream_t st, bool wide, const uint32_t* starts, const uint32_t* ends, const uint32_t* q,
                    const uint32_t* ids, const uint64_t* roff, const uint64_t* poff, uint32_t n_contigs, uint64_t ltot,
                    uint32_t n, uint32_t min_span, uint32_t span_bits, uint32_t q_max, uint32_t q_bits, void* keys);
void launch_qc_marks(hipStream_t st, bool wide, const void* sorted, const uint32_t* svals, uint32_t n, uint32_t q_bits,
                     const uint64_t* mask, uint32_t* kb, uint32_t* seg_end, uint32_t* seg_head_rev);
void launch_qc_choose(hipStream_t st, bool wide, const void* sorted, const uint32_t* svals, uint32_t n,
                      const uint32_t* P, const uint32_t* seg_end, const uint32_t* seg_head_rev, uint64_t* mask,
                      unsigned long long* counters);

// on-target downsampling (kernels/targets.inc.hip; api/targets.inc.hip drives them): every read validated (err as
// launch_bc_keys) and projected onto its contig's target axis by target_table.h's project_read -- offs (n_contigs + 1),
// rs / re / cum (n_regions) are the device copy of a TargetTable; on / off get one bit per read (on target; placed and off
// target), ps / pe the projection --, the stable compaction of the on-target reads (ids through remap, q may be NULL),
// the compact mask ORed into the zeroed input-order mask through orig, and mask |= other
void launch_target_project(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids, uint32_t n,
                           const uint32_t* lengths, uint32_t n_contigs, const uint32_t* offs, const uint32_t* rs,
                           const uint32_t* re, const uint32_t* cum, uint32_t n_regions, uint32_t* ps, uint32_t* pe,
                           uint64_t* on, uint64_t* off, uint32_t* err);
void launch_compact_reads(hipStream_t st, const uint32_t* ps, const uint32_t* pe, const uint32_t* ids, const uint32_t* q,
                          const uint32_t* remap, const uint64_t* on, const uint32_t* word_base, uint32_t n,
                          uint32_t* starts_c, uint32_t* ends_c, uint32_t* ids_c, uint32_t* q_c, uint32_t* orig);
void launch_expand_mask_reads(hipStream_t st, const uint64_t* mask_c, const uint32_t* orig, uint32_t n_c, uint64_t* mask);
void launch_or_words(hipStream_t st, uint64_t* mask, const uint64_t* other, uint32_t n_words);

// the depth report of qmcp_hip_depth_report_* (kernels/depth_report.inc.hip; api/depth_report.inc.hip drives it), one
// position batch = the contigs [c0, c1) on an axis of `positions` positions: the reads' events (ev: positions + 1 zeroed
// 64-bit words; lengths: every contig's; boff: the batch-local offsets of [c0, c1); mask may be NULL; counts: placed and
// kept reads; err as launch_bc_keys), the chunk sums and their scan (sums: depth_chunks(positions) words), and the pass
// that turns the events into rows (two tables of sorted disjoint intervals lo / hi with the accumulator row of each;
// acc64: 5 x n_rows, acc32: 4 x n_rows with the minima preset to ~0u) and histograms (hist: 2 x n_bins 64-bit words)
void launch_depth_events(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids, uint32_t n,
                         const uint64_t* mask, const uint32_t* lengths, const uint32_t* boff, uint32_t n_contigs,
                         uint32_t c0, uint32_t c1, uint64_t* ev, uint64_t* counts, uint32_t* err);
uint32_t depth_lds_contigs();  // contig tables up to this many contigs are staged in LDS
uint32_t depth_chunks(uint32_t positions);
void launch_depth_sums(hipStream_t st, const uint64_t* ev, uint32_t positions, uint64_t* sums);
void launch_depth_consume(hipStream_t st, const uint64_t* ev, uint32_t positions, const uint64_t* sums, uint32_t M,
                          const uint32_t* c_lo, const uint32_t* c_hi, const uint32_t* c_row, uint32_t n_c,
                          const uint32_t* r_lo, const uint32_t* r_hi, const uint32_t* r_row, uint32_t n_r,
                          bool scope_regions, uint32_t n_rows, uint64_t* acc64, uint32_t* acc32, uint32_t n_bins,
                          uint64_t* hist);

// the depth track of qmcp_hip_depth_track_* (kernels/depth_track.inc.hip; api/depth_track.inc.hip drives it) over the event
// words, chunk sums and chunks of the depth report: a batch's runs of equal (depth_in, depth_kept, short) inside the scope
// intervals s_lo / s_hi (sorted, disjoint: the merged regions, or the contigs), counted and then written.  cnt: 3 x
// depth_chunks(positions) words, totals: 3 words (runs, emitted positions, short positions in scope); launch_track_emit
// takes cnt as launch_track_count left it, with the same M, flags and depth_cap, and writes totals[0] records
void launch_track_count(hipStream_t st, const uint64_t* ev, uint32_t positions, const uint64_t* sums, uint32_t M,
                        uint32_t flags, uint32_t depth_cap, const uint32_t* s_lo, const uint32_t* s_hi, uint32_t n_s,
                        uint32_t* cnt, uint64_t* totals);
void launch_track_emit(hipStream_t st, const uint64_t* ev, uint32_t positions, const uint64_t* sums, uint32_t M,
                       uint32_t flags, uint32_t depth_cap, const uint32_t* s_lo, const uint32_t* s_hi, uint32_t n_s,
                       const uint32_t* c_lo, const uint32_t* c_hi, const uint32_t* c_row, uint32_t n_c,
                       const uint32_t* cnt, qmcp_hip_track_run* runs);

// duplicate-aware downsampling (kernels/dedup.inc.hip; api/dedup.inc.hip drives them; keys and forms: dedup_plan.h): the
// ranges and validation of a call (out: 9 words preset to {~0u, 0, ~0u, 0, ~0u, 0, 0, 0, 0} -- tag, quality and span min /
// max over the placed reads, err as launch_bc_keys, placed reads, pairs without a placed mate), a round's keys of the reads
// (key_bytes 4 or 8; idx == NULL: record j is read j) and of the units (cid: dense cell ids, idu for an unplaced mate),
// head flags over the n_act active records of a sorted order (form: DedupSortForm; compared on the keys above low_bits, or
// on the columns / cell ids after a sort field by field), the cell ids scattered to input order, survivor and duplicate
// bits + every family's first position from the scanned flags E, the family statistics (counters: families, duplicate
// units, largest, families above `keep`; keep == 1 for dedup: the units beyond the first `keep` of a family are its
// duplicates; hist_bins <= dedup_hist_max()), and the stable compaction of the survivors
uint32_t dedup_hist_max();
void launch_dd_range(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                     const uint32_t* tags, const uint32_t* q, uint32_t n, const uint32_t* lengths, uint32_t n_contigs,
                     bool pairs, uint32_t* out);
void launch_dd_read_keys(hipStream_t st, uint32_t key_bytes, const uint32_t* starts, const uint32_t* ends,
                         const uint32_t* ids, const uint32_t* tags, const uint32_t* q, const uint32_t* idx,
                         const uint64_t* poff, uint64_t ltot, uint32_t n, uint32_t min_span, uint32_t tag_min,
                         uint32_t q_max, const DedupPack& pack, void* keys);
void launch_dd_pair_keys(hipStream_t st, uint32_t key_bytes, const uint32_t* cid, const uint32_t* q, const uint32_t* idx,
                         uint32_t n_units, uint32_t idu, uint32_t q_min, uint32_t score_max, const DedupPack& pack,
                         void* keys);
void launch_dd_heads(hipStream_t st, uint32_t form, const void* sorted, const uint32_t* svals, uint32_t low_bits,
                     uint32_t n_act, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                     const uint32_t* tags, const uint32_t* cid, uint32_t* flag);
void launch_dd_cell_ids(hipStream_t st, const uint32_t* vals, uint32_t stride, const uint32_t* E, uint32_t n_placed,
                        uint32_t n, uint32_t idu, uint32_t* cid);
void launch_dd_segments(hipStream_t st, bool pairs, const uint32_t* vals, uint32_t stride, const uint32_t* E,
                        uint32_t n_act, uint64_t* surv, uint64_t* dup, uint32_t* headpos);
void launch_dd_family_stats(hipStream_t st, const uint32_t* headpos, const uint32_t* n_fam, uint32_t n_act, uint32_t keep,
                            uint32_t hist_bins, uint64_t* hist, uint64_t* counters);
void launch_dd_compact(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                       const uint64_t* surv, const uint32_t* word_base, uint32_t n, uint32_t* starts_c, uint32_t* ends_c,
                       uint32_t* ids_c, uint32_t* orig);

// start cap (kernels/start_cap.inc.hip; api/start_cap.inc.hip drives them; the range pass, the family statistics and the
// compaction are dedup's): a round's keys of the reads from {span_max - span, prio_max - prio, group - group_min, gstart},
// head flags over the n_act placed records of a sorted order (on the keys above low_bits, or on contig, start and group
// after a sort field by field), every cell's first position from the scanned flags E (headpos: cells + 1 entries),
// survivor bits below rank `cap` and capped bits from there on (capped may be NULL), and the kept members per cell under
// the final mask (cnt: one zeroed word per cell; counters, zeroed: cells with a kept member, the largest count)
void launch_sc_keys(hipStream_t st, uint32_t key_bytes, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                    const uint32_t* groups, const uint32_t* prio, const uint32_t* idx, const uint64_t* poff, uint64_t ltot,
                    uint32_t n, uint32_t span_max, uint32_t prio_max, uint32_t group_min, const DedupPack& pack,
                    void* keys);
void launch_sc_cell_flags(hipStream_t st, uint32_t form, const void* sorted, const uint32_t* svals, uint32_t low_bits,
                          uint32_t n_act, const uint32_t* starts, const uint32_t* ids, const uint32_t* groups,
                          uint32_t* flag);
void launch_sc_heads(hipStream_t st, const uint32_t* E, uint32_t n_act, uint32_t* headpos);
void launch_sc_rank(hipStream_t st, const uint32_t* vals, uint32_t stride, const uint32_t* E, const uint32_t* headpos,
                    uint32_t n_act, uint32_t cap, uint64_t* surv, uint64_t* capped);
void launch_sc_kept_cells(hipStream_t st, const uint32_t* vals, uint32_t stride, const uint32_t* E, uint32_t n_act,
                          const uint64_t* mask, uint32_t* cnt, uint64_t* counters);

// amplicon assignment and primer clipping (kernels/amplicon_clip.inc.hip; api/amplicon_clip.inc.hip drives it): the
// units (pairs of reads, or single reads) validated, filtered, assigned to an amplicon of their contig (tab:
// amplicon_assign.h's AssignTable::words on the device; at most kAcLdsMax amplicons are staged in LDS, more are read
// from global memory) and clipped to its insert.  label: one word per unit; unit_keep: one bit per unit; cs / ce / ci:
// the solve columns, one word per read; rs / re / ri (all NULL or all given): the columns rebased to the insert with the
// amplicon as id; used: n_amp zeroed words; partials: ac_partial_rows() x kAcCounts words; totals: kAcCounts words, the
// counters below; err as launch_bc_keys.  With pairs every column is read and written as uint2: 8-byte aligned.
enum AcCount : uint32_t {
    kAcAssigned = 0,    // units with an amplicon
    kAcFiltered = 1,    // units dropped by the length / MAPQ filters
    kAcNoAmplicon = 2,  // units that passed the filters and lie in no amplicon
    kAcSeveral = 3,     // assigned units that more than one amplicon contains
    kAcShortened = 4,   // reads that lost bases and kept some
    kAcAway = 5,        // reads wholly outside the insert
    kAcBases = 6,       // bases clipped off the reads of assigned units
    kAcUnused = 7,      // amplicons no unit was assigned to (k_ac_totals counts them)
    kAcCounts = 8
};
uint32_t ac_partial_rows();
void launch_amplicon_clip(hipStream_t st, bool pairs, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids,
                          const uint32_t* seq_lengths, const uint32_t* qualities, uint64_t n_units,
                          const uint32_t* lengths, uint32_t n_contigs, const uint32_t* amp_offs, const uint32_t* tab,
                          uint32_t n_amp, uint32_t min_length, uint32_t min_mapq, bool per_amplicon, uint32_t* label,
                          uint64_t* unit_keep, uint32_t* cs, uint32_t* ce, uint32_t* ci, uint32_t* rs, uint32_t* re,
                          uint32_t* ri, uint32_t* used, uint64_t* partials, uint64_t* totals, uint32_t* err);

// pair-aware downsampling (kernels/pairs.inc.hip; api/pairs.inc.hip drives them), one batch of the by-contig grouping and
// one stage after the first: the input-order mask of the kept set S as bits in the batch's grouped order (in_bits) and
// its complement inside the batch (rest_bits: the stage's candidates), ceil(n / 64) words each; the events of the batch's
// reads in S on its concatenated axis (ev: pair_credit_pad() + positions + 1 zeroed words; starts / ends: the batch's
// gathered columns; pos_off: the batch-local position offset of each of its contigs) -- launch_exclusive_scan over the
// whole buffer, in place, leaves credit[p] at ev[pair_credit_pad() + p]; need[p] = min(cov_rest(p), max(0, target -
// credit[p])) with launch_profile_need's cut bit and counters; and *count += the set bits of a mask
uint32_t pair_credit_pad();
void launch_pair_gather_mask(hipStream_t st, const void* sorted, uint32_t n, const uint64_t* mask, uint64_t* in_bits,
                             uint64_t* rest_bits);
void launch_pair_credit_events(hipStream_t st, const void* sorted, uint32_t n, const uint64_t* in_bits,
                               const uint32_t* starts, const uint32_t* ends, const uint32_t* pos_off, uint32_t first_contig,
                               uint32_t* ev);
void launch_pair_need(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, const uint32_t* credit, uint32_t ltot,
                      uint32_t target, uint32_t* need, unsigned long long* pstat, bool count_asked = false);
void launch_pair_count_bits(hipStream_t st, const uint64_t* mask, uint32_t n_words, unsigned long long* count);

// tiered downsampling (kernels/tiers.inc.hip; api/tiers.inc.hip drives them).  Its keys are launch_st_keys with a
// none_count (zeroed by the caller: += the reads whose stratum -- tier -- is QMCP_NO_STRATUM), its need is
// launch_pair_need with count_asked (pstat[2] += the positions with need > 0).  launch_tier_keep_list appends the reads
// that `mask` keeps of one solved batch (its gathered columns, its grouped Rec records, word_base: the mask's scanned
// word popcounts; key_base = tier * n_contigs) to the kept list at `out`, 16-byte entries {contig, start, end, 0}, in
// grouped order, at most `room` of them.  launch_tier_credit_events adds the events of the list's n_list entries that
// lie on the contigs [first_contig, first_contig + n_contigs) to launch_pair_credit_events' axis (same layout, same
// scan).
constexpr size_t kTierKeptBytes = 16;
void launch_tier_keep_list(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const void* sorted,
                           const uint64_t* mask, const uint32_t* word_base, uint32_t n, uint32_t key_base, void* out,
                           uint32_t room);
void launch_tier_credit_events(hipStream_t st, const void* list, uint32_t n_list, uint32_t first_contig, uint32_t n_contigs,
                               const uint32_t* pos_off, uint32_t* ev);

// template-aware downsampling (kernels/templates.inc.hip; api/templates.inc.hip drives them): ids holds one template id
// per segment, n <= 2^31.  Once per call: err |= 1 for an id >= n_templates, sizes[id] (n_templates zeroed words) counts
// the segments, tstat (10 zeroed counters) takes the size histogram [0 .. 7], the templates in use [8] and the largest
// size [9].  Per completion: flags (ceil(n_templates / 32) zeroed words) |= the ids of the segments set in mask; then
// mask = the segments whose template is flagged, whole words stored, no bit at or beyond n, and *count += its set bits
void launch_tpl_check_sizes(hipStream_t st, const uint32_t* ids, uint32_t n, uint32_t n_templates, uint32_t* err,
                            uint32_t* sizes, unsigned long long* tstat);
void launch_tpl_mark(hipStream_t st, const uint64_t* mask, const uint32_t* ids, uint32_t n, uint32_t n_templates,
                     uint32_t* flags);
void launch_tpl_spread(hipStream_t st, const uint32_t* ids, uint32_t n, uint32_t n_templates, const uint32_t* flags,
                       uint64_t* mask, unsigned long long* count);

// fragment depth (kernels/fragments.inc.hip; api/fragments.inc.hip drives them).  fstat: the call's counters, zeroed by the
// caller.  launch_frag_check, once per call over the rows in input order: kFragErr |= 1 for a contig id that is neither
// < n_contigs nor QMCP_NO_CONTIG, |= 2 for a placed row with start > end or end >= its contig's length; kFragPlaced and
// kFragBasesIn over the valid placed rows.  launch_frag_keys: a round's u64 keys (fragment_plan.h: FragmentRound), row j
// being idx[j] (idx == NULL: j).  launch_frag_scan_apply: idx is the input index of every row in the order (template,
// contig, start, input index); spine holds frag_spine_bytes(n) bytes; starts_out / cids_out (n words each, input order)
// take every row's clipped start and contig id; tflags (a bitset of n_templates bits, zeroed by the caller) takes the
// templates with a clipped or emptied segment.  frag_tile_rows(): the rows of one scan tile.
enum FragWord : uint32_t {
    kFragPlaced = 0,  // placed rows
    kFragBasesIn,     // their bases
    kFragClipped,     // rows whose start moved
    kFragEmptied,     // rows that lie inside what their group's earlier members cover
    kFragRemoved,     // the bases taken off both kinds
    kFragMaxGroup,    // most placed rows of one template on one contig
    kFragOverlapT,    // templates with a clipped or emptied row
    kFragErr,
    kFragWords
};
uint32_t frag_tile_rows();
size_t frag_spine_bytes(uint32_t n);
void launch_frag_check(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* cids, uint32_t n,
                       const uint32_t* lengths, uint32_t n_contigs, unsigned long long* fstat);
void launch_frag_keys(hipStream_t st, const uint32_t* starts, const uint32_t* cids, const uint32_t* tids, const uint32_t* idx,
                      uint32_t n, uint32_t start_bytes, uint32_t contig_bytes, uint32_t template_bytes, void* keys);
void launch_frag_scan_apply(hipStream_t st, const uint32_t* idx, const uint32_t* starts, const uint32_t* ends,
                            const uint32_t* cids, const uint32_t* tids, uint32_t n, uint32_t n_templates, void* spine,
                            uint32_t* starts_out, uint32_t* cids_out, uint32_t* tflags, unsigned long long* fstat);

// template-aware downsampling under a cap table (kernels/templates_profile.inc.hip; api/templates_profile.inc.hip drives
// them).  launch_tpl_profile_need is launch_pair_need with the target replaced by a region table as launch_profile_need
// takes it (the batch's regions in its global positions, ascending and disjoint, caps already scaled to the stage):
// need[p] = min(cov_rest(p), max(0, cap(p) - credit[p])), the cut bit, the two counters.  launch_tpl_on_cap, once per
// call over the segments in input order: roffs (n_contigs + 1) gives contig c the regions [roffs[c], roffs[c + 1]) of
// rs / re / cap in contig positions, before[k] the positions below rs[k] of its contig whose cap is positive
// (cap_table.h: cap_positive_before); a placed segment that covers a position with a positive cap sets its template's
// bit in flags (ceil(n_templates / 32) zeroed words) and adds one to *count
void launch_tpl_profile_need(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, const uint32_t* credit, uint32_t ltot,
                             const uint32_t* rs, const uint32_t* re, const uint32_t* cap, uint32_t n_regions,
                             uint32_t default_cap, uint32_t* need, unsigned long long* pstat);
void launch_tpl_on_cap(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                       const uint32_t* tids, uint32_t n, uint32_t n_contigs, uint32_t n_templates, const uint32_t* roffs,
                       const uint32_t* rs, const uint32_t* re, const uint32_t* cap, const uint32_t* before,
                       bool default_positive, uint32_t* flags, unsigned long long* count);

// ceiling downsampling (kernels/ceiling.inc.hip; api/ceiling.inc.hip drives them).  The region table and boff / eoff as
// launch_profile_need takes them.  launch_ceiling_need: need[p] = max(0, cov(p) - cap(p)), the cut bit where need(p) ==
// cov(p) (cov == 0 or cap == 0).  launch_ceiling_check, once the batch's D is marked: depth[p] (16-byte aligned) is the
// depth of D, kept(p) = cov(p) - depth[p] is held against cap(p) and min(cov(p), cap(p)).  launch_ceiling_finish, once per
// call: mask (ceil(n_reads / 64) words, input order) holds D and leaves as placed & ~D, with whole_pairs after the mates
// (2q, 2q + 1) of D's reads have joined D.  cst: kCeilingStatWords counters, zeroed by the caller.
enum CeilingStat : uint32_t {
    kCeilOverPositions = 0,  // positions with cov > cap
    kCeilOverBases,          // the sum of need
    kCeilMaxNeed,            // the largest need (cleared per batch: it plans the batch's sweep)
    kCeilExcessPositions,    // positions with kept > cap
    kCeilShortPositions,     // positions with kept < min(cov, cap)
    kCeilShortBases,         // the sum of that shortfall
    kCeilMaxKept,            // the largest kept depth
    kCeilPlaced,             // placed reads
    kCeilKept,               // placed reads outside D (and outside its mates, when they are joined)
    kCeilMatesDropped,       // placed reads dropped only as mates
    kCeilingStatWords = 12
};
void launch_ceiling_need(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, uint32_t ltot, const uint32_t* rs,
                         const uint32_t* re, const uint32_t* cap, uint32_t n_regions, uint32_t default_cap, uint32_t* need,
                         unsigned long long* cst);
void launch_ceiling_check(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, const uint32_t* depth, uint32_t ltot,
                          const uint32_t* rs, const uint32_t* re, const uint32_t* cap, uint32_t n_regions,
                          uint32_t default_cap, unsigned long long* cst);
void launch_ceiling_finish(hipStream_t st, const uint32_t* ids, uint64_t n_reads, bool whole_pairs, uint64_t* mask,
                           unsigned long long* cst);

// proportional downsampling (kernels/proportional.inc.hip; api/proportional.inc.hip drives them).  boff / eoff as
// launch_profile_need takes them.  launch_prop_need: need[p] = min(cov(p), max_coverage, max(ceil(cov(p) * num / den),
// floor_depth)) in exact integers (num <= den <= QMCP_PROPORTION_DEN_MAX), the cut bit where need(p) == cov(p).
// launch_prop_tally, once per call: starts / ends / ids are the call's columns in input order, mask (ceil(n_reads / 64)
// words) its final keep mask.  pst: kPropStatWords counters, zeroed by the caller.
enum PropStat : uint32_t {
    kPropDemand = 0,       // the sum of need
    kPropWholePositions,   // positions with cov > 0 and need == cov
    kPropFloorPositions,   // positions with q < min(floor, cov, max_coverage)
    kPropCappedPositions,  // positions with max(q, floor) > max_coverage and cov > max_coverage
    kPropMaxDepth,         // the largest depth (cleared per batch, with the next: the host keeps the call's maxima)
    kPropMaxNeed,          // the largest need (it plans the batch's sweep)
    kPropPlaced,           // placed reads
    kPropBasesIn,          // the sum of their spans
    kPropBasesKept,        // the sum of the kept reads' spans
    kPropStatWords = 12
};
void launch_prop_need(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, uint32_t ltot, uint32_t num, uint32_t den,
                      uint32_t floor_depth, uint32_t max_coverage, uint32_t* need, unsigned long long* pst);
void launch_prop_tally(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids, uint64_t n_reads,
                       const uint64_t* mask, unsigned long long* pst);

// budget downsampling (kernels/budget.inc.hip; api/budget.inc.hip drives them).  launch_budget_tally: cov[0 .. ltot) is a
// batch's per-position depth; hist (H bins, H <= kBudgetBinsMax) takes min(cov, H - 1), acc the largest depth and the sum of
// the depths -- both live across the batches of a call, zeroed by the caller.  launch_budget_curve, once: curve[M] =
// sum over positions of min(cov, M), M = 0 .. H - 1.  launch_budget_finish, per probe under QMCP_BUDGET_WHOLE_PAIRS: mask
// (ceil(n_reads / 64) words, input order, n_reads even) leaves with the mates (2q, 2q + 1) joined among the placed reads,
// its popcount added to acc[kBudgetKept].
static constexpr uint32_t kBudgetBinsMax = QMCP_BUDGET_CURVE_MAX + 1u;  // 32 KiB of LDS per workgroup
enum BudgetWord : uint32_t {
    kBudgetMaxDepth = 0,  // the largest depth
    kBudgetTotalBases,    // the sum of the depths
    kBudgetKept,          // a probe's reads after pair completion (cleared per probe)
    kBudgetWords = 4
};
void launch_budget_tally(hipStream_t st, const uint32_t* cov, uint32_t ltot, uint32_t H, unsigned long long* acc,
                         unsigned long long* hist);
void launch_budget_curve(hipStream_t st, const unsigned long long* hist, uint32_t H, unsigned long long* curve);
void launch_budget_finish(hipStream_t st, const uint32_t* ids, uint64_t n_reads, uint64_t* mask, unsigned long long* acc);

// mean-depth downsampling (kernels/mean_depth.inc.hip; api/mean_depth.inc.hip drives them, with launch_budget_curve and
// launch_budget_finish above, and launch_budget_tally when there is no region table).  launch_md_tally: launch_budget_tally
// with the histogram and the sum taken over the region positions of the batch only -- merged region k of the batch starts
// at rpos[k] on the batch's concatenated axis and holds the ranks from rcum[k] on, n_pos positions in all -- while
// acc[kBudgetMaxDepth] still takes the largest depth of ALL ltot positions.  launch_md_weights, once per call: w[i] = the
// positions of read i inside its contig's merged regions (offs / rs / re / cum: target_table.h's table, contig
// coordinates), or its span without a table; 0 for an unplaced read.  launch_md_count, per probe: acc[kMdBases] += the sum
// of w over the set bits of the input-order mask, acc[kMdKept] += their number (both cleared by the caller).
enum MeanDepthWord : uint32_t {
    kMdBases = 0,  // a probe's kept bases inside the regions
    kMdKept,       // a probe's kept reads
    kMdWords = 2
};
void launch_md_tally(hipStream_t st, const uint32_t* cov, uint32_t ltot, const uint32_t* rpos, const uint32_t* rcum,
                     uint32_t n_reg, uint32_t n_pos, uint32_t H, unsigned long long* acc, unsigned long long* hist);
void launch_md_weights(hipStream_t st, const uint32_t* starts, const uint32_t* ends, const uint32_t* ids, uint32_t n,
                       uint32_t n_contigs, bool has_table, const uint32_t* offs, const uint32_t* rs, const uint32_t* re,
                       const uint32_t* cum, uint32_t n_regions, uint32_t* w);
void launch_md_count(hipStream_t st, const uint64_t* mask, const uint32_t* w, uint64_t n_reads, unsigned long long* acc);

// coverage thresholds (kernels/thresholds.inc.hip; api/thresholds.inc.hip drives them).  thr has one 16-bit threshold per
// read and holds kThresholdNever everywhere before the first step.  launch_thresholds_step, per coverage M: the reads of
// the input-order `mask` that `seen` lacks get thr = M and join seen; acc[kThSeen] += their number, acc[kThViolations] +=
// the reads of seen that the mask lacks.  launch_thresholds_finish, once: under whole_pairs a placed read (ids) takes the
// smaller of its own and its placed mate's threshold; hist[t - lo] += 1 for every read with final threshold t (n_bins
// bins, zeroed by the caller; in LDS per workgroup up to kThresholdsBinsMax bins).  launch_thresholds_counts: hist's
// running sum in place.
static constexpr uint32_t kThresholdsBinsMax = 8192u;  // 32 KiB of LDS per workgroup
enum ThresholdsAccWord : uint32_t {
    kThSeen = 0,     // reads with a threshold so far
    kThViolations,   // (read, M) pairs in which a read with a threshold is not kept
    kThWords = 2
};
void launch_thresholds_step(hipStream_t st, const uint64_t* mask, uint64_t* seen, uint64_t n_reads, uint32_t M,
                            uint16_t* thr, unsigned long long* acc);
void launch_thresholds_finish(hipStream_t st, const uint32_t* ids, uint64_t n_reads, bool whole_pairs, uint32_t lo,
                              uint32_t n_bins, uint16_t* thr, unsigned long long* hist);
void launch_thresholds_counts(hipStream_t st, unsigned long long* counts, uint32_t n_bins);

// disjoint replicates (kernels/replicates.inc.hip; api/replicates.inc.hip drives them).  A replicate's candidates are n
// reads in three columns with an origin column (origin_in: the grouping's Rec{key, index} array when `first`, a plain
// column of input indices otherwise); `taken` has one bit per candidate (the solve's mask, or the input-order taken mask
// gathered through the origin) and taken_base its scanned word popcounts with the total behind the last word.
// launch_rep_split: the candidates that are NOT taken go, stably, to the other column set (16-byte aligned: the call's
// own buffers); label != 0: labels[origin] = label for the taken ones.  kRepTileReads: the candidates one workgroup
// takes at a time.  launch_rep_offsets: next[k] = offs[k] - (taken candidates before offs[k]) for k in [0, n_contigs].
// launch_rep_mark: labels[origin] = label and the origin's bit in the input-order mask taken_in for the candidates a
// solve kept; launch_rep_gather_taken: that mask's bits in candidate order; launch_rep_label_input: labels[i] = label
// for the set bits of an input-order mask; launch_rep_complete_pairs: a placed read with label 0 whose mate (2q, 2q + 1)
// carries `label` gets it too, with its bit in taken_in, *n_mates += the reads that joined; launch_rep_label_mask: the
// packed mask of labels == label.
static constexpr uint32_t kRepTileReads = 1024;
void launch_rep_split(hipStream_t st, bool first, const uint32_t* starts, const uint32_t* ends, const void* origin_in,
                      const uint64_t* taken, const uint32_t* taken_base, uint32_t n, uint32_t label, uint8_t* labels,
                      uint32_t* starts_f, uint32_t* ends_f, uint32_t* origin_f);
void launch_rep_offsets(hipStream_t st, const uint32_t* offs, uint32_t n_contigs, const uint64_t* taken,
                        const uint32_t* taken_base, uint32_t* next);
void launch_rep_mark(hipStream_t st, const uint64_t* kept, const uint32_t* origin, uint32_t n, uint32_t label,
                     uint8_t* labels, uint64_t* taken_in);
void launch_rep_gather_taken(hipStream_t st, bool first, const void* origin_in, uint32_t n, const uint64_t* taken_in,
                             uint64_t* taken);
void launch_rep_label_input(hipStream_t st, const uint64_t* mask, uint64_t n_reads, uint32_t label, uint8_t* labels);
void launch_rep_complete_pairs(hipStream_t st, const uint32_t* ids, uint64_t n_reads, uint32_t label, uint8_t* labels,
                               uint64_t* taken_in, unsigned long long* n_mates);
void launch_rep_label_mask(hipStream_t st, const uint8_t* labels, uint64_t n_reads, uint32_t label, uint64_t* mask);

}  // namespace qmcp
#endif
