// by_contig.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_by_contig_host / _device: reads of several contigs in any order, one contig id per read.
//   1-3. group_reads: k_bc_keys checks every read against its contig and writes the sort keys (contig id; n_contigs for
//      unplaced reads); the stable record radix (api/radix_passes.inc.hip) groups {key, read index} by key, one pass per
//      8 bits of n_contigs, into the context's own record buffers (the solves below never touch them); k_bc_bounds turns
//      the sorted keys into each contig's run; the bounds and the validation word come back to the host
//   4. by_contig_plan.h packs the contigs into batches within one call's limits; per batch solve_gathered_batch: its
//      columns gathered in grouped order, solved by the ordinary multi-contig solve, its mask ORed back into input order
// Grouping happens once; a batch only gathers its own reads.
// A coverage ladder (api/ladder.inc.hip) is this call with further levels run inside each batch, on its gathered columns.
// A coverage profile (api/profile.inc.hip) is this call with every batch solved under its own regions' caps; a ceiling
// solve (api/ceiling.inc.hip) is a profile whose batches select the DROPPED reads, complemented once the call is through.
// A pair-aware solve (api/pairs.inc.hip) is this call at its first target, with the further stages run over all batches
// once the last batch's mask is in place.
// A replicate split (api/replicates.inc.hip) is this call at its first coverage, with the further replicates run over all
// batches on the reads still free.
// A budget solve (api/budget.inc.hip) is this call's grouping and batches under a search of its own: several whole solves,
// each over every batch, at the coverages budget_plan.h picks.
namespace {

struct LadderRun;
int ladder_levels_of_batch(qmcp_hip_ctx* c, LadderRun& ld, const void* bsorted, uint32_t nb, const uint64_t* roff,
                           const uint32_t* lengths, uint32_t n_contigs);
struct ProfileRun;
int profile_solve_batch(qmcp_hip_ctx* c, ProfileRun& pf, const void* bsorted, const uint32_t* d_starts, const uint32_t* d_ends,
                        const uint64_t* roff, const uint32_t* lengths, uint32_t first_contig, uint32_t n_contigs,
                        uint64_t n64, uint64_t* d_mask, qmcp_hip_stats* st);
struct PairRun;
int pair_later_stages(qmcp_hip_ctx* c, PairRun& pr, const void* sorted, const std::vector<uint32_t>& offs,
                      const std::vector<qmcp::ContigBatch>& batches, const uint32_t* d_starts, const uint32_t* d_ends,
                      const uint32_t* lengths, uint64_t n64, uint64_t* d_mask, const qmcp_hip_stats& first);
struct ReplicatesRun;
int replicates_later(qmcp_hip_ctx* c, ReplicatesRun& rp, const void* sorted, const std::vector<uint32_t>& offs,
                     const std::vector<qmcp::ContigBatch>& batches, const uint32_t* d_starts, const uint32_t* d_ends,
                     const uint32_t* d_ids, const uint32_t* lengths, uint32_t n_contigs_all, uint64_t n64, uint64_t* d_mask,
                     const qmcp_hip_stats& first);

// the batches' stats as one: counts and times summed, the route of the batch with the most reads
void add_batch_stats(qmcp_hip_stats& s, const qmcp_hip_stats& b, bool first, bool largest) {
    s.n_reads += b.n_reads;
    s.n_kept += b.n_kept;
    s.min_span = first ? b.min_span : std::min(s.min_span, b.min_span);
    s.max_span = first ? b.max_span : std::max(s.max_span, b.max_span);
    s.sweep_stretches += b.sweep_stretches;
    s.ms_total += b.ms_total;
    s.ms_prepare += b.ms_prepare;
    s.ms_scan += b.ms_scan;
    s.ms_sort += b.ms_sort;
    s.ms_sweep += b.ms_sweep;
    s.ms_mark += b.ms_mark;
    s.spec_boundaries += b.spec_boundaries;
    s.spec_mismatches += b.spec_mismatches;
    s.spec_retry_mismatches += b.spec_retry_mismatches;
    s.sweep_blocks_changed += b.sweep_blocks_changed;
    s.sweep_blocks += b.sweep_blocks;
    s.arena_grown_mid_solve += b.arena_grown_mid_solve;
    s.near_uniform_exceptions += b.near_uniform_exceptions;
    s.near_uniform_selected += b.near_uniform_selected;
    if (largest) {
        s.path = b.path;
        s.sort_passes = b.sort_passes;
        s.near_uniform_rounds = b.near_uniform_rounds;
        s.near_uniform_giveup = b.near_uniform_giveup;
    }
}

// the timing spans of one grouping
struct GroupNames {
    RadixNames radix;
    const char* bounds;
};

// Steps 1-3 for every entry that groups reads by a key of its own.  The grouping buffers (bc_*) are sized, the mask and
// the error word cleared and the contig lengths uploaded; queue_keys() then queues the caller's key kernel (it reads
// bc_len and writes bc_key and bc_err); the keys are sorted into {key, index} records, k_bc_bounds turns them into the
// n_groups runs, and the n_groups + 1 offsets and the error word come back to the host (the one wait).  `sorted` is the
// record buffer that holds the grouped records; what the error bits mean is the caller's business.
template <typename QueueKeys>
int group_reads(qmcp_hip_ctx* c, uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, uint32_t n_groups,
                uint32_t passes, const GroupNames& nm, QueueKeys queue_keys, uint64_t* d_mask, std::vector<uint32_t>& offs,
                const void** sorted, uint32_t* err) {
    const uint32_t n = (uint32_t)n64;
    const size_t words = (size_t)((n64 + 63) / 64);
    const uint32_t n_tiles = qmcp::sort_tiles(n);
    hipStream_t st = c->stream;
    TRY(ensure(c, c->bc_len, (size_t)n_contigs * sizeof(uint32_t)));
    TRY(ensure(c, c->bc_offs, ((size_t)n_groups + 1) * sizeof(uint32_t)));
    TRY(ensure(c, c->bc_err, 16));
    TRY(ensure(c, c->bc_key, (size_t)n * sizeof(uint32_t)));
    TRY(ensure(c, c->bc_rec[0], (size_t)n * 2 * sizeof(uint32_t)));
    TRY(ensure(c, c->bc_rec[1], (size_t)n * 2 * sizeof(uint32_t)));
    TRY(ensure(c, c->bc_hist, (size_t)256 * n_tiles * sizeof(uint32_t)));
    TRY(ensure(c, c->bc_spine, (size_t)qmcp::scan_spine_entries(256u * n_tiles) * sizeof(uint32_t) + 16));
    if (words) HIP_TRY(hipMemsetAsync(d_mask, 0, words * sizeof(uint64_t), st));
    HIP_TRY(hipMemsetAsync(c->bc_err.p, 0, sizeof(uint32_t), st));
    HIP_TRY(hipMemcpyAsync(c->bc_len.p, lengths, (size_t)n_contigs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    queue_keys();
    int k = 0;
    if (n)
        TRY(radix_sort_records(c, st, (const uint32_t*)c->bc_key.p, n, passes, (uint32_t*)c->bc_hist.p,
                               (uint32_t*)c->bc_spine.p, c->bc_rec, nm.radix, &k));
    *sorted = c->bc_rec[k].p;
    {
        KernelSpan sp(c, nm.bounds);
        qmcp::launch_bc_bounds(st, *sorted, n, n_groups, (uint32_t*)c->bc_offs.p);
    }
    HIP_TRY(hipGetLastError());
    offs.assign((size_t)n_groups + 1, 0);
    *err = 0;
    HIP_TRY(hipMemcpyAsync(offs.data(), c->bc_offs.p, offs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(err, c->bc_err.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return QMCP_OK;
}

// the batch with the most reads (its route is the call's), and the gathered columns and the mask sized for it
template <typename Batch>
int reserve_batch_buffers(qmcp_hip_ctx* c, const std::vector<Batch>& batches, size_t* largest) {
    uint64_t most = 0;
    *largest = 0;
    for (size_t b = 0; b < batches.size(); ++b)
        if (batches[b].n_reads > most) {
            most = batches[b].n_reads;
            *largest = b;
        }
    TRY(ensure(c, c->bc_starts, (size_t)most * sizeof(uint32_t)));
    TRY(ensure(c, c->bc_ends, (size_t)most * sizeof(uint32_t)));
    TRY(ensure(c, c->bc_mask, (size_t)((most + 63) / 64) * sizeof(uint64_t)));
    return QMCP_OK;
}

// a batch's contig_read_offsets from the grouping's offsets: goffs points at its first group, n_contigs + 1 are read
void batch_roff(const uint32_t* goffs, uint32_t n_contigs, std::vector<uint64_t>& roff) {
    roff.resize((size_t)n_contigs + 1);
    for (uint32_t k = 0; k <= n_contigs; ++k) roff[k] = goffs[k] - goffs[0];
}

// One batch of grouped reads (nb > 0 records at bsorted; contigs first_contig .. + n_contigs, offsets from goffs): its
// columns gathered in grouped order, solved by the ordinary multi-contig solve at M (under `profile`'s caps when given),
// its mask ORed back into input order, its stats added to `sum`.  roff is left holding the batch's read offsets.
// gather == false: bc_starts / bc_ends hold this batch's columns already (a budget call of one batch, between its probes).
int solve_gathered_batch(qmcp_hip_ctx* c, const void* bsorted, uint32_t nb, const uint32_t* d_starts, const uint32_t* d_ends,
                         const uint32_t* goffs, const uint32_t* lengths, uint32_t first_contig, uint32_t n_contigs, uint32_t M,
                         ProfileRun* profile, uint64_t* d_mask, std::vector<uint64_t>& roff, qmcp_hip_stats& sum, bool first,
                         bool largest, bool gather = true) {
    hipStream_t st = c->stream;
    const uint32_t* bs_starts = (const uint32_t*)c->bc_starts.p;
    const uint32_t* bs_ends = (const uint32_t*)c->bc_ends.p;
    if (gather) {
        KernelSpan sp(c, "k_bc_gather");
        qmcp::launch_bc_gather(st, bsorted, nb, d_starts, d_ends, (uint32_t*)c->bc_starts.p, (uint32_t*)c->bc_ends.p);
    }
    HIP_TRY(hipGetLastError());
    batch_roff(goffs, n_contigs, roff);
    qmcp_hip_stats bs;
    std::memset(&bs, 0, sizeof(bs));
    if (profile)
        TRY(profile_solve_batch(c, *profile, bsorted, bs_starts, bs_ends, roff.data(), lengths, first_contig, n_contigs, nb,
                                (uint64_t*)c->bc_mask.p, &bs));
    else
        TRY(solve_on_device(c, bs_starts, bs_ends, roff.data(), lengths + first_contig, n_contigs, nb, M,
                            (uint64_t*)c->bc_mask.p, &bs));
    {
        KernelSpan sp(c, "k_bc_scatter_mask");
        qmcp::launch_bc_scatter_mask(st, (const uint64_t*)c->bc_mask.p, bsorted, nb, d_mask);
    }
    HIP_TRY(hipGetLastError());
    add_batch_stats(sum, bs, first, largest);
    return QMCP_OK;
}

int solve_by_contig_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                              uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, uint32_t M, uint64_t* d_mask,
                              qmcp_hip_stats* stats, LadderRun* ladder = nullptr,
                              ProfileRun* profile = nullptr /* then M is the default cap */,
                              PairRun* pairs = nullptr /* then M is the first stage's target */,
                              ReplicatesRun* replicates = nullptr /* then M is the first replicate's coverage */) {
    if (!lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    if (n64 > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n64);
    const uint32_t n = (uint32_t)n64;
    const uint32_t n_groups = n_contigs + 1;  // the contigs, then the unplaced reads
    hipStream_t st = c->stream;

    // 1-3: keys, grouping, bounds
    const uint32_t passes = std::max(1u, (bit_width(n_contigs) + 7) / 8);  // keys go up to n_contigs
    std::vector<uint32_t> offs;
    const void* sorted = nullptr;
    uint32_t err = 0;
    TRY(group_reads(
        c, n64, lengths, n_contigs, n_groups, passes,
        {{"k_radix_hist_rec(by contig)", "scan_radix_hist(by contig, 3 kernels)", "k_radix_scatter_rec(by contig)"},
         "k_bc_bounds"},
        [&] {
            KernelSpan sp(c, "k_bc_keys");
            qmcp::launch_bc_keys(st, d_starts, d_ends, d_ids, n, (const uint32_t*)c->bc_len.p, n_contigs,
                                 (uint32_t*)c->bc_key.p, (uint32_t*)c->bc_err.p);
        },
        d_mask, offs, &sorted, &err));
    if (err & 1u) return fail(QMCP_EINVAL, "a contig id is neither < n_contigs (%u) nor QMCP_NO_CONTIG", n_contigs);
    if (err & 2u) return fail(QMCP_EREAD, "a read has start > end or end >= its contig's length");

    // 4: batches
    std::vector<uint64_t> counts(n_contigs);
    for (uint32_t k = 0; k < n_contigs; ++k) counts[k] = offs[k + 1] - offs[k];
    std::vector<qmcp::ContigBatch> batches;
    uint32_t bad = 0;
    if (qmcp::plan_contig_batches(counts.data(), lengths, n_contigs, batches, &bad) != QMCP_OK)
        return fail(QMCP_ERANGE,
                    "contig %u alone exceeds one call's limits: %llu reads (at most 2^30), %u positions (at most 2^31 - 2)",
                    bad, (unsigned long long)counts[bad], lengths[bad]);
    size_t largest = 0;
    TRY(reserve_batch_buffers(c, batches, &largest));
    qmcp_hip_stats sum;
    std::memset(&sum, 0, sizeof(sum));
    bool first = true;
    std::vector<uint64_t> roff;
    for (size_t b = 0; b < batches.size(); ++b) {
        const qmcp::ContigBatch& bt = batches[b];
        sum.n_contigs += bt.n_contigs;
        sum.total_length += bt.positions;
        if (bt.n_reads == 0) continue;  // (nothing to solve: empty contigs keep nothing)
        const uint32_t nb = (uint32_t)bt.n_reads;
        const void* bsorted = (const uint32_t*)sorted + 2 * bt.first_read;  // {key, index} records
        TRY(solve_gathered_batch(c, bsorted, nb, d_starts, d_ends, offs.data() + bt.first_contig, lengths, bt.first_contig,
                                 bt.n_contigs, M, profile, d_mask, roff, sum, first, b == largest));
        if (ladder) TRY(ladder_levels_of_batch(c, *ladder, bsorted, nb, roff.data(), lengths + bt.first_contig, bt.n_contigs));
        first = false;
    }
    if (pairs) TRY(pair_later_stages(c, *pairs, sorted, offs, batches, d_starts, d_ends, lengths, n64, d_mask, sum));
    if (replicates)
        TRY(replicates_later(c, *replicates, sorted, offs, batches, d_starts, d_ends, d_ids, lengths, n_contigs, n64, d_mask,
                             sum));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    if (stats) *stats = sum;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_by_contig_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends,
                                  const uint32_t* contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                  uint32_t n_contigs, uint32_t max_coverage, uint64_t* keep_mask_out,
                                  qmcp_hip_stats* stats) {
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    TRY(ensure(c, c->mask, words * sizeof(uint64_t)));
    c->mask_reads = 0;
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
    }
    TRY(solve_by_contig_on_device(c, (const uint32_t*)c->in_starts.p, (const uint32_t*)c->in_ends.p,
                                  (const uint32_t*)c->in_aux0.p, n_reads, contig_lengths, n_contigs, max_coverage,
                                  (uint64_t*)c->mask.p, stats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_by_contig_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                    const uint32_t* d_contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                    uint32_t n_contigs, uint32_t max_coverage, uint64_t* d_keep_mask_out,
                                    void* hip_stream, qmcp_hip_stats* stats) {
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(order_after(c, hip_stream));
    return solve_by_contig_on_device(c, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, n_contigs, max_coverage,
                                     d_keep_mask_out, stats);
}

}  // extern "C"
