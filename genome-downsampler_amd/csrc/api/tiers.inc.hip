// tiers.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_tiers_host / _device: reads of several contigs AND several tiers in any order, one coverage M.  Tier 0
// is solved first; tier t >= 1 only fills what the kept reads of the tiers before it leave short of min(coverage, M).
//   1. group_reads (api/by_contig.inc.hip) around k_st_keys<true>: the stratified entry's key  tier * n_contigs + contig
//      (n_tiers * n_contigs for a read without contig or tier), validation, and the count of the reads without a tier
//   2. tiers_plan.h cuts every tier with reads into batches, never across a tier; they run in grouped order, so every
//      batch of the tiers before a batch's own is finished when it begins
//   3. a batch of tier 0: gather_batch and solve_scatter_batch with a PlainSolver at M -- the by-contig call's routes
//   4. a batch of tier t >= 1: a TierSolver -- the batch's credit (k_tier_credit_events over the kept list on a zeroed
//      axis, scanned in place), then capped_solve_batch (api/profile.inc.hip) on the batch's gathered columns with
//      k_pair_need<true> building need[p] = min(cov(p), max(0, M - credit[p])); its three counters come back before the
//      sweep is queued, and a batch that asks for nothing queues none
//   5. after a batch that kept reads, while a later tier has reads: k_word_popcounts -> exclusive scan ->
//      k_tier_keep_list appends the batch's kept reads to the kept list, at the count the solve has just brought back
//      (no wait of its own)
//   6. where rows are asked for, k_st_tally (a tier is a stratum there) reduces the grouped records against the final
//      mask into the rows' bases (n_tiers x 32 bytes come back); the reads and kept reads of a tier are known from the
//      grouping and the solves.  The count of step 1 comes back
// The kept list holds {contig, start, end} of every kept read of every finished batch, in the order the batches ran.  A
// later batch reads the whole list and takes the entries on its own contigs: a call has as many batches per tier as its
// reads and positions need solver calls (one, up to 2^30 reads and 2^31 - 2 positions), and the list holds the kept
// reads only -- about M * positions / span of them, under 1 % of the reads on deep data -- so the filter costs less than
// a table of slices per (tier, contig) and the wait that would bring its offsets back after every batch.
// Buffers: the grouping and the batches live in the by-contig solve's buffers (bc_*), which nothing else uses while
// this call runs; everything else is this file's own (tr_*).  Nothing a solve owns is held across a solve.
namespace {

// Room for `entries` entries in the kept list, of which the first `held` are in use: the list is filled across the
// batches of one call, so when it has to grow what it holds moves to the new block (at least twice the old one).  This
// happens between two solves, never inside one.
int reserve_kept_list(qmcp_hip_ctx* c, size_t entries, size_t held) {
    DevBuf& b = c->tr_list;
    const size_t bytes = entries * qmcp::kTierKeptBytes;
    if (b.cap >= bytes || held == 0) return ensure(c, b, bytes);
    HIP_TRY(hipStreamSynchronize(c->stream));  // (what was queued may still be filling the old block)
    DevBuf fresh;
    TRY(ensure(c, fresh, std::max(bytes, 2 * b.cap)));
    HIP_TRY(hipMemcpy(fresh.p, b.p, held * qmcp::kTierKeptBytes, hipMemcpyDeviceToDevice));
    std::swap(b.p, fresh.p);  // (`fresh` now owns the old block and frees it)
    std::swap(b.cap, fresh.cap);
    return QMCP_OK;
}

// need[] of a batch of a later tier, through k_pair_need<true>: need[] lives in tr_need, the counters in tr_stat[0 .. 2]
struct TierNeed : CappedNeed {
    uint32_t target;
    unsigned long long counters[3] = {0, 0, 0};  // capped positions, demand, asked positions: this batch's
    explicit TierNeed(uint32_t M) : target(M) {}
    const char* name() const override { return "k_pair_need(tiers)"; }
    DevBuf& need_buf(qmcp_hip_ctx* c) override { return c->tr_need; }
    int reserve(qmcp_hip_ctx*) override { return QMCP_OK; }
    int upload(qmcp_hip_ctx* c, hipStream_t st) override {
        HIP_TRY(hipMemsetAsync(c->tr_stat.p, 0, sizeof(counters), st));
        return QMCP_OK;
    }
    void launch(qmcp_hip_ctx* c, hipStream_t st, uint32_t ltot, uint32_t* need) override {
        qmcp::launch_pair_need(st, c->boff.u32(), c->eoff.u32(), c->tr_credit.u32() + qmcp::pair_credit_pad(), ltot, target,
                               need, c->tr_stat.as<unsigned long long>(), true);
    }
    int no_demand(qmcp_hip_ctx* c, hipStream_t st, bool* none) override {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(counters, c->tr_stat.p, sizeof(counters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *none = counters[1] == 0;
        return QMCP_OK;
    }
};

// a batch of a tier after the first: the credit of the kept list's n_listed entries, then the capped route
struct TierSolver : BatchSolver {
    uint32_t M;
    uint32_t n_listed;
    TierNeed need;
    bool swept = false;
    TierSolver(uint32_t m, uint32_t listed) : M(m), n_listed(listed), need(m) {}
    int solve(qmcp_hip_ctx* c, BatchView& v, qmcp_hip_stats* bs) override {
        hipStream_t st = c->stream;
        const uint32_t pad = qmcp::pair_credit_pad();
        const uint32_t ltot = (uint32_t)v.positions;  // (a batch holds at most 2^31 - 2 positions)
        const size_t tab = (size_t)v.n_contigs + 1;
        TRY(ensure(c, c->tr_credit, ((size_t)ltot + pad + 4) * sizeof(uint32_t)));
        TRY(ensure(c, c->tr_cspine, scan_spine_bytes(ltot + pad, 1)));
        TRY(ensure(c, c->tr_poff, tab * sizeof(uint32_t)));
        HIP_TRY(hipMemsetAsync(c->tr_credit.p, 0, ((size_t)ltot + pad) * sizeof(uint32_t), st));
        if (n_listed) {  // (an empty list leaves the zeroed axis: it is its own scan)
            v.tables32();
            HIP_TRY(hipMemcpyAsync(c->tr_poff.p, v.poff32.data(), tab * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            KernelSpan sp(c, "k_tier_credit_events + scan");
            qmcp::launch_tier_credit_events(st, c->tr_list.p, n_listed, v.first_contig, v.n_contigs, c->tr_poff.u32(),
                                            c->tr_credit.u32());
            qmcp::launch_exclusive_scan(st, c->tr_credit.u32(), ltot + pad, c->tr_credit.u32(), c->tr_cspine.u32(), false);
        }
        HIP_TRY(hipGetLastError());
        return capped_solve_batch(c, need, M, c->bc_starts.u32(), c->bc_ends.u32(), v.roff.data(), v.lengths, v.n_contigs,
                                  v.nb, c->bc_mask.u64(), bs, &swept);
    }
};

// what both entries check first, before anything is copied or launched
int check_tiers_entry(const uint32_t* lengths, uint32_t n_contigs, const uint32_t* tiers, uint32_t n_tiers, uint32_t M,
                      uint64_t n64) {
    qmcp::TierRefusal why = qmcp::kTierCallOk;
    const int rc = qmcp::check_tiers_call(lengths != nullptr, n_contigs, tiers != nullptr, n_tiers, M, n64, &why);
    switch (why) {
        case qmcp::kTierCallOk: return QMCP_OK;
        case qmcp::kTierNoContigs: return fail(rc, "contig_lengths missing or n_contigs == 0");
        case qmcp::kTierNoColumn: return fail(rc, "tiers missing");
        case qmcp::kTierNoTiers: return fail(rc, "n_tiers == 0: a tiered call needs at least one tier");
        case qmcp::kTierTooManyTiers:
            return fail(rc, "n_tiers %u exceeds %u per tiered call", n_tiers, (unsigned)QMCP_TIERS_MAX);
        case qmcp::kTierTooManyGroups:
            return fail(rc, "n_tiers %u x n_contigs %u = %llu exceeds 2^24 (tier, contig) groups per call", n_tiers, n_contigs,
                        (unsigned long long)((uint64_t)n_tiers * n_contigs));
        case qmcp::kTierCoverage: return fail(rc, "max_coverage %u is 2^31 or more", M);
        case qmcp::kTierTooManyReads:
            return fail(rc, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n64);
    }
    return fail(QMCP_EINVAL, "the tiered call was refused");
}

int solve_tiers_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                          const uint32_t* d_tiers, uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, uint32_t M,
                          uint32_t n_tiers, uint64_t* d_mask, qmcp_hip_tier_row* rows_out, qmcp_hip_stats* stats,
                          qmcp_hip_tiers_stats* tstats) {
    const uint32_t n = (uint32_t)n64;
    const uint32_t n_pairs = n_tiers * n_contigs;  // the (tier, contig) groups, <= 2^24
    const uint32_t n_groups = n_pairs + 1;         // ... then the reads without contig or tier
    hipStream_t st = c->stream;
    const size_t row_bytes = (size_t)n_tiers * 4 * sizeof(uint64_t);  // k_st_tally's rows
    TRY(ensure(c, c->tr_rows, row_bytes));
    TRY(ensure(c, c->tr_stat, 4 * sizeof(unsigned long long)));
    unsigned long long* d_untiered = c->tr_stat.as<unsigned long long>() + 3;
    EventPair ev_all(c);
    if (!ev_all.a || !ev_all.b) return fail(QMCP_EHIP, "event creation failed");
    HIP_TRY(hipEventRecord(ev_all.a, st));

    // 1: keys, grouping, bounds
    const uint32_t passes = std::max(1u, (bit_width(n_pairs) + 7) / 8);  // keys go up to n_pairs
    std::vector<uint32_t> offs;
    const void* sorted = nullptr;
    uint32_t err = 0;
    HIP_TRY(hipMemsetAsync(d_untiered, 0, sizeof(unsigned long long), st));
    TRY(group_reads(
        c, n64, lengths, n_contigs, n_groups, passes,
        {{"k_radix_hist_rec(tiers)", "scan_radix_hist(tiers, 3 kernels)", "k_radix_scatter_rec(tiers)"}, "k_bc_bounds(tiers)"},
        [&] {
            KernelSpan sp(c, "k_st_keys(tiers)");
            qmcp::launch_st_keys(st, d_starts, d_ends, d_ids, d_tiers, n, c->bc_len.u32(), n_contigs, n_tiers,
                                   c->bc_key.u32(), c->bc_err.u32(), d_untiered);
        },
        d_mask, offs, &sorted, &err));
    if (err & 1u) return fail(QMCP_EINVAL, "a contig id is neither < n_contigs (%u) nor QMCP_NO_CONTIG", n_contigs);
    if (err & 4u) return fail(QMCP_EINVAL, "a tier id is neither < n_tiers (%u) nor QMCP_NO_TIER", n_tiers);
    if (err & 2u) return fail(QMCP_EREAD, "a read has start > end or end >= its contig's length");

    // 2: batches, none across a tier boundary
    std::vector<uint64_t> counts(n_pairs);
    for (uint32_t k = 0; k < n_pairs; ++k) counts[k] = offs[k + 1] - offs[k];
    const uint32_t n_placed = offs[n_pairs];
    std::vector<qmcp::TierBatch> batches;
    uint32_t bad_t = 0, bad_c = 0;
    const int prc = qmcp::plan_tier_batches(counts.data(), lengths, n_contigs, n_tiers, M, batches, &bad_t, &bad_c);
    if (prc == QMCP_ERANGE)
        return fail(QMCP_ERANGE,
                    "tier %u on contig %u alone exceeds one call's limits: %llu reads (at most 2^30), %u positions (at most "
                    "2^31 - 2)",
                    bad_t, bad_c, (unsigned long long)counts[(size_t)bad_t * n_contigs + bad_c], lengths[bad_c]);
    if (prc != QMCP_OK) return fail(prc, "the tiered plan refused its tables");
    size_t largest = 0;
    TRY(reserve_batch_buffers(c, batches, &largest));
    uint32_t last_tier = 0;  // the last tier that is solved: its kept reads are nobody's credit
    for (const qmcp::TierBatch& bt : batches)
        if (bt.n_reads != 0) last_tier = bt.stratum;
    size_t largest0 = 0;  // the largest batch of tier 0: its route is the stats'
    for (size_t b = 0; b < batches.size() && batches[b].stratum == 0; ++b)
        if (batches[b].n_reads > batches[largest0].n_reads) largest0 = b;

    qmcp_hip_stats sum;  // tier 0's solver calls
    std::memset(&sum, 0, sizeof(sum));
    sum.n_contigs = n_contigs;
    for (uint32_t k = 0; k < n_contigs; ++k) sum.total_length += lengths[k];
    std::vector<qmcp_hip_tier_row> rows(n_tiers);
    std::memset(rows.data(), 0, rows.size() * sizeof(qmcp_hip_tier_row));
    float ms_solves = 0.f;
    uint64_t n_listed = 0;  // entries of the kept list
    bool first0 = true;
    BatchView v;
    for (size_t b = 0; b < batches.size(); ++b) {
        const qmcp::TierBatch& bt = batches[b];
        if (bt.n_reads == 0) continue;  // (contigs the tier has no reads on keep nothing)
        const uint32_t t = bt.stratum;
        qmcp_hip_tier_row& row = rows[t];
        batch_view(sorted, offs.data() + (size_t)t * n_contigs + bt.first_contig, lengths, bt, v);
        TRY(gather_batch(c, v, d_starts, d_ends));
        qmcp_hip_stats one;  // this batch's
        std::memset(&one, 0, sizeof(one));
        if (t == 0) {  // 3
            PlainSolver plain(M);
            TRY(solve_scatter_batch(c, v, plain, d_mask, one, true, true));
            add_batch_stats(sum, one, first0, b == largest0);
            first0 = false;
            row.sweeps += 1u;
        } else {  // 4
            TierSolver later(M, (uint32_t)n_listed);
            TRY(solve_scatter_batch(c, v, later, d_mask, one, true, true));
            row.capped_positions += later.need.counters[0];
            row.demand += later.need.counters[1];
            row.asked_positions += later.need.counters[2];
            row.sweeps += later.swept ? 1u : 0u;
        }
        row.n_kept += one.n_kept;
        row.ms_stage += one.ms_total;
        ms_solves += one.ms_total;
        // 5: the batch's kept reads join the list
        if (t < last_tier && one.n_kept != 0) {
            const uint32_t words = (v.nb + 63u) / 64u;
            TRY(ensure(c, c->tr_words, ((size_t)words + 2) * sizeof(uint32_t)));
            TRY(ensure(c, c->tr_spine, scan_spine_bytes(words + 1, 1)));
            const size_t floor_entries = std::max<size_t>(4096, n_placed / 32);
            TRY(reserve_kept_list(c, std::max<size_t>(floor_entries, n_listed + one.n_kept), (size_t)n_listed));
            KernelSpan sp(c, "k_tier_keep_list(popcounts, scan, compaction)");
            queue_mask_ranks(st, c->bc_mask.u64(), words, c->tr_words, c->tr_spine);
            qmcp::launch_tier_keep_list(st, c->bc_starts.u32(), c->bc_ends.u32(), v.records, c->bc_mask.u64(),
                                        c->tr_words.u32(), v.nb, t * n_contigs,
                                        c->tr_list.as<unsigned char>() + (size_t)n_listed * qmcp::kTierKeptBytes,
                                        (uint32_t)one.n_kept);
            n_listed += one.n_kept;
        }
        HIP_TRY(hipGetLastError());
    }

    sum.n_reads = offs[n_contigs];  // tier 0's placed reads (they are its solver calls' reads, unless M == 0 made none)

    // 6: the rows' bases (the reads and the kept reads of a tier are known from the grouping and the solves: a call that
    // asks for no rows runs no pass over the records), the reads without a tier
    std::vector<uint64_t> tally((size_t)n_tiers * 4, 0);
    unsigned long long untiered = 0;
    if (rows_out) {
        HIP_TRY(hipMemsetAsync(c->tr_rows.p, 0, row_bytes, st));
        {
            KernelSpan sp(c, "k_st_tally(tiers)");
            qmcp::launch_st_tally(st, sorted, n_placed, n_contigs, d_starts, d_ends, d_mask, c->tr_rows.u64());
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(tally.data(), c->tr_rows.p, row_bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(&untiered, d_untiered, sizeof(untiered), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev_all.b, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    qmcp_hip_tiers_stats ts;
    std::memset(&ts, 0, sizeof(ts));
    ts.n_tiers = n_tiers;
    ts.reads_untiered = untiered;
    ts.ms_tiers = std::max(0.f, elapsed(ev_all.a, ev_all.b) - ms_solves);
    for (uint32_t t = 0; t < n_tiers; ++t) {
        rows[t].n_reads = offs[(size_t)(t + 1) * n_contigs] - offs[(size_t)t * n_contigs];
        if (rows_out && (tally[4 * (size_t)t] != rows[t].n_reads || tally[4 * (size_t)t + 1] != rows[t].n_kept))
            return fail(QMCP_EHIP, "tier %u: the rows' pass counted other reads than the grouping and the solves", t);
        rows[t].bases_in = tally[4 * (size_t)t + 2];
        rows[t].bases_kept = tally[4 * (size_t)t + 3];
        ts.tiers_used += rows[t].n_kept != 0 ? 1u : 0u;
    }
    if (rows_out) std::memcpy(rows_out, rows.data(), rows.size() * sizeof(qmcp_hip_tier_row));
    if (stats) *stats = sum;
    if (tstats) *tstats = ts;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_tiers_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                              const uint32_t* tiers, uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                              uint32_t max_coverage, uint32_t n_tiers, uint64_t* keep_mask_out, qmcp_hip_tier_row* rows_out,
                              qmcp_hip_stats* stats, qmcp_hip_tiers_stats* tstats) {
    TRY(check_tiers_entry(contig_lengths, n_contigs, tiers, n_tiers, max_coverage, n_reads));
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    TRY(ensure(c, c->tr_tiers, nb));
    TRY(ensure(c, c->mask, words * sizeof(uint64_t)));
    c->mask_reads = 0;
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->tr_tiers.p, tiers, nb, hipMemcpyHostToDevice, c->stream));
    }
    // the rows land in a buffer of the call's own: a failure leaves rows_out as it was
    std::vector<qmcp_hip_tier_row> rows(rows_out ? n_tiers : 0);
    TRY(solve_tiers_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), c->tr_tiers.u32(), n_reads,
                              contig_lengths, n_contigs, max_coverage, n_tiers, c->mask.u64(),
                              rows_out ? rows.data() : nullptr, stats, tstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (rows_out) std::memcpy(rows_out, rows.data(), rows.size() * sizeof(qmcp_hip_tier_row));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_tiers_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                const uint32_t* d_contig_ids, const uint32_t* d_tiers, uint64_t n_reads,
                                const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage, uint32_t n_tiers,
                                uint64_t* d_keep_mask_out, qmcp_hip_tier_row* rows_out, void* hip_stream,
                                qmcp_hip_stats* stats, qmcp_hip_tiers_stats* tstats) {
    TRY(check_tiers_entry(contig_lengths, n_contigs, d_tiers, n_tiers, max_coverage, n_reads));
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(order_after(c, hip_stream));
    return solve_tiers_on_device(c, d_starts, d_ends, d_contig_ids, d_tiers, n_reads, contig_lengths, n_contigs, max_coverage,
                                 n_tiers, d_keep_mask_out, rows_out, stats, tstats);
}

}  // extern "C"
