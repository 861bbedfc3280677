// stratified.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_stratified_host / _device: reads of several contigs AND several strata (strand, read group, sample)
// in any order, one coverage cap per stratum.  The mask is the OR over the strata of the by-contig solve of that
// stratum's reads alone at its cap.
//   1, 2. group_reads (api/by_contig.inc.hip) around k_st_keys, which checks every read against its contig, checks its
//      stratum id, and writes the stratum-major sort key stratum * n_contigs + contig (n_strata * n_contigs for a read
//      without contig or stratum): one radix pass per 8 bits of n_strata * n_contigs, each (stratum, contig)'s run
//   3. stratified_plan.h cuts every stratum that has a cap and reads into batches (by_contig_plan.h's packing, one
//      stratum at a time); per batch gather_batch and solve_scatter_batch with a PlainSolver at the stratum's cap
//   4. k_st_tally reduces the grouped records against the final mask into one row per stratum; n_strata x 32 bytes
//      come back
// Buffers: the grouping and the batches live in the by-contig solve's buffers (bc_*), which nothing else uses while
// this call runs; the strata column of the host entry (st_strata) and the rows (st_rows) are this file's own.
namespace {

int check_stratified_call(const uint32_t* lengths, uint32_t n_contigs, const uint32_t* caps, uint32_t n_strata,
                          uint64_t n64) {
    if (!lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (!caps) return fail(QMCP_EINVAL, "max_coverages missing");
    if (n_strata == 0) return fail(QMCP_EINVAL, "n_strata == 0: a stratified call needs at least one stratum");
    if (n_strata > qmcp::kMaxStrata)
        return fail(QMCP_ERANGE, "n_strata %u exceeds %u per stratified call", n_strata, qmcp::kMaxStrata);
    if ((uint64_t)n_strata * n_contigs > qmcp::kMaxStratumGroups)
        return fail(QMCP_ERANGE, "n_strata %u x n_contigs %u = %llu exceeds 2^24 (stratum, contig) groups per call",
                    n_strata, n_contigs, (unsigned long long)((uint64_t)n_strata * n_contigs));
    if (n64 > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n64);
    return QMCP_OK;
}

int solve_stratified_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                               const uint32_t* d_strata, uint64_t n64, const uint32_t* lengths, uint32_t n_contigs,
                               const uint32_t* caps, uint32_t n_strata, uint64_t* d_mask, qmcp_hip_stratum_row* rows_out,
                               qmcp_hip_stats* stats) {
    const uint32_t n = (uint32_t)n64;
    const uint32_t n_pairs = n_strata * n_contigs;  // the (stratum, contig) groups, <= 2^24
    const uint32_t n_groups = n_pairs + 1;          // ... then the reads without contig or stratum
    hipStream_t st = c->stream;
    TRY(ensure(c, c->st_rows, (size_t)n_strata * sizeof(qmcp_hip_stratum_row)));

    // 1, 2: keys, grouping, bounds
    const uint32_t passes = std::max(1u, (bit_width(n_pairs) + 7) / 8);  // keys go up to n_pairs
    std::vector<uint32_t> offs;
    const void* sorted = nullptr;
    uint32_t err = 0;
    TRY(group_reads(
        c, n64, lengths, n_contigs, n_groups, passes,
        {{"k_radix_hist_rec(stratified)", "scan_radix_hist(stratified, 3 kernels)", "k_radix_scatter_rec(stratified)"},
         "k_bc_bounds(stratified)"},
        [&] {
            KernelSpan sp(c, "k_st_keys");
            qmcp::launch_st_keys(st, d_starts, d_ends, d_ids, d_strata, n, c->bc_len.u32(), n_contigs, n_strata,
                                 c->bc_key.u32(), c->bc_err.u32());
        },
        d_mask, offs, &sorted, &err));
    if (err & 1u) return fail(QMCP_EINVAL, "a contig id is neither < n_contigs (%u) nor QMCP_NO_CONTIG", n_contigs);
    if (err & 4u) return fail(QMCP_EINVAL, "a stratum id is neither < n_strata (%u) nor QMCP_NO_STRATUM", n_strata);
    if (err & 2u) return fail(QMCP_EREAD, "a read has start > end or end >= its contig's length");

    // 3: batches, none across a stratum boundary
    std::vector<uint64_t> counts(n_pairs);
    for (uint32_t k = 0; k < n_pairs; ++k) counts[k] = offs[k + 1] - offs[k];
    const uint32_t n_placed = offs[n_pairs];
    std::vector<qmcp::StratumBatch> batches;
    uint32_t bad_s = 0, bad_c = 0;
    const int prc = qmcp::plan_stratum_batches(counts.data(), lengths, n_contigs, caps, n_strata, batches, &bad_s, &bad_c);
    if (prc == QMCP_ERANGE)
        return fail(QMCP_ERANGE,
                    "stratum %u on contig %u alone exceeds one call's limits: %llu reads (at most 2^30), %u positions (at "
                    "most 2^31 - 2)",
                    bad_s, bad_c, (unsigned long long)counts[(size_t)bad_s * n_contigs + bad_c], lengths[bad_c]);
    if (prc != QMCP_OK) return fail(prc, "the stratified plan refused its tables");
    size_t largest = 0;
    TRY(reserve_batch_buffers(c, batches, &largest));
    qmcp_hip_stats sum;
    std::memset(&sum, 0, sizeof(sum));
    bool first = true;
    BatchView v;
    for (size_t b = 0; b < batches.size(); ++b) {
        const qmcp::StratumBatch& bt = batches[b];
        sum.n_contigs += bt.n_contigs;
        sum.total_length += bt.positions;
        if (bt.n_reads == 0) continue;  // (contigs the stratum has no reads on keep nothing)
        batch_view(sorted, offs.data() + (size_t)bt.stratum * n_contigs + bt.first_contig, lengths, bt, v);
        PlainSolver plain(bt.M);
        TRY(gather_batch(c, v, d_starts, d_ends));
        TRY(solve_scatter_batch(c, v, plain, d_mask, sum, first, b == largest));
        first = false;
    }
    sum.n_reads = n_placed;  // (strata without a cap are not solved, yet their reads are part of the call)

    // 4: the rows
    if (rows_out) {
        HIP_TRY(hipMemsetAsync(c->st_rows.p, 0, (size_t)n_strata * sizeof(qmcp_hip_stratum_row), st));
        {
            KernelSpan sp(c, "k_st_tally");
            qmcp::launch_st_tally(st, sorted, n_placed, n_contigs, d_starts, d_ends, d_mask, c->st_rows.u64());
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rows_out, c->st_rows.p, (size_t)n_strata * sizeof(qmcp_hip_stratum_row),
                               hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    if (stats) *stats = sum;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_stratified_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends,
                                   const uint32_t* contig_ids, const uint32_t* strata, uint64_t n_reads,
                                   const uint32_t* contig_lengths, uint32_t n_contigs, const uint32_t* max_coverages,
                                   uint32_t n_strata, uint64_t* keep_mask_out, qmcp_hip_stratum_row* rows_out,
                                   qmcp_hip_stats* stats) {
    TRY(check_stratified_call(contig_lengths, n_contigs, max_coverages, n_strata, n_reads));
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !strata || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    TRY(ensure(c, c->st_strata, nb));
    TRY(ensure(c, c->mask, words * sizeof(uint64_t)));
    c->mask_reads = 0;
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->st_strata.p, strata, nb, hipMemcpyHostToDevice, c->stream));
    }
    // the rows land in a buffer of the call's own: a failure leaves rows_out as it was
    std::vector<qmcp_hip_stratum_row> rows(rows_out ? n_strata : 0);
    TRY(solve_stratified_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), c->st_strata.u32(),
        n_reads, contig_lengths, n_contigs, max_coverages, n_strata, c->mask.u64(), rows_out ? rows.data() : nullptr,
        stats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (rows_out) std::memcpy(rows_out, rows.data(), rows.size() * sizeof(qmcp_hip_stratum_row));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_stratified_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                     const uint32_t* d_contig_ids, const uint32_t* d_strata, uint64_t n_reads,
                                     const uint32_t* contig_lengths, uint32_t n_contigs, const uint32_t* max_coverages,
                                     uint32_t n_strata, uint64_t* d_keep_mask_out, qmcp_hip_stratum_row* rows_out,
                                     void* hip_stream, qmcp_hip_stats* stats) {
    TRY(check_stratified_call(contig_lengths, n_contigs, max_coverages, n_strata, n_reads));
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_strata || !d_keep_mask_out))
        return fail(QMCP_EINVAL, "null buffer");
    TRY(order_after(c, hip_stream));
    std::vector<qmcp_hip_stratum_row> rows(rows_out ? n_strata : 0);
    TRY(solve_stratified_on_device(c, d_starts, d_ends, d_contig_ids, d_strata, n_reads, contig_lengths, n_contigs,
                                   max_coverages, n_strata, d_keep_mask_out, rows_out ? rows.data() : nullptr, stats));
    if (rows_out) std::memcpy(rows_out, rows.data(), rows.size() * sizeof(qmcp_hip_stratum_row));
    return QMCP_OK;
}

}  // extern "C"
