// by_contig.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_by_contig_host / _device: reads of several contigs in any order, one contig id per read.  The pieces, which
// every entry of the by-contig family (ladder, profile, ceiling, proportional, budget, pairs, templates, replicates; stratified with keys
// and a plan of its own) puts together in a flow of its own:
//   group_reads      a key kernel checks every read and writes its sort key; the stable record radix
//                    (api/radix_passes.inc.hip) groups {key, read index} by key into the context's own record buffers (the
//                    solves never touch them); k_bc_bounds turns the sorted keys into each group's run; the bounds and the
//                    validation word come back to the host
//   group_by_contig  the grouping as a value (GroupedReads), once per call: group_reads around k_bc_keys (key: the contig
//                    id; n_contigs for unplaced reads), by_contig_plan.h's batches within one call's limits, the gathered
//                    columns and the batch mask sized for the largest batch
//   BatchView        one batch: its records, contigs' lengths and read offsets; on request the 32-bit offset tables
//   run_batches      per batch with reads: gather_batch (its columns in grouped order), solve_scatter_batch (a BatchSolver
//                    -- PlainSolver is the ordinary multi-contig solve at M -- fills the batch mask, which is ORed back
//                    into input order; the batch's stats join the call's), then the solver's after_batch
// The by-contig call itself is group_by_contig, run_batches with a PlainSolver, and the final wait.
// The entries that solve one grouping at several coverages (budget, mean-depth, thresholds) put these together once more,
// in api/cap_search.inc.hip: the probe solve, and for the first two the depth-curve stage and the search loop.
namespace {

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
    TRY(ensure(c, c->bc_spine, scan_spine_bytes(256u * n_tiles)));
    if (words) HIP_TRY(hipMemsetAsync(d_mask, 0, words * sizeof(uint64_t), st));
    HIP_TRY(hipMemsetAsync(c->bc_err.p, 0, sizeof(uint32_t), st));
    HIP_TRY(hipMemcpyAsync(c->bc_len.p, lengths, (size_t)n_contigs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    queue_keys();
    int k = 0;
    if (n)
        TRY(radix_sort_records(c, st, c->bc_key.u32(), n, passes, c->bc_hist.u32(),
                               c->bc_spine.u32(), c->bc_rec, nm.radix, &k));
    *sorted = c->bc_rec[k].p;
    {
        KernelSpan sp(c, nm.bounds);
        qmcp::launch_bc_bounds(st, *sorted, n, n_groups, c->bc_offs.u32());
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

// One batch of grouped reads as its consumers see it: nb > 0 records, contigs first_contig .. + n_contigs.
struct BatchView {
    const void* records = nullptr;  // the batch's {key, index} records
    uint32_t nb = 0, first_contig = 0, n_contigs = 0;
    uint64_t positions = 0;
    const uint32_t* lengths = nullptr;     // of the batch's contigs
    std::vector<uint64_t> roff;            // contig_read_offsets, n_contigs + 1
    std::vector<uint32_t> offs32, poff32;  // after tables32(): roff and the contigs' position offsets in 32 bits
    void tables32() {  // (a batch holds at most 2^30 reads and 2^31 - 2 positions)
        offs32.assign(roff.begin(), roff.end());
        poff32.assign(roff.size(), 0);
        for (uint32_t k = 0; k < n_contigs; ++k) poff32[k + 1] = poff32[k] + lengths[k];
    }
};

// goffs points at the offsets of the batch's first group in the grouping's table
template <typename Batch>
void batch_view(const void* sorted, const uint32_t* goffs, const uint32_t* lengths, const Batch& bt, BatchView& v) {
    v.records = (const uint32_t*)sorted + 2 * bt.first_read;
    v.nb = (uint32_t)bt.n_reads;
    v.first_contig = bt.first_contig;
    v.n_contigs = bt.n_contigs;
    v.positions = bt.positions;
    v.lengths = lengths + bt.first_contig;
    v.roff.resize((size_t)bt.n_contigs + 1);
    for (uint32_t k = 0; k <= bt.n_contigs; ++k) v.roff[k] = goffs[k] - goffs[0];
}

// What one grouping by contig produced, and what every consumer of it needs.
struct GroupedReads {
    const uint32_t *d_starts = nullptr, *d_ends = nullptr, *d_ids = nullptr;  // the call's device columns, input order
    const uint32_t* lengths = nullptr;                                        // host
    uint32_t n_contigs = 0;
    uint64_t n64 = 0, total_length = 0;
    const void* sorted = nullptr;  // the grouped {key, index} records
    std::vector<uint32_t> offs;    // each contig's run in them, then the unplaced reads'
    std::vector<qmcp::ContigBatch> batches;
    std::vector<size_t> live;  // the batches with reads
    size_t largest = 0;        // the batch with the most reads: its route is the call's
    void view(size_t b, BatchView& v) const {
        batch_view(sorted, offs.data() + batches[b].first_contig, lengths, batches[b], v);
    }
};

// Steps 1-4 of a by-contig call up to its first batch: the size checks, the grouping (mask_to_clear is cleared before the
// reads are validated), the device-found refusals, the batches, the buffers of the largest one.
int group_by_contig(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids, uint64_t n64,
                    const uint32_t* lengths, uint32_t n_contigs, uint64_t* mask_to_clear, GroupedReads& g) {
    if (!lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    if (n64 > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n64);
    g = GroupedReads{d_starts, d_ends, d_ids, lengths, n_contigs, n64};
    const uint32_t passes = std::max(1u, (bit_width(n_contigs) + 7) / 8);  // keys go up to n_contigs
    uint32_t err = 0;
    TRY(group_reads(
        c, n64, lengths, n_contigs, n_contigs + 1 /* the contigs, then the unplaced reads */, passes,
        {{"k_radix_hist_rec(by contig)", "scan_radix_hist(by contig, 3 kernels)", "k_radix_scatter_rec(by contig)"},
         "k_bc_bounds"},
        [&] {
            KernelSpan sp(c, "k_bc_keys");
            qmcp::launch_bc_keys(c->stream, d_starts, d_ends, d_ids, (uint32_t)n64, c->bc_len.u32(), n_contigs,
                                 c->bc_key.u32(), c->bc_err.u32());
        },
        mask_to_clear, g.offs, &g.sorted, &err));
    if (err & 1u) return fail(QMCP_EINVAL, "a contig id is neither < n_contigs (%u) nor QMCP_NO_CONTIG", n_contigs);
    if (err & 2u) return fail(QMCP_EREAD, "a read has start > end or end >= its contig's length");
    std::vector<uint64_t> counts(n_contigs);
    for (uint32_t k = 0; k < n_contigs; ++k) counts[k] = g.offs[k + 1] - g.offs[k];
    uint32_t bad = 0;
    if (qmcp::plan_contig_batches(counts.data(), lengths, n_contigs, g.batches, &bad) != QMCP_OK)
        return fail(QMCP_ERANGE,
                    "contig %u alone exceeds one call's limits: %llu reads (at most 2^30), %u positions (at most 2^31 - 2)",
                    bad, (unsigned long long)counts[bad], lengths[bad]);
    TRY(reserve_batch_buffers(c, g.batches, &g.largest));
    for (size_t b = 0; b < g.batches.size(); ++b) {
        g.total_length += g.batches[b].positions;
        if (g.batches[b].n_reads != 0) g.live.push_back(b);
    }
    return QMCP_OK;
}

// What solves one gathered batch: its columns are in bc_starts / bc_ends in grouped order, its mask goes to bc_mask.
struct BatchSolver {
    virtual ~BatchSolver() {}
    virtual int solve(qmcp_hip_ctx* c, BatchView& v, qmcp_hip_stats* bs) = 0;
    // once the batch's mask is in input order and its stats are added (the ladder's further levels)
    virtual int after_batch(qmcp_hip_ctx*, BatchView&) { return QMCP_OK; }
};

// the ordinary multi-contig solve at M
struct PlainSolver : BatchSolver {
    uint32_t M;
    explicit PlainSolver(uint32_t m) : M(m) {}
    int solve(qmcp_hip_ctx* c, BatchView& v, qmcp_hip_stats* bs) override {
        return solve_on_device(c, c->bc_starts.u32(), c->bc_ends.u32(), v.roff.data(), v.lengths,
                               v.n_contigs, v.nb, M, c->bc_mask.u64(), bs);
    }
};

// the batch's columns, in grouped order, into bc_starts / bc_ends
int gather_batch(qmcp_hip_ctx* c, const BatchView& v, const uint32_t* d_starts, const uint32_t* d_ends) {
    {
        KernelSpan sp(c, "k_bc_gather");
        qmcp::launch_bc_gather(c->stream, v.records, v.nb, d_starts, d_ends, c->bc_starts.u32(), c->bc_ends.u32());
    }
    HIP_TRY(hipGetLastError());
    return QMCP_OK;
}

// a gathered batch solved, its mask ORed back into input order, its stats added to `sum`
int solve_scatter_batch(qmcp_hip_ctx* c, BatchView& v, BatchSolver& solver, uint64_t* d_mask, qmcp_hip_stats& sum, bool first,
                        bool largest) {
    qmcp_hip_stats bs;
    std::memset(&bs, 0, sizeof(bs));
    TRY(solver.solve(c, v, &bs));
    {
        KernelSpan sp(c, "k_bc_scatter_mask");
        qmcp::launch_bc_scatter_mask(c->stream, c->bc_mask.u64(), v.records, v.nb, d_mask);
    }
    HIP_TRY(hipGetLastError());
    add_batch_stats(sum, bs, first, largest);
    return QMCP_OK;
}

// a call's stats before its first batch: every contig counts, those of batches without reads included
void start_sum(const GroupedReads& g, qmcp_hip_stats& sum) {
    std::memset(&sum, 0, sizeof(sum));
    sum.n_contigs = g.n_contigs;
    sum.total_length = g.total_length;
}

// The batch loop: every batch with reads gathered, solved by `solver`, scattered into d_mask (cleared by the grouping:
// the scatter ORs); `sum` takes the call's stats.  (Batches without reads solve nothing: empty contigs keep nothing.)
int run_batches(qmcp_hip_ctx* c, const GroupedReads& g, BatchSolver& solver, uint64_t* d_mask, qmcp_hip_stats& sum) {
    start_sum(g, sum);
    BatchView v;
    for (size_t b : g.live) {
        g.view(b, v);
        TRY(gather_batch(c, v, g.d_starts, g.d_ends));
        TRY(solve_scatter_batch(c, v, solver, d_mask, sum, b == g.live.front(), b == g.largest));
        TRY(solver.after_batch(c, v));
    }
    return QMCP_OK;
}

int solve_by_contig_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                              uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, uint32_t M, uint64_t* d_mask,
                              qmcp_hip_stats* stats) {
    GroupedReads g;
    TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, d_mask, g));
    PlainSolver plain(M);
    qmcp_hip_stats sum;
    TRY(run_batches(c, g, plain, d_mask, sum));
    HIP_TRY(hipStreamSynchronize(c->stream));
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
    TRY(solve_by_contig_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), n_reads, contig_lengths,
        n_contigs, max_coverage, c->mask.u64(), stats));
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
