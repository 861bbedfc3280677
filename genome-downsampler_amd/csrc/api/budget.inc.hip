// budget.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_budget_host / _device: the deepest coverage M* in 0 .. top whose by-contig solve keeps at most
// budget_reads reads (after pair completion under QMCP_BUDGET_WHOLE_PAIRS), and that solve's mask.
//   1. group_by_contig (api/by_contig.inc.hip): once per call
//   2. depth_curve (api/cap_search.inc.hip) with k_budget_tally over every position: the curve, the largest depth and the
//      sum of the depths
//   3. budget_plan.h starts from the curve and the reads' largest span; search_cap (api/cap_search.inc.hip) runs its
//      probes.  A probe counts the reads its solve kept: the solve's own n_kept, or under the flag k_budget_finish's word
//      after it completed the pairs in the probe's mask
// Buffers: bg_acc (CapAcc: BudgetWord words | curve | histogram), bg_mask (the probes' second mask).
namespace {

// the checks both entries make before anything is copied or launched
int check_budget_call(uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                      uint32_t flags, const uint64_t* curve_out, uint32_t curve_capacity) {
    if (flags & ~QMCP_BUDGET_WHOLE_PAIRS) return fail(QMCP_EINVAL, "unknown flag bits 0x%x", flags & ~QMCP_BUDGET_WHOLE_PAIRS);
    if ((flags & QMCP_BUDGET_WHOLE_PAIRS) && (n_reads & 1ull))
        return fail(QMCP_EINVAL, "n_reads %llu is odd: reads (2q, 2q + 1) are pair q", (unsigned long long)n_reads);
    if (!contig_lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (max_coverage == 0) return fail(QMCP_EINVAL, "max_coverage == 0: the search needs an upper end of at least 1");
    if (max_coverage >= (1u << 31)) return fail(QMCP_ERANGE, "max_coverage %u is 2^31 or more", max_coverage);
    if (!curve_out && curve_capacity) return fail(QMCP_EINVAL, "curve_capacity %u without curve_out", curve_capacity);
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    return QMCP_OK;
}

int solve_budget_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                           uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, uint32_t max_coverage, uint64_t budget,
                           uint32_t flags, uint64_t* curve_out, uint32_t curve_capacity, uint64_t* d_mask,
                           qmcp_hip_stats* stats, qmcp_hip_budget_stats* bstats) {
    qmcp_hip_budget_stats bs;
    std::memset(&bs, 0, sizeof(bs));
    bs.budget = budget;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (bstats) *bstats = bs;
    const size_t words = (size_t)((n64 + 63) / 64);
    const bool whole_pairs = (flags & QMCP_BUDGET_WHOLE_PAIRS) != 0;
    hipStream_t st = c->stream;
    CapAcc a;
    TRY(reserve_cap_acc(c, max_coverage, words, 0, a));

    // 1: the grouping (the mask it clears is the budget's own: a refused call leaves d_mask alone)
    GroupedReads g;
    TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, c->bg_mask.u64(), g));
    const uint64_t placed = g.offs[n_contigs];

    // 2: the depth histogram over every batch, the curve
    ProbeSolve probe{g};
    TimedLaunches timed{c};
    DepthCurve d;
    TRY(depth_curve(c, probe, a, max_coverage, timed,
                    [&](size_t, const BatchView&, uint32_t ltot) { tally_every_position(c, a, ltot); }, d));
    bs.ms_budget = d.ms;
    bs.reads_placed = placed;
    bs.max_depth = d.max_depth;
    bs.total_bases = d.total_bases;
    bs.top = d.top;
    bs.curve_entries = d.copy_out(curve_out, curve_capacity);

    // 3: the probes
    qmcp::BudgetPlan plan;
    plan.start(d.curve, a.H, d.top, d.span_max, d.total_bases, placed, budget);
    auto kept_reads = [&](uint64_t* pm, const qmcp_hip_stats& sum, uint64_t* count) -> int {
        *count = sum.n_kept;
        if (!whole_pairs) return QMCP_OK;
        unsigned long long kept = 0;
        HIP_TRY(hipMemsetAsync(a.acc + qmcp::kBudgetKept, 0, sizeof(unsigned long long), st));
        TRY(timed.run([&] {
            KernelSpan sp(c, "k_budget_finish");
            qmcp::launch_budget_finish(st, d_ids, n64, pm, a.acc);
        }));
        HIP_TRY(hipMemcpyAsync(&kept, a.acc + qmcp::kBudgetKept, sizeof(kept), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        bs.ms_budget += timed.total();
        *count = kept;
        return QMCP_OK;
    };
    TRY(search_cap(c, plan, d_mask, c->bg_mask.u64(), words, probe, kept_reads, stats, &bs.ms_solves));
    bs.coverage = plan.lo;
    bs.n_kept = plan.count_lo;
    bs.probes = plan.probes;
    if (plan.hi <= bs.top) {
        bs.kept_above = plan.count_hi;
        bs.bound_above = plan.bound_hi;
    }
    bs.saturated = bs.n_kept == placed ? 1u : 0u;
    if (bstats) *bstats = bs;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_budget_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                               uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                               uint64_t budget_reads, uint32_t flags, uint64_t* curve_out, uint32_t curve_capacity,
                               uint64_t* keep_mask_out, qmcp_hip_stats* stats, qmcp_hip_budget_stats* bstats) {
    // (the refusals need no device: they come before the context is looked at)
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(check_budget_call(n_reads, contig_lengths, n_contigs, max_coverage, flags, curve_out, curve_capacity));
    TRY(use_device(c));
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
    TRY(solve_budget_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), n_reads, contig_lengths,
        n_contigs, max_coverage, budget_reads, flags, curve_out, curve_capacity, c->mask.u64(), stats, bstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_budget_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                 const uint32_t* d_contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                 uint32_t n_contigs, uint32_t max_coverage, uint64_t budget_reads, uint32_t flags,
                                 uint64_t* curve_out, uint32_t curve_capacity, uint64_t* d_keep_mask_out, void* hip_stream,
                                 qmcp_hip_stats* stats, qmcp_hip_budget_stats* bstats) {
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(check_budget_call(n_reads, contig_lengths, n_contigs, max_coverage, flags, curve_out, curve_capacity));
    TRY(use_device(c));
    TRY(order_after(c, hip_stream));
    return solve_budget_on_device(c, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, n_contigs, max_coverage,
                                  budget_reads, flags, curve_out, curve_capacity, d_keep_mask_out, stats, bstats);
}

}  // extern "C"
