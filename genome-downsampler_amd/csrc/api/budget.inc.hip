// budget.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_budget_host / _device: the deepest coverage M* in 0 .. top whose by-contig solve keeps at most
// budget_reads reads (after pair completion under QMCP_BUDGET_WHOLE_PAIRS), and that solve's mask.
//   1. group_by_contig (api/by_contig.inc.hip): once per call
//   2. per batch with reads, before the first probe: its columns gathered, its per-position depth built by the launches
//      of coverage_common (k_prepare's start counts, the two scans, the end counts, k_coverage), k_budget_tally over it
//   3. k_budget_curve; the curve, the largest depth and the sum of the depths come back in one copy
//   4. budget_plan.h picks the probes; a probe is run_batches with a PlainSolver at M into a cleared input-order mask,
//      then k_budget_finish under the flag.  Two masks: the one a probe scatters into and the one of the best
//      feasible probe; they swap roles when a probe is feasible, so nothing is solved twice
// A call of one batch with reads gathers its columns once, in step 2, for all probes: its probes are solve_scatter_batch.
// Buffers: bg_acc (BudgetWord words | curve | histogram), bg_mask; step 2 passes through the solve's own arena (cstart,
// boff, ecnt, eoff, cov) before the first solve and holds nothing of it afterwards.
namespace {

// the per-position depth of a gathered batch into c->cov (coverage_common's launches, on device columns); *span_max takes
// the batch's largest span
int budget_batch_depth(qmcp_hip_ctx* c, const uint32_t* bs_starts, const uint32_t* bs_ends, const uint64_t* roff,
                       const uint32_t* lengths, uint32_t n_contigs, uint64_t nb, uint32_t* ltot_out, uint32_t* span_max) {
    Problem pr;
    TRY(check_problem(roff, lengths, n_contigs, nb, pr));
    const uint32_t n = (uint32_t)pr.n, ltot = (uint32_t)pr.ltot;
    *ltot_out = ltot;
    if (ltot == 0 || n == 0) return QMCP_OK;
    TRY(upload_tables(c, roff, pr));
    uint32_t hs[3];
    TRY(run_prepare(c, bs_starts, bs_ends, pr, nullptr, true, true, false, 0, nullptr, hs));
    *span_max = std::max(*span_max, hs[1]);
    TRY(scan_counts(c, c->cstart, c->boff, ltot));
    TRY(ensure(c, c->ecnt, ((size_t)ltot + 1) * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(c->ecnt.p, 0, ((size_t)ltot + 1) * sizeof(uint32_t), c->stream));
    qmcp::launch_general_keys(c->stream, false, c->vals[1].u32(), bs_starts, bs_ends, n, 0, hs[1], nullptr,
                              nullptr, c->ecnt.u32(), ltot + 1);
    HIP_TRY(hipGetLastError());
    TRY(scan_counts(c, c->ecnt, c->eoff, ltot));
    TRY(ensure(c, c->cov, (size_t)ltot * sizeof(uint32_t)));
    qmcp::launch_coverage(c->stream, c->boff.u32(), c->eoff.u32(), ltot, c->cov.u32());
    HIP_TRY(hipGetLastError());
    return QMCP_OK;
}

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
    const uint32_t H = std::min(max_coverage, (uint32_t)QMCP_BUDGET_CURVE_MAX) + 1u;
    const size_t acc_words = (size_t)qmcp::kBudgetWords + 2 * (size_t)H;
    TRY(ensure(c, c->bg_mask, words * sizeof(uint64_t)));
    TRY(ensure(c, c->bg_acc, acc_words * sizeof(unsigned long long)));
    unsigned long long* d_acc = c->bg_acc.as<unsigned long long>();
    unsigned long long* d_curve = d_acc + qmcp::kBudgetWords;
    unsigned long long* d_hist = d_curve + H;
    HIP_TRY(hipMemsetAsync(d_acc, 0, acc_words * sizeof(unsigned long long), st));

    // 1: the grouping (the mask it clears is the budget's own: a refused call leaves d_mask alone)
    GroupedReads g;
    TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, c->bg_mask.u64(), g));
    const uint64_t placed = g.offs[n_contigs];

    // 2-3: the depth histogram over every batch, the curve
    std::vector<std::unique_ptr<EventPair>> evs;  // one per k_budget_tally, one for k_budget_curve
    auto bracket = [&]() -> EventPair* {
        evs.emplace_back(new EventPair(c));
        return evs.back()->a && evs.back()->b ? evs.back().get() : nullptr;
    };
    uint32_t span_max = 0;
    BatchView v;
    for (size_t b : g.live) {  // (no read: no depth)
        g.view(b, v);
        TRY(gather_batch(c, v, d_starts, d_ends));
        uint32_t ltot = 0;
        TRY(budget_batch_depth(c, c->bc_starts.u32(), c->bc_ends.u32(), v.roff.data(), v.lengths,
                               v.n_contigs, v.nb, &ltot, &span_max));
        EventPair* ev = bracket();
        if (!ev) return fail(QMCP_EHIP, "event creation failed");
        HIP_TRY(hipEventRecord(ev->a, st));
        {
            KernelSpan sp(c, "k_budget_tally");
            qmcp::launch_budget_tally(st, c->cov.u32(), ltot, H, d_acc, d_hist);
        }
        HIP_TRY(hipEventRecord(ev->b, st));
        HIP_TRY(hipGetLastError());
    }
    {
        EventPair* ev = bracket();
        if (!ev) return fail(QMCP_EHIP, "event creation failed");
        HIP_TRY(hipEventRecord(ev->a, st));
        {
            KernelSpan sp(c, "k_budget_curve");
            qmcp::launch_budget_curve(st, d_hist, H, d_curve);
        }
        HIP_TRY(hipEventRecord(ev->b, st));
        HIP_TRY(hipGetLastError());
    }
    std::vector<unsigned long long> back((size_t)qmcp::kBudgetWords + H);
    HIP_TRY(hipMemcpyAsync(back.data(), d_acc, back.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (auto& ev : evs) bs.ms_budget += elapsed(ev->a, ev->b);
    evs.clear();
    const uint64_t* curve = (const uint64_t*)(back.data() + qmcp::kBudgetWords);
    bs.reads_placed = placed;
    bs.max_depth = (uint32_t)back[qmcp::kBudgetMaxDepth];
    bs.total_bases = back[qmcp::kBudgetTotalBases];
    bs.top = std::min(max_coverage, bs.max_depth);
    if (curve_out && curve_capacity) {
        bs.curve_entries = std::min(std::min(bs.top, (uint32_t)QMCP_BUDGET_CURVE_MAX), curve_capacity - 1u) + 1u;
        for (uint32_t m = 0; m < bs.curve_entries; ++m) curve_out[m] = curve[m];
    }

    // 4: the probes
    qmcp::BudgetPlan plan;
    plan.start(curve, H, bs.top, span_max, bs.total_bases, placed, budget);
    uint64_t* masks[2] = {d_mask, c->bg_mask.u64()};
    int best = -1, scratch = 0;
    qmcp_hip_stats best_stats;
    std::memset(&best_stats, 0, sizeof(best_stats));
    EventPair fin(c);
    if (whole_pairs && (!fin.a || !fin.b)) return fail(QMCP_EHIP, "event creation failed");
    while (!plan.done()) {
        const uint32_t M = plan.next();
        uint64_t* pm = masks[scratch];
        if (words) HIP_TRY(hipMemsetAsync(pm, 0, words * sizeof(uint64_t), st));  // (k_bc_scatter_mask ORs)
        PlainSolver plain(M);
        qmcp_hip_stats sum;
        if (g.live.size() > 1) {
            TRY(run_batches(c, g, plain, pm, sum));
        } else {  // v is the one batch with reads, if any, and bc_starts / bc_ends hold its columns since step 2
            start_sum(g, sum);
            if (!g.live.empty()) TRY(solve_scatter_batch(c, v, plain, pm, sum, true, true));
        }
        uint64_t count = sum.n_kept;
        if (whole_pairs) {
            unsigned long long kept = 0;
            HIP_TRY(hipMemsetAsync(d_acc + qmcp::kBudgetKept, 0, sizeof(unsigned long long), st));
            HIP_TRY(hipEventRecord(fin.a, st));
            {
                KernelSpan sp(c, "k_budget_finish");
                qmcp::launch_budget_finish(st, d_ids, n64, pm, d_acc);
            }
            HIP_TRY(hipEventRecord(fin.b, st));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&kept, d_acc + qmcp::kBudgetKept, sizeof(kept), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            bs.ms_budget += elapsed(fin.a, fin.b);
            count = kept;
        }
        bs.ms_solves += sum.ms_total;
        plan.report(M, count);
        if (count <= budget) {  // the best feasible probe so far: the other mask takes the next one
            best = scratch;
            scratch ^= 1;
            best_stats = sum;
        }
    }
    if (words) {
        if (best < 0)
            HIP_TRY(hipMemsetAsync(d_mask, 0, words * sizeof(uint64_t), st));
        else if (masks[best] != d_mask)
            HIP_TRY(hipMemcpyAsync(d_mask, masks[best], words * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    bs.coverage = plan.lo;
    bs.n_kept = plan.count_lo;
    bs.probes = plan.probes;
    if (plan.hi <= bs.top) {
        bs.kept_above = plan.count_hi;
        bs.bound_above = plan.bound_hi;
    }
    bs.saturated = bs.n_kept == placed ? 1u : 0u;
    if (stats) *stats = best_stats;
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
