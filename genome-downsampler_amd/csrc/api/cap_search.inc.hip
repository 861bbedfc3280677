// cap_search.inc.hip -- part of qmcp_api.hip (one translation unit).
// What the entries that solve one grouping again and again at different coverages share:
//   ProbeSolve     (budget, mean-depth, thresholds) the whole call solved at M into an input-order mask; a call of one
//                  batch with reads gathers its columns once for all its solves
//   TimedLaunches  launches bracketed by event pairs one by one, their times summed after the next wait
//   CapAcc         (budget, mean-depth) bg_acc's layout; reserve_cap_acc sizes and clears it, and sizes bg_mask
//   depth_curve    (budget, mean-depth) the histogram of the per-position depths over every batch, the curve from it
//   search_cap     (budget, mean-depth) the probes budget_plan.h picks, between two masks, and the best one's mask
namespace {

struct ProbeSolve {
    const GroupedReads& g;
    BatchView v;            // the batch gather() took last: in a call of one batch with reads, that batch
    bool gathered = false;  // ... and bc_starts / bc_ends hold its columns: no probe gathers them again

    // batch b's columns, in grouped order, into bc_starts / bc_ends
    int gather(qmcp_hip_ctx* c, size_t b) {
        g.view(b, v);
        TRY(gather_batch(c, v, g.d_starts, g.d_ends));
        gathered = g.live.size() == 1;
        return QMCP_OK;
    }

    // the whole call at M into d_mask (input order; the scatter ORs, so the caller has cleared it); `sum` takes the stats
    int solve(qmcp_hip_ctx* c, uint32_t M, uint64_t* d_mask, qmcp_hip_stats& sum) {
        PlainSolver plain(M);
        if (g.live.size() > 1) return run_batches(c, g, plain, d_mask, sum);
        start_sum(g, sum);
        if (g.live.empty()) return QMCP_OK;
        if (!gathered) TRY(gather(c, g.live.front()));
        return solve_scatter_batch(c, v, plain, d_mask, sum, true, true);
    }
};

struct TimedLaunches {
    qmcp_hip_ctx* c;
    std::vector<std::unique_ptr<EventPair>> evs;  // one per run() since the last total()

    template <typename Launch>
    int run(Launch launch) {
        evs.emplace_back(new EventPair(c));
        const EventPair& ev = *evs.back();
        if (!ev.a || !ev.b) return fail(QMCP_EHIP, "event creation failed");
        HIP_TRY(hipEventRecord(ev.a, c->stream));
        launch();
        HIP_TRY(hipEventRecord(ev.b, c->stream));
        HIP_TRY(hipGetLastError());
        return QMCP_OK;
    }

    // the sum of the launches' own times, not the time from the first to the last; only after a wait
    float total() {
        float ms = 0.f;
        for (auto& ev : evs) ms += elapsed(ev->a, ev->b);
        evs.clear();
        return ms;
    }
};

// bg_acc: BudgetWord words | curve | histogram | `extra` words of the caller's; H entries each for the coverages
// 0 .. min(max_coverage, QMCP_BUDGET_CURVE_MAX)
struct CapAcc {
    uint32_t H = 0;
    unsigned long long *acc = nullptr, *curve = nullptr, *hist = nullptr, *extra = nullptr;
};

// bg_acc sized and cleared, bg_mask sized for a mask of `words` words
int reserve_cap_acc(qmcp_hip_ctx* c, uint32_t max_coverage, size_t words, size_t extra, CapAcc& a) {
    a.H = std::min(max_coverage, (uint32_t)QMCP_BUDGET_CURVE_MAX) + 1u;
    const size_t acc_words = (size_t)qmcp::kBudgetWords + 2 * (size_t)a.H + extra;
    TRY(ensure(c, c->bg_mask, words * sizeof(uint64_t)));
    TRY(ensure(c, c->bg_acc, acc_words * sizeof(unsigned long long)));
    a.acc = c->bg_acc.as<unsigned long long>();
    a.curve = a.acc + qmcp::kBudgetWords;
    a.hist = a.curve + a.H;
    a.extra = a.hist + a.H;
    HIP_TRY(hipMemsetAsync(a.acc, 0, acc_words * sizeof(unsigned long long), c->stream));
    return QMCP_OK;
}

// the per-position depth of a gathered batch into c->cov (coverage_common's launches, on device columns); *span_max takes
// the batch's largest span
int gathered_batch_depth(qmcp_hip_ctx* c, const BatchView& v, uint32_t* ltot_out, uint32_t* span_max) {
    const uint32_t *bs_starts = c->bc_starts.u32(), *bs_ends = c->bc_ends.u32();
    Problem pr;
    TRY(check_problem(v.roff.data(), v.lengths, v.n_contigs, v.nb, pr));
    const uint32_t n = (uint32_t)pr.n, ltot = (uint32_t)pr.ltot;
    *ltot_out = ltot;
    if (ltot == 0 || n == 0) return QMCP_OK;
    TRY(upload_tables(c, v.roff.data(), pr));
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

// the tally where every position counts: the depths in c->cov into the histogram, the largest and their sum
void tally_every_position(qmcp_hip_ctx* c, const CapAcc& a, uint32_t ltot) {
    KernelSpan sp(c, "k_budget_tally");
    qmcp::launch_budget_tally(c->stream, c->cov.u32(), ltot, a.H, a.acc, a.hist);
}

struct DepthCurve {
    std::vector<unsigned long long> back;  // the BudgetWord words and the curve as they came back
    const uint64_t* curve = nullptr;       // S(0 .. H - 1), in `back`
    uint32_t max_depth = 0, top = 0, span_max = 0;
    uint64_t total_bases = 0;
    float ms = 0.f;  // `timed`: the caller's launches before the stage, the tallies, k_budget_curve

    // what fits of S(0 .. min(top, QMCP_BUDGET_CURVE_MAX)) into curve_out -> the entries written
    uint32_t copy_out(uint64_t* curve_out, uint32_t curve_capacity) const {
        if (!curve_out || !curve_capacity) return 0;
        const uint32_t entries = std::min(std::min(top, (uint32_t)QMCP_BUDGET_CURVE_MAX), curve_capacity - 1u) + 1u;
        for (uint32_t m = 0; m < entries; ++m) curve_out[m] = curve[m];
        return entries;
    }
};

// Per batch with reads, before the first probe: its columns gathered (in a call of one such batch, the gather its probes
// reuse), its depth built, and tally(b, v, ltot) -- the caller's launch, under its own span, over the ltot depths of batch
// b, view v, in c->cov.  Then k_budget_curve; the curve, the largest depth and the sum of the depths come back in one copy.
// The stage passes through the solve's own arena (cstart, boff, ecnt, eoff, cov) and holds nothing of it afterwards.
template <typename Tally>
int depth_curve(qmcp_hip_ctx* c, ProbeSolve& probe, const CapAcc& a, uint32_t max_coverage, TimedLaunches& timed,
                Tally tally, DepthCurve& d) {
    hipStream_t st = c->stream;
    for (size_t b : probe.g.live) {  // (no read: no depth)
        TRY(probe.gather(c, b));
        uint32_t ltot = 0;
        TRY(gathered_batch_depth(c, probe.v, &ltot, &d.span_max));
        TRY(timed.run([&] { tally(b, probe.v, ltot); }));
    }
    TRY(timed.run([&] {
        KernelSpan sp(c, "k_budget_curve");
        qmcp::launch_budget_curve(st, a.hist, a.H, a.curve);
    }));
    d.back.resize((size_t)qmcp::kBudgetWords + a.H);
    HIP_TRY(hipMemcpyAsync(d.back.data(), a.acc, d.back.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    d.ms = timed.total();
    d.curve = (const uint64_t*)(d.back.data() + qmcp::kBudgetWords);
    d.max_depth = (uint32_t)d.back[qmcp::kBudgetMaxDepth];
    d.total_bases = d.back[qmcp::kBudgetTotalBases];
    d.top = std::min(max_coverage, d.max_depth);
    return QMCP_OK;
}

// The probes of a started plan, the mask of the best feasible one (an empty mask if none was) settled into d_mask, the
// final wait and the spans.  measure(pm, sum, &count) counts what the plan is told of the probe whose mask is pm and
// whose stats are `sum`; it may launch, copy back and wait.  `stats` takes the best probe's, *ms_solves every probe's
// solve time.  d_spare is the second input-order mask.
template <typename Measure>
int search_cap(qmcp_hip_ctx* c, qmcp::BudgetPlan& plan, uint64_t* d_mask, uint64_t* d_spare, size_t words, ProbeSolve& probe,
               Measure measure, qmcp_hip_stats* stats, float* ms_solves) {
    hipStream_t st = c->stream;
    uint64_t* masks[2] = {d_mask, d_spare};
    int best = -1, scratch = 0;
    qmcp_hip_stats best_stats;
    std::memset(&best_stats, 0, sizeof(best_stats));
    while (!plan.done()) {
        const uint32_t M = plan.next();
        uint64_t* pm = masks[scratch];
        if (words) HIP_TRY(hipMemsetAsync(pm, 0, words * sizeof(uint64_t), st));  // (k_bc_scatter_mask ORs)
        qmcp_hip_stats sum;
        TRY(probe.solve(c, M, pm, sum));
        uint64_t count = 0;
        TRY(measure(pm, sum, &count));
        *ms_solves += sum.ms_total;
        plan.report(M, count);
        if (count <= plan.budget) {  // the best feasible probe so far: the other mask takes the next one
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
    if (stats) *stats = best_stats;
    return QMCP_OK;
}

}  // namespace
