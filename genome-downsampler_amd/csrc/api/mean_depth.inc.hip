// mean_depth.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_mean_depth_host / _device: the deepest coverage M* in 0 .. top whose by-contig solve keeps at most
// budget_bases bases inside a region set R (every position without one; after pair completion under
// QMCP_MEAN_DEPTH_WHOLE_PAIRS), and that solve's mask.  The budget entry's flow (api/budget.inc.hip) with bases for reads:
//   1. target_table.h merges the regions on the host (padding 0); group_by_contig, once per call
//   2. k_md_weights, once: w[i] = |read i n R|
//   3. depth_curve (api/cap_search.inc.hip) with k_md_tally over the batch's part of R (its merged regions moved onto the
//      batch's concatenated axis) -- k_budget_tally without a table: S_R(M) = sum over R of min(cov, M), the largest
//      depth and the sum
//   4. budget_plan.h starts with spans of 1: its bound is then S_R(M) itself, and the first probe the largest M with
//      S_R(M) <= budget; search_cap (api/cap_search.inc.hip) runs its probes.  A probe counts the bases its mask keeps:
//      k_budget_finish under the flag, then k_md_count; the MeanDepthWord words come back in one copy
// Buffers: bg_acc (CapAcc: BudgetWord words | curve | histogram | MeanDepthWord words), bg_mask, md_tab (offs | rs | re |
// cum in contig coordinates, then rpos | rcum per batch), md_w.
namespace {

// the regions as both entries check them: after the budget's checks, in the order of the targets entries
int check_mean_depth_regions(const uint32_t* contig_lengths, uint32_t n_contigs, const uint32_t* region_offsets,
                             const uint32_t* region_starts, const uint32_t* region_ends, qmcp::TargetTable& tab) {
    if (!region_offsets) return QMCP_OK;
    if (qmcp::check_target_offsets(region_offsets, n_contigs) != QMCP_OK)
        return fail(QMCP_EINVAL, "region_offsets must start at 0 and never decrease (%u contigs)", n_contigs);
    if (region_offsets[n_contigs] && (!region_starts || !region_ends)) return fail(QMCP_EINVAL, "null region table");
    if (qmcp::build_target_table(region_offsets, region_starts, region_ends, 0, contig_lengths, n_contigs, tab) != QMCP_OK)
        return fail(QMCP_EINVAL, "a region has start > end");
    return QMCP_OK;
}

int solve_mean_depth_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                               uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, uint32_t max_coverage,
                               uint64_t budget, const qmcp::TargetTable* tab, uint32_t flags, uint64_t* curve_out,
                               uint32_t curve_capacity, uint64_t* d_mask, qmcp_hip_stats* stats,
                               qmcp_hip_mean_depth_stats* mstats) {
    qmcp_hip_mean_depth_stats ms;
    std::memset(&ms, 0, sizeof(ms));
    ms.budget = budget;
    if (tab) {
        ms.positions = tab->positions;
        ms.regions_in = tab->regions_in;
        ms.regions_used = tab->regions_merged;
    } else {
        for (uint32_t k = 0; k < n_contigs; ++k) ms.positions += lengths[k];
    }
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (mstats) *mstats = ms;
    const size_t words = (size_t)((n64 + 63) / 64);
    const bool whole_pairs = (flags & QMCP_MEAN_DEPTH_WHOLE_PAIRS) != 0;
    hipStream_t st = c->stream;
    CapAcc a;
    TRY(reserve_cap_acc(c, max_coverage, words, qmcp::kMdWords, a));
    TRY(ensure(c, c->md_w, (size_t)n64 * sizeof(uint32_t) + 16));

    // 1: the grouping (the mask it clears is the call's own: a refused call leaves d_mask alone)
    GroupedReads g;
    TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, c->bg_mask.u64(), g));
    const uint64_t placed = g.offs[n_contigs];

    // the table: in contig coordinates for the weights, on each batch's concatenated axis for the tally
    const uint32_t n_reg = tab ? tab->regions_merged : 0u;
    uint32_t *d_offs = nullptr, *d_rs = nullptr, *d_re = nullptr, *d_cum = nullptr, *d_rpos = nullptr, *d_rcum = nullptr;
    std::vector<uint32_t> rpos(n_reg), rcum(n_reg), batch_pos(g.batches.size(), 0);
    if (tab) {
        for (size_t b = 0; b < g.batches.size(); ++b) {
            const qmcp::ContigBatch& bt = g.batches[b];
            uint32_t off = 0, rank = 0;  // (a batch holds at most 2^31 - 2 positions)
            for (uint32_t k = bt.first_contig; k < bt.first_contig + bt.n_contigs; ++k) {
                for (uint32_t r = tab->offs[k]; r < tab->offs[k + 1]; ++r) {
                    rpos[r] = off + tab->rs[r];
                    rcum[r] = rank;
                    rank += tab->re[r] - tab->rs[r] + 1u;
                }
                off += lengths[k];
            }
            batch_pos[b] = rank;
        }
        TRY(ensure(c, c->md_tab, ((size_t)n_contigs + 1 + 5 * (size_t)n_reg) * sizeof(uint32_t)));
        d_offs = c->md_tab.u32();
        d_rs = d_offs + n_contigs + 1;
        d_re = d_rs + n_reg;
        d_cum = d_re + n_reg;
        d_rpos = d_cum + n_reg;
        d_rcum = d_rpos + n_reg;
        HIP_TRY(hipMemcpyAsync(d_offs, tab->offs.data(), ((size_t)n_contigs + 1) * 4, hipMemcpyHostToDevice, st));
        if (n_reg) {
            HIP_TRY(hipMemcpyAsync(d_rs, tab->rs.data(), (size_t)n_reg * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_re, tab->re.data(), (size_t)n_reg * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_cum, tab->cum.data(), (size_t)n_reg * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_rpos, rpos.data(), (size_t)n_reg * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_rcum, rcum.data(), (size_t)n_reg * 4, hipMemcpyHostToDevice, st));
        }
    }

    // 2: the weights
    ProbeSolve probe{g};
    TimedLaunches timed{c};
    TRY(timed.run([&] {
        KernelSpan sp(c, "k_md_weights");
        qmcp::launch_md_weights(st, d_starts, d_ends, d_ids, (uint32_t)n64, n_contigs, tab != nullptr, d_offs, d_rs, d_re,
                                d_cum, n_reg, c->md_w.u32());
    }));
    // 3: the depth histogram inside R over every batch, the curve
    auto tally = [&](size_t b, const BatchView& v, uint32_t ltot) {
        if (!tab) return tally_every_position(c, a, ltot);
        const uint32_t r0 = tab->offs[v.first_contig], r1 = tab->offs[v.first_contig + v.n_contigs];
        KernelSpan sp(c, "k_md_tally");
        qmcp::launch_md_tally(st, c->cov.u32(), ltot, d_rpos + r0, d_rcum + r0, r1 - r0, batch_pos[b], a.H, a.acc, a.hist);
    };
    DepthCurve d;
    TRY(depth_curve(c, probe, a, max_coverage, timed, tally, d));
    ms.ms_mean_depth = d.ms;
    ms.reads_placed = placed;
    ms.max_depth = d.max_depth;
    ms.total_bases = d.total_bases;
    ms.top = d.top;
    ms.curve_entries = d.copy_out(curve_out, curve_capacity);

    // 4: the probes.  Spans of 1: the planner's bound is the curve itself, its mean span 1
    qmcp::BudgetPlan plan;
    plan.start(d.curve, a.H, d.top, 1, placed, placed, budget);
    uint64_t kept_lo = 0;  // the reads of the best feasible probe
    auto kept_bases = [&](uint64_t* pm, const qmcp_hip_stats&, uint64_t* count) -> int {
        unsigned long long got[qmcp::kMdWords] = {0, 0};
        HIP_TRY(hipMemsetAsync(a.extra, 0, sizeof(got), st));
        if (whole_pairs) HIP_TRY(hipMemsetAsync(a.acc + qmcp::kBudgetKept, 0, sizeof(unsigned long long), st));
        TRY(timed.run([&] {
            if (whole_pairs) {
                KernelSpan sp(c, "k_budget_finish");
                qmcp::launch_budget_finish(st, d_ids, n64, pm, a.acc);
            }
            KernelSpan sp(c, "k_md_count");
            qmcp::launch_md_count(st, pm, c->md_w.u32(), n64, a.extra);
        }));
        HIP_TRY(hipMemcpyAsync(got, a.extra, sizeof(got), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        ms.ms_mean_depth += timed.total();
        *count = got[qmcp::kMdBases];
        if (*count <= budget) kept_lo = got[qmcp::kMdKept];
        return QMCP_OK;
    };
    TRY(search_cap(c, plan, d_mask, c->bg_mask.u64(), words, probe, kept_bases, stats, &ms.ms_solves));
    ms.coverage = plan.lo;
    ms.n_kept = kept_lo;
    ms.kept_bases = plan.count_lo;
    ms.probes = plan.probes;
    if (plan.hi <= ms.top) {
        ms.bases_above = plan.count_hi;
        ms.bound_above = plan.bound_hi;
    }
    ms.saturated = ms.n_kept == placed ? 1u : 0u;
    if (mstats) *mstats = ms;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_mean_depth_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                   uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                   uint32_t max_coverage, uint64_t budget_bases, const uint32_t* region_offsets,
                                   const uint32_t* region_starts, const uint32_t* region_ends, uint32_t flags,
                                   uint64_t* curve_out, uint32_t curve_capacity, uint64_t* keep_mask_out,
                                   qmcp_hip_stats* stats, qmcp_hip_mean_depth_stats* mstats) {
    // (the refusals need no device: they come before the context is looked at)
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(check_budget_call(n_reads, contig_lengths, n_contigs, max_coverage, flags, curve_out, curve_capacity));
    qmcp::TargetTable tab;
    TRY(check_mean_depth_regions(contig_lengths, n_contigs, region_offsets, region_starts, region_ends, tab));
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
    TRY(solve_mean_depth_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), n_reads, contig_lengths,
                                   n_contigs, max_coverage, budget_bases, region_offsets ? &tab : nullptr, flags, curve_out,
                                   curve_capacity, c->mask.u64(), stats, mstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_mean_depth_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                     const uint32_t* d_contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                     uint32_t n_contigs, uint32_t max_coverage, uint64_t budget_bases,
                                     const uint32_t* region_offsets, const uint32_t* region_starts,
                                     const uint32_t* region_ends, uint32_t flags, uint64_t* curve_out,
                                     uint32_t curve_capacity, uint64_t* d_keep_mask_out, void* hip_stream,
                                     qmcp_hip_stats* stats, qmcp_hip_mean_depth_stats* mstats) {
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(check_budget_call(n_reads, contig_lengths, n_contigs, max_coverage, flags, curve_out, curve_capacity));
    qmcp::TargetTable tab;
    TRY(check_mean_depth_regions(contig_lengths, n_contigs, region_offsets, region_starts, region_ends, tab));
    TRY(use_device(c));
    TRY(order_after(c, hip_stream));
    return solve_mean_depth_on_device(c, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, n_contigs, max_coverage,
                                      budget_bases, region_offsets ? &tab : nullptr, flags, curve_out, curve_capacity,
                                      d_keep_mask_out, stats, mstats);
}

}  // extern "C"
