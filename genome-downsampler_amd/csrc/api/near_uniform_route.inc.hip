// near_uniform_route.inc.hip -- part of qmcp_api.hip (one translation unit).
// The near-uniform route's half of the tail (kernels/near_uniform.inc.hip).  Called when the call's spans differ.
// done = true: the keep mask is written (sweep, ranking and the selected exceptions); false: the caller takes the
// mixed-span route (nothing has touched the mask).  The head's producer may already have filtered on c->nu_ell
// (run.nu_filter); otherwise the reads are counted first and, if the longest span is the dominant one, the head's
// stages are queued again with the filter on.
// (stretches two run-ins long instead of the one-span route's four: the route sweeps several times, and a sweep is
//  as long as its longest stretch -- two 10^7-position contigs at 1.5 x M: 0.43 -> 0.24 ms a sweep; one run-in long: 0.37)
constexpr uint32_t kNuRunInsApart = 2;
int near_uniform_tail(qmcp_hip_ctx* c, uint32_t min_span, uint32_t max_span, uint32_t max_load, bool& done) {
    namespace w = qmcp::words;
    done = false;
    SolveRun& run = c->run;
    uint32_t* const d_iters = w::sweep_iters(c->scalars.p);
    const Problem& pr = run.pr;
    qmcp_hip_stats& local = run.local;
    const uint32_t n = (uint32_t)pr.n, ltot = (uint32_t)pr.ltot, n_contigs = run.n_contigs, M = run.M;
    local.near_uniform_giveup = QMCP_NU_GIVEUP_NOT_TRIED;
    if (c->opt.near_uniform < 0) return QMCP_OK;
    const uint32_t ell = max_span;
    const Shape shape{run.n64, pr.ltot, M, ell};
    uint32_t longest = 0;
    for (uint32_t k = 0; k < n_contigs; ++k) longest = run.lengths[k] > longest ? run.lengths[k] : longest;
    // which sweep the rounds run, and whether the route is tried at all (sweep_plan.h)
    const qmcp::NearUniformPlan plan = qmcp::plan_near_uniform(c->opt, n, ell, min_span, ltot, n_contigs, longest, M, run.may_rank);
    const bool stretches = plan.stretches, speculate = plan.speculate;
    const bool dbg = c->opt.near_uniform_debug == 1;
    if (dbg) fprintf(stderr, "[near] pm %d may_rank %d ell %u ev %d depth %.2f min_span %u filter %u\n", (int)run.pm,
                     (int)run.may_rank, ell, (int)qmcp::sweep_uniform_ev_supported(ell, M), plan.depth, min_span, run.nu_filter);
    if (!plan.tried) return QMCP_OK;
    if (c->mem.nu_failed == shape) {
        local.near_uniform_giveup = QMCP_NU_GIVEUP_REMEMBERED;
        c->nu_ell = 0;
        return QMCP_OK;
    }
    hipStream_t st = c->stream;
    const uint32_t cap = nu_cap_for(n);
    uint32_t n_exc = 0;
    uint32_t* d_stats = c->stats.u32();
    if (run.nu_filter == ell) {
        n_exc = c->h_head[w::kHeadExceptions];  // (read back beside the statistics)
        if (c->h_head[w::kHeadListOverflowed] != 0) { c->nu_ell = 0; local.near_uniform_giveup = QMCP_NU_GIVEUP_TOO_MANY; return QMCP_OK; }  // a pass held more exceptions than it can stage
    } else {
        // how many reads have the longest span?  (one pass over the spans; the host waits for the count)
        TRY(ensure_near_uniform(c, n, ltot, n_contigs));
        uint32_t* d_count = d_stats + w::kLongestSpanReads;
        HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint32_t), st));
        qmcp::launch_nu_count_span(st, run.d_starts, run.d_ends, n, ell, d_count);
        HIP_TRY(hipMemcpyAsync(c->h_nu + w::kNuScratch, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        n_exc = n - c->h_nu[w::kNuScratch];
        if (dbg) fprintf(stderr, "[near] reads of span %u: %u of %u, list holds %u\n", ell, c->h_nu[w::kNuScratch], n, cap);
        if (n_exc > n / 10u) {
            // (fewer than nine tenths of the reads have the LONGEST span: either many exceptions, or -- nearly all reads
            //  shorter than a few -- the dominant span is not the longest: reads lengthened by a deletion)
            c->nu_ell = 0;
            local.near_uniform_giveup = n_exc > n - n / 10u ? QMCP_NU_GIVEUP_LONGER_READS : QMCP_NU_GIVEUP_TOO_MANY;
            return QMCP_OK;
        }
        // the head again, regular reads only (exceptions listed): producer, scan, range table, bucket offsets
        c->nu_ell = ell;
        if (run.pm) TRY(queue_pm_head(c, st, ell, true));
        else TRY(queue_rm_head(c, st, ell, true));
        HIP_TRY(hipMemcpyAsync(c->h_nu + w::kNuScratch, w::max_load(c->ranges.u32()), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(c->h_nu + w::kNuSelectedLast, d_stats + w::kExceptions, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        max_load = c->h_nu[w::kNuScratch];
        if (c->h_nu[w::kNuSelectedLast] != n_exc || c->h_nu[w::kNuFlags] != 0) { c->nu_ell = 0; local.near_uniform_giveup = QMCP_NU_GIVEUP_TOO_MANY; return QMCP_OK; }  // (a pass held more than it can stage)
    }
    local.near_uniform_exceptions = n_exc;
    if (n_exc == 0 || n_exc > n / 10u || (uint64_t)max_load * kRankBalance > (uint64_t)n) {
        if (n_exc > n / 10u) c->nu_ell = 0;
        local.near_uniform_giveup = n_exc > n / 10u ? QMCP_NU_GIVEUP_TOO_MANY : n_exc == 0 ? QMCP_NU_GIVEUP_NOT_TRIED : QMCP_NU_GIVEUP_HEAVY_RANGE;
        return QMCP_OK;
    }
    // scratch of the event-driven sweep (launch_uniform_sweep)
    const uint32_t ev_wg_max = qmcp::sweep_ev_workgroups_max(n_contigs);
    if (!stretches) {
        TRY(ensure(c, c->evpk, qmcp::sweep_ev_pack_bytes(ltot, ell, ev_wg_max)));
        TRY(ensure(c, c->evlast, qmcp::sweep_ev_last_bytes(ltot, ell, ev_wg_max)));
    }
    const uint32_t* boff = c->boff.u32();
    const uint64_t* poff = c->poff.u64();
    uint32_t* selend = c->selend.u32();
    uint32_t* exc = c->nu_exc.u32();
    int32_t* nadj = c->nu_nadj.as<int32_t>();
    uint32_t* state = c->nu_state.u32();
    unsigned long long* viol_key = (unsigned long long*)(c->nu_state.as<char>() + 64);
    uint32_t* viol_idx = (uint32_t*)(viol_key + n_contigs);
    uint32_t* sweep_from[2] = {viol_idx + n_contigs, viol_idx + 2 * (size_t)n_contigs};  // this round's, the next round's
    if (!stretches) TRY(ensure(c, c->nu_ckpt, qmcp::sweep_ev_ckpt_bytes(ltot, ell, ev_wg_max)));
    HIP_TRY(hipMemsetAsync(sweep_from[0], 0, (size_t)n_contigs * sizeof(uint32_t), st));
    HIP_TRY(hipEventRecord(c->ev[EV_SCAN], st));
    HIP_TRY(hipEventRecord(c->ev[EV_SORT], st));
    {
        KernelSpan sp(c, "near-uniform setup (exception coverage, need, pre-selection)");
        qmcp::launch_nu_setup(st, exc, cap, n_exc, d_stats + w::kOverflowEntries, boff, ltot, ell, M, c->nu_ce.u32(), c->spine.u32(),
                              nadj, state);
    }
    qmcp::SweepAxis ax{st, boff, poff, n_contigs, ltot};
    const uint32_t windows = plan.windows, burn_blocks = plan.burn_blocks;
    // stretches: the exact table once (the cut points do not move between rounds), the speculative ones per sweep
    if (windows != 0) {
        KernelSpan sp(c, "k_find_cuts", st);
        ax = qmcp::launch_sweep_segments(ax, nullptr, ell, M, windows, c->segs.u32(), c->nu_ce.u32());
    }
    // later rounds sweep only the exact stretches a selection of the round before touched (k_nu_select_apply marks them)
    uint32_t* marks[2] = {(uint32_t*)(c->nu_sus.as<char>() + qmcp::nu_suspect_bytes(nu_suspects_for(n))), nullptr};
    const uint32_t mw = nu_marks_words(n_contigs);
    marks[1] = marks[0] + mw;
    // ... and, where the sweeps speculate, only the first tier's stretches that read or write something a selection changed
    // (k_nu_select_apply; a boundary is compared when the stretch on either side of it was swept)
    uint32_t* fine[2] = {marks[1] + mw, marks[1] + 2 * (size_t)mw};
    uint32_t* dirty[2] = {fine[1] + mw, nullptr};  // (cells a replay reads from that changed: kernels/near_uniform.inc.hip NuBins)
    dirty[1] = dirty[0] + qmcp::nu_cells_bytes() / sizeof(uint32_t);
    if (stretches) HIP_TRY(hipMemsetAsync(dirty[0], 0, 2 * qmcp::nu_cells_bytes(), st));
    // (the first tier's table: launch_sweep_segments_speculative(..., tier 1) builds it at this place on every sweep, from
    //  the same cut points -- the same table every round)
    const uint32_t* seg_fine = speculate ? c->segs.u32() + qmcp::sweep_segment_table_offset(n_contigs, windows, 1) : nullptr;
    if (c->opt.near_uniform_debug == 2) seg_fine = nullptr;  // (lab: every round sweeps every stretch its exact marks cover)
    // Rounds are queued two at a time and the host looks at the state words after each pair: a round whose contigs are
    // all settled is eight launches that return at once (the chain sweeps nothing, the verification skips every
    // exception: ~0.1 ms), about what one more host round trip costs; measured at cfg4 with 1 % clipped reads (7 rounds),
    // batches of 1 / 2 / 2 + 4 + 4: 4.62 / 4.5 / 4.60 ms.
    uint32_t rounds = 0;
    bool settled = false;
    const uint32_t budget = nu_round_budget(c, run.lengths, n_contigs);
    // A shape that settled within a few rounds last time: queue that many (a round whose contigs are all settled sweeps
    // and verifies nothing) and the ranking behind them WITHOUT waiting in between; collect_one looks at the state words.
    const bool defer = !dbg && c->opt.near_uniform_rounds == 0 && c->mem.nu_need_rounds != 0 && c->mem.nu_need_rounds <= 8 &&
                       c->mem.nu_need == shape && run.nu_filter == ell;
    while (rounds < budget && !settled) {
        const uint32_t batch = 2u;
        for (uint32_t r = 0; r < batch; ++r) {
            ++rounds;
            if (stretches) {
                if (speculate) {
                    // (the first tier's stretches a selection of the round before left alone keep their output)
                    auto own_marks = [&](const qmcp::SweepAxis& tier) {
                        return (tier.seg == seg_fine && rounds > 1) ? fine[0] : nullptr;
                    };
                    TRY(speculative_sweep(
                        c, ax, ell, ell, burn_blocks, kNuRunInsApart, "k_sweep_uniform_gen",
                        [&](const qmcp::SweepAxis& tier, uint32_t* run_in_out, const uint32_t* redo_in) {
                            return qmcp::launch_sweep_uniform_gen(tier, ell, M, selend, d_iters, run_in_out, redo_in, nadj,
                                                                  own_marks(tier));
                        },
                        [&](const qmcp::SweepAxis& tier, uint32_t* mismatches, const uint32_t* redo_in, uint32_t* redo_out) {
                            qmcp::launch_spec_verify(tier, ell, selend, c->cstart.u32(), mismatches, redo_in, redo_out,
                                                     own_marks(tier));
                        },
                        rounds == 1 ? nullptr : marks[0]));
                } else {
                    KernelSpan sp(c, "k_sweep_uniform_gen", st);
                    if (!qmcp::launch_sweep_uniform_gen(ax, ell, M, selend, d_iters, nullptr,
                                                        (ax.seg != nullptr && rounds > 1) ? marks[0] : nullptr, nadj))
                        return fail(QMCP_ERANGE, "near-uniform route: span %u not supported", ell);
                }
            } else {
            {
                KernelSpan sp(c, "k_sweep_pack", st);
                qmcp::launch_sweep_ev_pack(ax, ell, M, c->evpk.u32(), nadj, sweep_from[0]);
            }
            {
                KernelSpan sp(c, "k_sweep_uniform_ev", st);
                qmcp::launch_sweep_ev_chain(ax, ell, M, c->evpk.u32(), c->cstart.u32(), c->evlast.u32(), d_iters, nadj,
                                            c->nu_ckpt.u32(), sweep_from[0]);
            }
            {
                KernelSpan sp(c, "k_sweep_expand", st);
                qmcp::launch_sweep_ev_expand(ax, ell, M, c->cstart.u32(), c->evlast.u32(), selend, sweep_from[0]);
            }
            }
            {
                KernelSpan sp(c, "near-uniform round (verify, replay, select, apply)");
                qmcp::launch_nu_round(st, exc, cap, n_exc, d_stats + w::kOverflowEntries, rounds == 1, boff, selend, nadj, c->nu_ce.u32(), poff, n_contigs, ell, M,
                                      c->nu_sus.as<uint2>(), nu_suspects_for(n), state, viol_key, viol_idx, sweep_from[0], sweep_from[1],
                                      ltot, c->spine.u32(), stretches ? ax.seg : nullptr, ax.n_seg_max, marks[1],
                                      stretches ? c->nu_prev.u32() : nullptr, dirty[0], dirty[1], seg_fine, fine[1]);
                std::swap(sweep_from[0], sweep_from[1]);
                std::swap(marks[0], marks[1]);
                std::swap(fine[0], fine[1]);
                std::swap(dirty[0], dirty[1]);
            }
        }
        HIP_TRY(hipGetLastError());
        if (defer && rounds < c->mem.nu_need_rounds) continue;
        HIP_TRY(hipMemcpyAsync(c->h_nu, state, w::kNuStateWords * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (defer) break;  // (looked at when the solve is collected)
        HIP_TRY(hipStreamSynchronize(st));
        if (dbg) {
            uint32_t more[8];
            (void)hipMemcpy(more, state + 8, sizeof(more), hipMemcpyDeviceToHost);
            fprintf(stderr, "[near] open question: s %u u1 %u S(u1-1) %u C(u1-1) %u b %u c0 %u\n", more[0], more[1], more[2], more[3], more[4], more[5]);
            fprintf(stderr, "[near] after %u rounds: last round selected %u, flags %u (read %u), selected in all %u, suspects %u, rounds that selected %u; next sweeps from block",
                    rounds, c->h_nu[w::kNuSelectedLast], c->h_nu[w::kNuFlags], c->h_nu[w::kNuFlagsRead], c->h_nu[w::kNuSelected],
                    c->h_nu[w::kNuSuspects], c->h_nu[w::kNuRoundsThatSelected]);
            std::vector<uint32_t> from(n_contigs);
            (void)hipMemcpy(from.data(), sweep_from[0], (size_t)n_contigs * sizeof(uint32_t), hipMemcpyDeviceToHost);
            for (uint32_t k = 0; k < n_contigs && k < 16; ++k) fprintf(stderr, " %d", (int)from[k]);
            fprintf(stderr, "\n");
        }
        if (c->h_nu[w::kNuFlags] != 0) break;          // a run the replay does not model, or too many suspects
        settled = c->h_nu[w::kNuSelectedLast] == 0;    // the last round wanted no exception: the sweep's counts are the greedy's
    }
    c->nu_deferred = defer;
    if (defer) {
        settled = true;  // (provisionally: collect_one checks, and solves the call again if it is not)
    } else if (settled) {
        c->mem.nu_need = shape;
        c->mem.nu_need_rounds = rounds;                   // (queued: an even number)
        rounds = c->h_nu[w::kNuRoundsThatSelected] + 1;   // (the rounds that did something, and the one that found nothing left)
    }
    local.near_uniform_rounds = rounds;
    local.near_uniform_selected = defer ? 0u : c->h_nu[w::kNuSelected];
    if (!settled) {
        c->mem.nu_need_rounds = 0;
        // (the head must not filter on this span again, and the next call of this shape must not burn the budget again)
        local.near_uniform_giveup = c->h_nu[w::kNuFlags] != 0 ? QMCP_NU_GIVEUP_UNMODELLED : QMCP_NU_GIVEUP_BUDGET;
        c->nu_ell = 0;
        c->mem.nu_failed = shape;
        return QMCP_OK;
    }
    local.near_uniform_giveup = QMCP_NU_GIVEUP_NONE;
    HIP_TRY(hipEventRecord(c->ev[EV_SWEEP], st));
    queue_rank(c, st, nullptr, nullptr, 0);
    {
        KernelSpan sp(c, "k_nu_mark_selected");
        qmcp::launch_nu_mark_selected(st, exc, cap, n_exc, d_stats + w::kOverflowEntries, (unsigned long long*)run.d_mask,
                                      c->scalars.as<unsigned long long>());
    }
    HIP_TRY(hipGetLastError());
    done = true;
    return QMCP_OK;
}
