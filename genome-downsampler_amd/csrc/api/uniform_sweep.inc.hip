// uniform_sweep.inc.hip -- part of qmcp_api.hip (one translation unit).
// The one-length sweep's launches: block-scan pipelines, event-driven form, stretches at cut points, speculative boundaries in
// tiers.  Which of them a call takes is decided in sweep_plan.h (plan_uniform_sweep).

// The tiers of a speculative sweep over `ax`, the axis under its exact table.  `unit`: positions per block of run-in (the
// span; the largest span of a mix), `round_to`: the run-in is made a multiple of this many positions.  sweep(the axis
// under a tier's table, second output or null, marks to obey or null) launches the sweep kernel; check(that axis,
// mismatch counter, marks to obey or null, marks to set) the comparison and the merge behind it.  A disagreement marks
// the exact stretch it lies in; tier 2 (three times the run-in) sweeps only marked parts, the exact sweep only what
// tier 2 marked.
template <class Sweep, class Check>
int speculative_sweep(qmcp_hip_ctx* c, const qmcp::SweepAxis& ax, uint32_t unit, uint32_t round_to, uint32_t burn_blocks,
                      uint32_t run_ins_apart, const char* sweep_name, Sweep sweep, Check check,
                      const uint32_t* only_marked = nullptr /* per exact stretch: the parts of the genome to sweep at all
                                                               (the near-uniform route's later rounds); null: everything */) {
    const qmcp::words::SpecWords w = qmcp::words::spec_words(c->scalars.p);  // (behind the solve's other scalars)
    hipStream_t st = ax.st;
    const uint32_t n_cand = ax.n_seg_max, windows = n_cand - ax.n_contigs;
    TRY(ensure(c, c->specflags, 2 * (size_t)n_cand * sizeof(uint32_t)));
    uint32_t* redo1 = c->specflags.u32();
    uint32_t* redo2 = redo1 + n_cand;
    HIP_TRY(hipMemsetAsync(redo1, 0, 2 * (size_t)n_cand * sizeof(uint32_t), st));
    auto positions = [&](uint64_t blocks) { return (uint32_t)((blocks * unit + round_to - 1) / round_to * round_to); };
    const uint32_t burn1 = positions(burn_blocks);
    uint32_t burn2 = positions(3ull * burn_blocks);
    if ((uint64_t)ax.ltot < 2ull * run_ins_apart * burn2) burn2 = 0;  // too short a genome: tier 2 is the exact table
    qmcp::SweepAxis tier1 = ax, tier2 = ax;
    {
        KernelSpan sp(c, "k_find_cuts", st);
        tier1.seg = qmcp::launch_sweep_segments_speculative(ax, windows, burn1, c->segs.u32(), w.n_spec1, run_ins_apart, 1);
        tier2.seg = qmcp::launch_sweep_segments_speculative(ax, windows, burn2, c->segs.u32(), w.n_spec2, run_ins_apart, 2);
    }
    // the second output: one span -- every stretch's run-in; a mix of spans -- the odd stretches' whole output
    uint32_t* second_out = c->cstart.u32();
    {
        KernelSpan sp(c, sweep_name, st);
        if (!sweep(tier1, second_out, only_marked)) return fail(QMCP_ERANGE, "speculative sweep: span not supported");
    }
    {
        KernelSpan sp(c, "k_spec_verify + k_spec_merge", st);
        check(tier1, w.mismatches1, only_marked, redo1);
    }
    {
        KernelSpan sp(c, "second tier, where the first disagreed", st);
        (void)sweep(tier2, second_out, redo1);
        check(tier2, w.mismatches2, redo1, redo2);
    }
    KernelSpan sp(c, "exact sweep, where the second tier disagreed", st);
    (void)sweep(ax, nullptr, redo2);
    HIP_TRY(hipGetLastError());
    return QMCP_OK;
}
int launch_uniform_sweep(qmcp_hip_ctx* c, hipStream_t st, uint32_t n, uint32_t ltot, uint32_t n_contigs,
                         uint32_t span, uint32_t M, uint32_t* d_iters, uint32_t empty_positions,
                         bool* expand_left_out = nullptr /* in: the caller can read the event sweep's own output;
                                                            out: the event sweep ran whole contigs and selend[] was not written */) {
    const bool may_leave_expand = expand_left_out != nullptr && *expand_left_out;
    if (expand_left_out) *expand_left_out = false;
    const qmcp::UniformSweepPlan plan = qmcp::plan_uniform_sweep(c->opt, n, span, ltot, n_contigs, M, empty_positions);
    uint32_t* selend = c->selend.u32();
    qmcp::SweepAxis ax{st, c->boff.u32(), c->poff.u64(), n_contigs, ltot};
    if (plan.windows != 0) {
        KernelSpan sp(c, "k_find_cuts", st);
        ax = qmcp::launch_sweep_segments(ax, nullptr, span, M, plan.windows, c->segs.u32());
    }
    switch (plan.form) {
    case qmcp::UniformForm::Events: {
        // scratch of the event-driven form: 256 bytes per block, so it depends on the span, which is only
        // known here -- grown on the first deep call of a size (ensure() waits for the streams then), kept after
        {
            const uint32_t wg_max = qmcp::sweep_ev_workgroups_max(n_contigs);
            TRY(ensure(c, c->evpk, qmcp::sweep_ev_pack_bytes(ltot, span, wg_max)));
            TRY(ensure(c, c->evlast, qmcp::sweep_ev_last_bytes(ltot, span, wg_max)));
        }
        uint32_t* pk = c->evpk.u32();
        uint32_t* sev = c->cstart.u32();
        uint32_t* lastns = c->evlast.u32();
        {
            KernelSpan sp(c, "k_sweep_pack", st);
            qmcp::launch_sweep_ev_pack(ax, span, M, pk);
        }
        {
            KernelSpan sp(c, "k_sweep_uniform_ev", st);
            qmcp::launch_sweep_ev_chain(ax, span, M, pk, sev, lastns, d_iters);
        }
        if (may_leave_expand && ax.seg == nullptr) {
            *expand_left_out = true;  // (the ranking reads sev / lastns itself)
            return QMCP_OK;
        }
        KernelSpan sp(c, "k_sweep_expand", st);
        qmcp::launch_sweep_ev_expand(ax, span, M, sev, lastns, selend);
        return QMCP_OK;
    }
    case qmcp::UniformForm::SpeculativeGeneral:
        return speculative_sweep(
            c, ax, plan.unit, plan.round_to, plan.burn_blocks, plan.run_ins_apart, "k_sweep_uniform_gen",
            [&](const qmcp::SweepAxis& tier, uint32_t* run_in_out, const uint32_t* redo_in) {
                return qmcp::launch_sweep_uniform_gen(tier, span, M, selend, d_iters, run_in_out, redo_in);
            },
            [&](const qmcp::SweepAxis& tier, uint32_t* mismatches, const uint32_t* redo_in, uint32_t* redo_out) {
                qmcp::launch_spec_verify(tier, span, selend, c->cstart.u32(), mismatches, redo_in, redo_out);
            });
    case qmcp::UniformForm::General:
    case qmcp::UniformForm::Fast: {
        const bool gen = plan.form == qmcp::UniformForm::General;
        KernelSpan sp(c, gen ? "k_sweep_uniform_gen" : "k_sweep_uniform_mw", st);
        const bool ok = gen ? qmcp::launch_sweep_uniform_gen(ax, span, M, selend, d_iters)
                            : qmcp::launch_sweep_uniform_mw(ax, span, M, selend, d_iters);
        if (ok) return QMCP_OK;
        break;  // (the single-wave kernel)
    }
    case qmcp::UniformForm::SingleWave:
        break;
    }
    KernelSpan sp(c, "k_sweep_uniform", st);
    if (!qmcp::launch_sweep_uniform(ax, span, M, selend, d_iters)) return fail(QMCP_ERANGE, "uniform span %u not supported", span);
    return QMCP_OK;
}
