// solve_tail.inc.hip -- part of qmcp_api.hip (one translation unit).
// A solve's tail, collection, context creation, the enqueue / complete pair.  The tail (enqueue_tail, below the routes) is
// three steps: read_head (wait for the head's read-back, validate it), the pick of the route -- the one place where it is
// decided --, and the route: a straight-line function that queues its launches in order and ends in close_solve.  The
// stages the sort-based routes share with the capped solve are solve_stages.inc.hip's.

// what the head's read-back says about the call
struct HeadFacts {
    uint32_t min_span, max_span;
    uint32_t max_load;         // reads in the heaviest range (0: the range-ranked head did not run)
    uint32_t empty_positions;  // the last solve of this shape's, or this one's (~0: unknown)
    bool uniform;              // one span, and one the block sweep takes
};

// The closing step of every route but the trivial one: EV_MARK, the scalar read-back, and what collect_one needs.
// whole_contigs: the sweep ran without a stretch table that counts its own stretches (mixed spans, no cut points).
int close_solve(qmcp_hip_ctx* c, bool whole_contigs = false) {
    namespace w = qmcp::words;
    SolveRun& run = c->run;
    TRY(queue_result_scalars(c));
    c->pend_spiky = run.ranked_counted;
    if (run.ranked_counted) {
        HIP_TRY(hipMemcpyAsync(c->h_scalars + w::kHostEmptyPositions, c->stats.u32() + w::kEmptyPositions, sizeof(uint32_t),
                               hipMemcpyDeviceToHost, c->stream));
        c->mem.spiky = Shape{run.n64, run.pr.ltot};
    }
    c->pend_stats = run.local;
    c->pend_M = run.M;
    c->pend_whole_contig_chains = whole_contigs ? whole_contig_chains(run.lengths, run.n_contigs) : 0u;
    c->pending = true;
    return QMCP_OK;
}

// Step 1: wait for the head's read-back and validate it.
int read_head(qmcp_hip_ctx* c, HeadFacts& h) {
    namespace w = qmcp::words;
    SolveRun& run = c->run;
    const uint32_t* hs = c->h_head;
    if (run.may_rank) {
        HIP_TRY(hipStreamSynchronize(c->stream2));
        if (run.wait_empty) HIP_TRY(hipStreamSynchronize(c->stream));
        if (hs[w::kHeadBadRead] != 0) {
            (void)hipStreamSynchronize(c->stream);  // what was queued stays in bounds; let it drain
            return fail(QMCP_EREAD, "a read has start > end or end >= its contig length");
        }
    }
    h.min_span = hs[w::kHeadMinSpan];
    h.max_span = hs[w::kHeadMaxSpan];
    h.max_load = hs[w::kHeadMaxLoad];
    h.empty_positions = hs[w::kHeadEmptyPositions];
    h.uniform = h.min_span == h.max_span && h.max_span <= qmcp::kMaxUniformSpan;
    if (run.pm) run.local.pm_heaviest_wave_slots = hs[w::kHeadMaxLoadWaveSlots];
    run.local.min_span = h.min_span;
    run.local.max_span = h.max_span;
    if (!h.uniform && h.max_span > qmcp::kMaxGeneralSpan)
        return fail(QMCP_ERANGE, "mixed-span reads with span %u > %u are not supported by this build",
                    h.max_span, qmcp::kMaxGeneralSpan);
    run.local.path = h.uniform ? QMCP_PATH_UNIFORM : QMCP_PATH_GENERAL;
    if (h.uniform)
        for (uint32_t k = 0; k < run.n_contigs; ++k)
            if (run.roff[k + 1] - run.roff[k] >= (1ull << 28))
                return fail(QMCP_ERANGE, "contig %u holds %llu reads; the block sweep handles < 2^28 per contig",
                            k, (unsigned long long)(run.roff[k + 1] - run.roff[k]));
    return QMCP_OK;
}

// The head listed every read as an exception to the last call's span: its stages again, unfiltered, and the heaviest
// range's load as it is now.
int head_again_unfiltered(qmcp_hip_ctx* c, HeadFacts& h) {
    namespace w = qmcp::words;
    c->nu_ell = 0;
    if (c->run.pm) TRY(queue_pm_head(c, c->stream, 0, true));
    else TRY(queue_rm_head(c, c->stream, 0, true));
    HIP_TRY(hipMemcpyAsync(c->h_nu + w::kNuScratch, w::max_load(c->ranges.u32()), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    h.max_load = c->h_nu[w::kNuScratch];
    return QMCP_OK;
}

// global start position per read into vals[1], where the head has not left it there (the range-ranked head)
void need_gstart(qmcp_hip_ctx* c) {
    SolveRun& run = c->run;
    if (run.have_gstart) return;
    KernelSpan sp(c, "k_gstart");
    qmcp::launch_gstart(c->stream, run.d_starts, (uint32_t)run.pr.n, c->roff.u64(), c->poff.u64(), run.n_contigs, c->vals[1].u32());
    run.have_gstart = true;
}

int uniform_sweep(qmcp_hip_ctx* c, const HeadFacts& h, bool* expand_left_out = nullptr) {
    const SolveRun& run = c->run;
    return launch_uniform_sweep(c, c->stream, (uint32_t)run.pr.n, (uint32_t)run.pr.ltot, run.n_contigs, h.max_span, run.M,
                                qmcp::words::sweep_iters(c->scalars.p), h.empty_positions, expand_left_out);
}

// The trivial route: no read, or no position.  The head has cleared the mask.
int trivial_route(qmcp_hip_ctx* c) {
    for (int i = EV_PREP; i <= EV_MARK; ++i) HIP_TRY(hipEventRecord(c->ev[i], c->stream));
    for (uint32_t i = 0; i <= qmcp::words::kHostEmptyPositions; ++i) c->h_scalars[i] = 0;
    c->pend_stats = c->run.local;
    c->pend_whole_contig_chains = 0;
    c->pending = true;
    return QMCP_OK;
}

// One span after a range-ranked head: the sweep from the head's own bucket offsets (the partition and the offsets are
// already queued).  *expand_left_out: as launch_uniform_sweep's.
int sweep_from_early_counts(qmcp_hip_ctx* c, const HeadFacts& h, bool* expand_left_out) {
    HIP_TRY(hipEventRecord(c->ev[EV_SCAN], c->stream));
    // (a pass-major head: k_pm_tables cleared the scalars on this stream, and nothing has touched them since)
    if (!c->run.pm) HIP_TRY(hipMemsetAsync(c->scalars.p, 0, qmcp::words::kScalarsBytes, c->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[EV_SORT], c->stream));
    TRY(uniform_sweep(c, h, expand_left_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[EV_SWEEP], c->stream));
    return QMCP_OK;
}

// The ranked one-span route.  Neither the sweep nor the keep mask needs a full sort: the head has partitioned {start,
// index} records by position range and counted per range; the sweep runs from those counts, and a per-range ordered
// ranking against S(p) writes the mask -- see "range-ranked uniform path" in the kernels.
int ranked_route(qmcp_hip_ctx* c, const HeadFacts& h) {
    // (the pass-major ranking can take its quotas from the event-driven sweep's own output: no expand, no selend[])
    bool expand_left_out = c->run.pm && !c->opt.keep_expand;
    TRY(sweep_from_early_counts(c, h, &expand_left_out));
    queue_rank(c, c->stream, expand_left_out ? c->cstart.u32() : nullptr, c->evlast.u32(), h.max_span);
    HIP_TRY(hipGetLastError());
    c->run.local.sort_passes = 1;  // one range partition, no sort
    return close_solve(c);
}

// The sorted one-span route: the reads sorted by start position, the mask from the sorted records.  A small call takes
// its bucket offsets from the sorted keys and sweeps then.  A call whose head ran ranked (after_ranked_head) but whose
// heaviest range holds too much for the ranking -- one wave's serial walk -- has its offsets from the head and its sweep
// from those, queued before the sort: the only case whose sweep is already done, and only the mask comes from the sort.
int sorted_route(qmcp_hip_ctx* c, const HeadFacts& h, bool after_ranked_head) {
    SolveRun& run = c->run;
    const uint32_t n = (uint32_t)run.pr.n, ltot = (uint32_t)run.pr.ltot;
    if (after_ranked_head) {
        TRY(sweep_from_early_counts(c, h, nullptr));
    } else {
        HIP_TRY(hipEventRecord(c->ev[EV_SCAN], c->stream));
        HIP_TRY(hipMemsetAsync(c->scalars.p, 0, qmcp::words::kScalarsBytes, c->stream));
    }
    SortedReads s = key_layout(ltot, h.max_span, h.max_span);
    run.local.sort_passes = s.passes;
    need_gstart(c);  // the key is the start position itself
    TRY(queue_sort(c, c->vals[1].u32(), n, s, {"k_radix_hist_rec", "scan_radix_hist(3 kernels)", "k_radix_scatter_rec"}, {}));
    if (!after_ranked_head) {
        TRY(queue_bucket_offsets(c, n, ltot, s));
        HIP_TRY(hipEventRecord(c->ev[EV_SORT], c->stream));
        TRY(uniform_sweep(c, h));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev[EV_SWEEP], c->stream));
    }
    queue_mark(c, ltot, s, run.d_mask);
    return close_solve(c);
}

// The near-uniform route (near_uniform_route.inc.hip).  done == false: it declined, nothing has touched the mask, and
// the caller takes the mixed route.
int near_uniform_route(qmcp_hip_ctx* c, const HeadFacts& h, bool& done) {
    HIP_TRY(hipMemsetAsync(c->scalars.p, 0, qmcp::words::kScalarsBytes, c->stream));
    TRY(near_uniform_tail(c, h.min_span, h.max_span, h.max_load, done));
    if (!done) return QMCP_OK;
    c->run.local.path = QMCP_PATH_NEAR_UNIFORM;
    c->run.local.sort_passes = 1;
    return close_solve(c);
}

// The mixed sweep for spans the LDS-cached walk takes: run lengths, then the register-resident walk (spans up to 448;
// speculative boundaries where the plan asks for them) or the cached one.  ax: the axis, under the exact table if any.
int mixed_sweep_cached(qmcp_hip_ctx* c, const HeadFacts& h, const SortedReads& s, qmcp::MixedSweepPlan plan,
                       const qmcp::SweepAxis& ax) {
    SolveRun& run = c->run;
    const uint32_t n = (uint32_t)run.pr.n, n_contigs = run.n_contigs, M = run.M;
    const uint32_t max_span = h.max_span;
    TRY(queue_run_lengths(c, n, s));
    if (plan.sample_span_mode) {
        uint32_t* d_share = c->stats.u32() + qmcp::words::kSpanSample;
        qmcp::launch_span_mode_share(c->stream, run.d_starts, run.d_ends, n, d_share);
        uint32_t share[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(share, d_share, sizeof(share), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        uint32_t longest = 0;
        for (uint32_t k = 0; k < n_contigs; ++k) longest = run.lengths[k] > longest ? run.lengths[k] : longest;
        plan = qmcp::refine_mixed_with_span_sample(c->opt, plan, share, longest);
    }
    const qmcp::SortedSpans reads{s.wide, c->keys[s.k].p, c->next_head.u32(), s.span_bits, max_span};
    const qmcp::SweepDemand demand{c->eoff.u32(), false};
    if (!plan.speculate) {
        uint32_t ring = 64;
        while (ring < max_span + 64) ring <<= 1;  // 64 buckets enter per chunk
        KernelSpan sp(c, plan.in_regs ? "k_sweep_general_reg" : "k_sweep_general_cached");
        if (!plan.in_regs || !qmcp::launch_sweep_general_reg(ax, reads, demand, M, c->selend.u32()))
            qmcp::launch_sweep_general_cached(ax, reads, demand.per_position, M, c->selend.u32(), ring);
        return QMCP_OK;
    }
    TRY(ensure(c, c->specsnap, qmcp::spec_snap_bytes(ax.n_seg_max)));
    TRY(speculative_sweep(
        c, ax, max_span, plan.round_to, plan.burn_blocks, plan.run_ins_apart, "k_sweep_general_reg",
        [&](const qmcp::SweepAxis& tier, uint32_t* out_odd, const uint32_t* redo_in) {
            return qmcp::launch_sweep_general_reg(tier, reads, demand, M, c->selend.u32(), out_odd, redo_in, c->specsnap.u32());
        },
        [&](const qmcp::SweepAxis& tier, uint32_t* mismatches, const uint32_t* redo_in, uint32_t* redo_out) {
            qmcp::launch_spec_verify_merge_mixed(tier, max_span, c->selend.u32(), c->cstart.u32(), c->specsnap.u32(),
                                                 mismatches, redo_in, redo_out);
        }));
    // stats.sweep_stretches: the first tier's table
    HIP_TRY(hipMemcpyAsync(qmcp::words::sweep_iters(c->scalars.p) + qmcp::words::kStretches,
                           c->segs.u32() + qmcp::sweep_segment_table_offset(n_contigs, ax.n_seg_max - n_contigs, 1),
                           sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    return QMCP_OK;
}

// The mixed sweep: cut points and speculative boundaries as sweep_plan.h plans them (a solve of this shape that
// speculated in vain is remembered), then the walk its longest span allows.  whole_contigs: no stretch table.
int mixed_sweep(qmcp_hip_ctx* c, const HeadFacts& h, const SortedReads& s, bool& whole_contigs) {
    SolveRun& run = c->run;
    const uint32_t n = (uint32_t)run.pr.n, ltot = (uint32_t)run.pr.ltot, n_contigs = run.n_contigs, M = run.M;
    // spans up to 448: the window of live buckets fits the wave's registers (8 per lane)
    const bool in_regs = h.max_span + 64 <= 512 && !c->opt.mixed_sweep_in_lds;
    const qmcp::MixedSweepPlan plan = qmcp::plan_mixed_sweep(c->opt, n, h.max_span, ltot, n_contigs, M, in_regs,
                                                             c->mem.spec_hopeless == Shape{run.n64, run.pr.ltot, M});
    qmcp::SweepAxis ax{c->stream, c->boff.u32(), c->poff.u64(), n_contigs, ltot};
    if (plan.windows != 0) {
        KernelSpan sp(c, "k_find_cuts");
        ax = qmcp::launch_sweep_segments(ax, c->eoff.u32(), h.max_span, M, plan.windows, c->segs.u32());
        // stats.sweep_stretches: the table's count (the uniform kernels count themselves)
        HIP_TRY(hipMemcpyAsync(qmcp::words::sweep_iters(c->scalars.p) + qmcp::words::kStretches, ax.seg, sizeof(uint32_t),
                               hipMemcpyDeviceToDevice, c->stream));
    }
    whole_contigs = ax.seg == nullptr;
    if (h.max_span <= qmcp::kMaxCachedSpan) return mixed_sweep_cached(c, h, s, plan, ax);
    Rings rings;
    TRY(sweep_rings(c, h.max_span, ax.workgroups(), rings));
    KernelSpan sp(c, "k_sweep_general");
    qmcp::launch_sweep_general(ax, {s.wide, c->keys[s.k].p, nullptr, s.span_bits, h.max_span}, {c->eoff.u32(), false}, M,
                               c->selend.u32(), rings.size, rings.global);
    return QMCP_OK;
}

// The mixed route: reads sorted by (start, span descending), bucket offsets from the sorted keys, the event-driven
// priority sweep, the mask from the sorted records.
int mixed_route(qmcp_hip_ctx* c, const HeadFacts& h) {
    SolveRun& run = c->run;
    const uint32_t n = (uint32_t)run.pr.n, ltot = (uint32_t)run.pr.ltot;
    need_gstart(c);
    SortedReads s = key_layout(ltot, h.min_span, h.max_span);
    TRY(queue_mixed_keys(c, run.d_starts, run.d_ends, n, ltot, h.max_span, s));
    HIP_TRY(hipEventRecord(c->ev[EV_SCAN], c->stream));
    HIP_TRY(hipMemsetAsync(c->scalars.p, 0, qmcp::words::kScalarsBytes, c->stream));
    run.local.sort_passes = s.passes;
    TRY(queue_sort(c, c->vals[0].u32(), n, s, {"k_radix_hist_rec", "scan_radix_hist(3 kernels)", "k_radix_scatter_rec"},
                   {"k_radix_hist", "scan_radix_hist(3 kernels)", "k_radix_scatter"}));
    TRY(queue_bucket_offsets(c, n, ltot, s));
    HIP_TRY(hipEventRecord(c->ev[EV_SORT], c->stream));
    bool whole_contigs = false;
    TRY(mixed_sweep(c, h, s, whole_contigs));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[EV_SWEEP], c->stream));
    queue_mark(c, ltot, s, run.d_mask);
    return close_solve(c, whole_contigs);
}

int enqueue_tail(qmcp_hip_ctx* c) {
    SolveRun& run = c->run;
    if (run.trivial) return trivial_route(c);
    HeadFacts h;
    TRY(read_head(c, h));
    if (h.uniform) {
        if (!run.may_rank) return sorted_route(c, h, false);
        if (run.nu_filter != 0 && run.nu_filter != h.max_span) TRY(head_again_unfiltered(c, h));
        // ranked while no range holds more than 1 / kRankBalance of the reads (force_sort_route: test hook)
        const bool ranked = (uint64_t)h.max_load * kRankBalance <= run.pr.n && !c->opt.force_sort_route;
        return ranked ? ranked_route(c, h) : sorted_route(c, h, true);
    }
    c->mixed_seen = true;
    if (h.max_span <= qmcp::kMaxUniformSpan) {
        bool done = false;
        TRY(near_uniform_route(c, h, done));
        if (done) return QMCP_OK;
    }
    return mixed_route(c, h);
}

int solve_enqueue(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint64_t* roff,
                  const uint32_t* lengths, uint32_t n_contigs, uint64_t n64, uint32_t M, uint64_t* d_mask);
int collect_one(qmcp_hip_ctx* c, qmcp_hip_stats* st) {
    namespace w = qmcp::words;
    if (!c->pending) return fail(QMCP_EINVAL, "no solve is pending on this context");
    c->pending = false;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->nu_deferred) {
        // the near-uniform route queued its rounds and the ranking unseen (near_uniform_tail): did they settle?
        c->nu_deferred = false;
        if (c->h_nu[w::kNuFlags] != 0 || c->h_nu[w::kNuSelectedLast] != 0) {
            // no: the call again, the blocking way (the head clears the mask; the contig tables are the context's copies)
            c->mem.nu_need_rounds = 0;
            const SolveRun r = c->run;
            const size_t count = (size_t)r.n_contigs + 1;
            std::vector<uint64_t> roff(c->h_tables.p, c->h_tables.p + count);
            std::vector<uint32_t> lengths(r.n_contigs);
            for (uint32_t k = 0; k < r.n_contigs; ++k) lengths[k] = (uint32_t)(c->h_tables[count + k + 1] - c->h_tables[count + k]);
            TRY(solve_enqueue(c, r.d_starts, r.d_ends, roff.data(), lengths.data(), r.n_contigs, r.n64, r.M, r.d_mask));
            return collect_one(c, st);
        }
        c->pend_stats.near_uniform_rounds = c->h_nu[w::kNuRoundsThatSelected] + 1;
        c->pend_stats.near_uniform_selected = c->h_nu[w::kNuSelected];
    }
    collect_spans(c);
#ifdef QMCP_EV_STAMP
    if (c->scalars.p) {
        uint32_t raw[16];
        HIP_TRY(hipMemcpy(raw, c->scalars.p, sizeof(raw), hipMemcpyDeviceToHost));
        const uint32_t* it = raw + w::kSweepItersAt / sizeof(uint32_t);
        fprintf(stderr, "[ev stamp] changed %u of %u blocks, stretches %u | x16 cycles: total %u general %u wait-for-ring %u slow-pieces %u (%u pieces) "
                        "failing rounds %u (%u rounds), blocks through the two scans %u\n",
                it[0], it[1], it[2], it[4], it[5], it[6], it[7], it[8], it[9], it[10], it[11]);
    }
#endif
    qmcp_hip_stats local = c->pend_stats;
    const unsigned long long* host_scalars = c->h_scalars;
    if (c->pend_spiky) {
        c->mem.spiky_empty = w::lo32(host_scalars[w::kHostEmptyPositions]);
        c->mem.spiky_known = true;
    }
    local.n_kept = host_scalars[w::kHostKept];
    c->last_iters = w::lo32(host_scalars[w::kHostIters]);
    c->last_blocks = w::hi32(host_scalars[w::kHostIters]);
    local.sweep_blocks_changed = c->last_iters;
    local.sweep_blocks = c->last_blocks;
    local.sweep_stretches = w::lo32(host_scalars[w::kHostStretches]) + c->pend_whole_contig_chains;
    local.spec_mismatches = w::lo32(host_scalars[w::kHostSpecTier1]);
    local.spec_boundaries = w::hi32(host_scalars[w::kHostSpecTier1]);
    local.spec_retry_mismatches = local.spec_mismatches ? w::lo32(host_scalars[w::kHostSpecTier2]) : 0u;
    if (local.path == QMCP_PATH_GENERAL && local.spec_boundaries >= 4 && 2u * local.spec_mismatches > local.spec_boundaries &&
        c->opt.speculation_run_in == 0) {
        // (three sweeps -- both tiers and the exact one -- where one would have done: 430 against 185 ms on cfg4's reads
        //  with 1 % clipped at 7.5 x M, lab/mixed_spec_check.py)
        c->mem.spec_hopeless = Shape{local.n_reads, local.total_length, c->pend_M};
    }
    phase_times(c, local);
    local.arena_grown_mid_solve = c->grew_mid_solve;
    if (st) *st = local;
    return QMCP_OK;
}

int solve_complete(qmcp_hip_ctx* c, qmcp_hip_stats* st) { return collect_one(c, st); }

// The environment's debug overrides of a new context's options -- the only place the library reads the environment.
void options_from_env(qmcp_hip_options& o) {
    auto num = [](const char* name) -> uint32_t { const char* e = std::getenv(name); return e ? (uint32_t)std::strtoul(e, nullptr, 10) : 0u; };
    auto flag = [](const char* name) -> int32_t { return std::getenv(name) != nullptr ? 1 : 0; };
    auto tri = [](const char* name) -> int32_t { const char* e = std::getenv(name); return !e ? 0 : e[0] == '1' ? 1 : e[0] == '0' ? -1 : 0; };
    o.pass_major = tri("QMCP_HIP_PM");
    if (const char* e = std::getenv("QMCP_HIP_SWEEP"))
        o.sweep = std::strcmp(e, "fast") == 0 ? QMCP_SWEEP_FAST : std::strcmp(e, "gen") == 0 ? QMCP_SWEEP_GENERAL
                  : std::strcmp(e, "ev") == 0 ? QMCP_SWEEP_EVENTS : QMCP_SWEEP_AUTO;
    o.cut_points = tri("QMCP_HIP_CUTS");
    o.speculation = tri("QMCP_HIP_SPEC");
    o.speculation_run_in = num("QMCP_HIP_SPEC_BURN");
    o.near_uniform = tri("QMCP_HIP_NEAR") < 0 ? -1 : 0;
    o.near_uniform_rounds = num("QMCP_HIP_NEAR_ROUNDS");
    if (const char* e = std::getenv("QMCP_HIP_NEAR_MIN_DEPTH")) o.near_uniform_min_depth = (float)std::strtod(e, nullptr);
    o.near_uniform_debug = flag("QMCP_HIP_NEAR_DEBUG");
    o.force_sort_route = flag("QMCP_HIP_NO_RANK");
    o.keep_expand = flag("QMCP_HIP_EXPAND");
    o.mixed_sweep_in_lds = flag("QMCP_HIP_GENERAL_LDS");
    o.rank_min_reads = num("QMCP_HIP_RANK_MIN");
    o.host_threads = num("QMCP_HIP_HOST_THREADS");
    o.copy_streams = num("QMCP_HIP_COPY_STREAMS");
    o.host_both_columns = flag("QMCP_HIP_HOST_BOTH_COLUMNS");
    if (const char* e = std::getenv("QMCP_HIP_PM_GRID")) o.pm_grid = e[0] == '-' ? -1 : e[0] == '1' || e[0] == '+' ? 1 : 0;
}

int create_ctx(int device, qmcp_hip_ctx** out_ctx) {
    if (!out_ctx) return fail(QMCP_EINVAL, "out_ctx is null");
    *out_ctx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(QMCP_ENODEVICE, "no HIP device available (quasi-mcp-hip has no CPU fallback)");
    }
    if (device < 0 || device >= n) return fail(QMCP_ENODEVICE, "device %d out of range [0,%d)", device, n);
    HIP_TRY(hipSetDevice(device));
    qmcp_hip_ctx* c = new (std::nothrow) qmcp_hip_ctx();
    if (!c) return fail(QMCP_ENOMEM, "host allocation failed");
    c->device = device;
    qmcp_hip_default_options(&c->opt);
    options_from_env(c->opt);
    hipError_t e = hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking);
    for (int i = 0; e == hipSuccess && i < EV_COUNT; ++i) e = hipEventCreate(&c->ev[i].h);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_in.h, hipEventDisableTiming);
    if (e == hipSuccess) {
        int lo = 0, hi = 0;  // numerically lower == higher priority
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        e = hipStreamCreateWithPriority(&c->stream2.h, hipStreamNonBlocking, hi);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork.h, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_head.h, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_done.h, hipEventDisableTiming);
    // (a half-built context is deleted like a whole one: what was not created is null and is skipped)
    int rc = e == hipSuccess ? ensure_pinned(c, c->h_head, qmcp::words::kHeadWords * sizeof(uint32_t))
                             : fail(QMCP_EHIP, "context setup: %s", hipGetErrorString(e));
    if (rc != QMCP_OK) {
        qmcp_hip_destroy(c);
        return rc;
    }
    c->h_stats_init = c->h_head + qmcp::words::kHeadStatsInit;
    c->h_stats_init[qmcp::words::kMinSpan] = 0xFFFFFFFFu;
    for (uint32_t i = 1; i < qmcp::words::kStatsInitWords; ++i) c->h_stats_init[i] = 0u;
    *out_ctx = c;
    return QMCP_OK;
}


// Everything of a solve up to and including its last launch; nothing here waits for the device
// except the small read-back that picks the route (span statistics, heaviest range), and that
// wait leaves the device free to work on whatever else is queued.  solve_complete collects.
int solve_enqueue(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                  const uint64_t* roff, const uint32_t* lengths, uint32_t n_contigs, uint64_t n64,
                  uint32_t M, uint64_t* d_mask) {
    if (c->pending) return fail(QMCP_EINVAL, "a solve is already pending on this context (call qmcp_hip_solve_end)");
    TRY(enqueue_head(c, d_starts, d_ends, roff, lengths, n_contigs, n64, M, d_mask));
    return enqueue_tail(c);
}

int solve_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                    const uint64_t* roff, const uint32_t* lengths, uint32_t n_contigs, uint64_t n64,
                    uint32_t M, uint64_t* d_mask, qmcp_hip_stats* st) {
    TRY(solve_enqueue(c, d_starts, d_ends, roff, lengths, n_contigs, n64, M, d_mask));
    return solve_complete(c, st);
}

int use_device(qmcp_hip_ctx* c, bool may_be_pending = false) {
    if (!c) return fail(QMCP_EINVAL, "null context");
    if (c->pending && !may_be_pending)
        return fail(QMCP_EINVAL, "a solve is pending on this context (call qmcp_hip_solve_end first)");
    HIP_TRY(hipSetDevice(c->device));
    return QMCP_OK;
}

// Order the solver stream after the caller's producer stream (NULL = the default stream:
// the solver stream is non-blocking, so even that needs an explicit edge).
int order_after(qmcp_hip_ctx* c, void* user_stream) {
    if ((hipStream_t)user_stream != c->stream) {
        HIP_TRY(hipEventRecord(c->ev_in, (hipStream_t)user_stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_in, 0));
    }
    return QMCP_OK;
}
