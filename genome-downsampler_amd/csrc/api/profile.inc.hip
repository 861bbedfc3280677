// profile.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_profile_host / _device: a cap per region, need(p) = min(cov(p), cap(p)).  The call is the by-contig flow
// (api/by_contig.inc.hip: group_by_contig, run_batches, the final wait) with ProfileSolver as the batch solver, which solves
// every batch under its own regions:
//   1. cap_table.h builds the table on the host (a bad table fails here, before anything is copied or launched)
//   2. a batch without a region is the unchanged solve at default_cap (a call without regions is therefore exactly
//      qmcp_hip_solve_by_contig_* at default_cap); a batch whose largest cap is 0 keeps nothing
//   3. any other batch takes the sort-based mixed-span route whatever its spans (span_bits == 0 is legal):
//      k_prepare -> k_general_keys + ecnt scan -> radix -> bucket heads -> k_profile_need -> [k_profile_cuts +
//      k_build_segments] -> capped sweep -> k_mark.  Windows as plan_mixed_sweep chooses them for M = the batch's largest
//      cap, exact cuts only.  One blocking round trip after k_prepare (span statistics, validation) and one at the end
//      (kept count, stretches), as the mixed route of the plain solve has.
// Buffers: the solve's own arena for everything the plain mixed route uses; need[] in pf_need, the batch's regions in
// pf_tab, the two counters in pf_stat.
// Step 3 is capped_solve_batch, which takes what builds need[] as a CappedNeed: the region table here (ProfileNeed), the
// credit of the reads already kept in api/pairs.inc.hip, the dual need of a ceiling in api/ceiling.inc.hip (a batch solver
// of its own over the same ProfileRun).
namespace {

struct ProfileRun {
    const qmcp::CapTable* tab = nullptr;
    uint32_t default_cap = 0;
    float ms_profile = 0.f;
    std::vector<uint32_t> gs, ge, gcap;  // the batch's regions in its global positions
};

// What builds need[] for capped_solve_batch: a profile's regions here, the credit of the reads already kept in
// api/pairs.inc.hip.  reserve runs inside the solve's arena block, upload behind the contig tables, launch once boff and
// eoff exist; no_demand may look at what launch counted (a blocking read-back) and report that nothing is asked for.
struct CappedNeed {
    float ms = 0.f;  // device time of launch (+ the cut-point scan), summed over the batches
    virtual ~CappedNeed() {}
    virtual const char* name() const = 0;
    virtual DevBuf& need_buf(qmcp_hip_ctx* c) = 0;
    virtual int reserve(qmcp_hip_ctx* c) = 0;
    virtual int upload(qmcp_hip_ctx* c, hipStream_t st) = 0;
    virtual void launch(qmcp_hip_ctx* c, hipStream_t st, uint32_t ltot, uint32_t* need) = 0;
    virtual int no_demand(qmcp_hip_ctx*, hipStream_t, bool* none) {
        *none = false;
        return QMCP_OK;
    }
    // the cap that chooses the sweep's windows, asked for after no_demand: the caller's max_cap, unless the largest demand
    // is only known once launch has counted it
    virtual uint32_t plan_cap(uint32_t max_cap) const { return max_cap; }
};

// One batch on the sort-based mixed-span route under need[] (steps 3 of the header above); max_cap > 0 is the largest
// cap the batch can meet, which chooses the windows (through nd.plan_cap, once need[] is built).  *swept (may be NULL):
// a sweep was queued.
int capped_solve_batch(qmcp_hip_ctx* c, CappedNeed& nd, uint32_t max_cap, const uint32_t* d_starts, const uint32_t* d_ends,
                       const uint64_t* roff, const uint32_t* lengths, uint32_t n_contigs, uint64_t n64, uint64_t* d_mask,
                       qmcp_hip_stats* st_out, bool* swept_out = nullptr) {
    if (swept_out) *swept_out = false;
    if (c->pending) return fail(QMCP_EINVAL, "a solve is already pending on this context (call qmcp_hip_solve_end)");
    Problem pr;
    TRY(check_problem(roff, lengths, n_contigs, n64, pr));
    const uint32_t n = (uint32_t)pr.n, ltot = (uint32_t)pr.ltot;
    const size_t mask_words = (size_t)((n64 + 63) / 64);
    hipStream_t st = c->stream;
    qmcp_hip_stats local;
    std::memset(&local, 0, sizeof(local));
    local.n_reads = n64;
    local.n_contigs = n_contigs;
    local.total_length = pr.ltot;
    local.path = QMCP_PATH_GENERAL;
    if (mask_words) HIP_TRY(hipMemsetAsync(d_mask, 0, mask_words * sizeof(uint64_t), st));
    if (n == 0 || ltot == 0 || max_cap == 0) {  // (reads on zero-length contigs were refused by k_bc_keys)
        if (st_out) *st_out = local;
        return QMCP_OK;
    }
    TRY(ensure_pinned(c, c->h_scalars, qmcp::words::kHostScalarsWords * sizeof(unsigned long long)));
    // the arena, sized before anything is queued
    const uint32_t n_tiles = qmcp::sort_tiles(n);
    c->sized = false;
    {
        TRY(ensure(c, c->spine, std::max(scan_spine_bytes(256u * n_tiles), scan_spine_bytes(std::max(ltot, n) + 1, 1))));
        TRY(ensure(c, c->hist, (size_t)256 * std::max(qmcp::seg_tile_bound(n), n_tiles) * sizeof(uint32_t)));
        TRY(ensure(c, c->keys[0], (size_t)n * sizeof(uint64_t)));
        TRY(ensure(c, c->keys[1], (size_t)n * sizeof(uint64_t)));
        TRY(ensure(c, c->vals[0], (size_t)n * sizeof(uint32_t)));
        TRY(ensure(c, c->vals[1], (size_t)n * sizeof(uint32_t)));
        TRY(ensure(c, c->boff, ((size_t)ltot + 1) * sizeof(uint32_t)));
        TRY(ensure(c, c->ecnt, ((size_t)ltot + 1) * sizeof(uint32_t)));
        TRY(ensure(c, c->eoff, ((size_t)ltot + 1) * sizeof(uint32_t)));
        TRY(ensure(c, c->selend, ((size_t)ltot + 8) * sizeof(uint32_t)));
        TRY(ensure(c, c->next_head, ((size_t)n + 2) * sizeof(uint32_t)));
        TRY(ensure(c, c->scalars, qmcp::words::kScalarsBytes));
        TRY(ensure(c, c->stats, qmcp::words::kStatsWords * sizeof(uint32_t)));
        TRY(ensure(c, c->segs, qmcp::sweep_segment_words(n_contigs < 256 ? n_contigs : 0, qmcp::kMaxSweepWindows) * sizeof(uint32_t)));
        TRY(ensure(c, nd.need_buf(c), ((size_t)ltot + 8) * sizeof(uint32_t)));
        TRY(nd.reserve(c));
    }
    c->grew_mid_solve = 0;
    c->mixed_seen = true;
    HIP_TRY(hipEventRecord(c->ev[EV_BEGIN], st));
    TRY(upload_tables(c, roff, pr));
    c->sized = true;
    TRY(nd.upload(c, st));
    // span statistics, validation, global start positions (vals[1]): the one read-back that shapes the keys
    uint32_t hs[3];
    TRY(run_prepare(c, d_starts, d_ends, pr, nullptr, true, false, false, 0, nullptr, hs));
    HIP_TRY(hipEventRecord(c->ev[EV_PREP], st));
    const uint32_t min_span = hs[0], max_span = hs[1];
    local.min_span = min_span;
    local.max_span = max_span;
    if (max_span > qmcp::kMaxGeneralSpan)
        return fail(QMCP_ERANGE, "reads with span %u > %u are not supported by this build", max_span, qmcp::kMaxGeneralSpan);
    // the plain solve's mixed route up to the bucket offsets (solve_stages.inc.hip), under this route's span names
    SortedReads s = key_layout(ltot, min_span, max_span);
    TRY(queue_mixed_keys(c, d_starts, d_ends, n, ltot, max_span, s));
    HIP_TRY(hipEventRecord(c->ev[EV_SCAN], st));
    HIP_TRY(hipMemsetAsync(c->scalars.p, 0, qmcp::words::kScalarsBytes, st));
    local.sort_passes = s.passes;
    const RadixNames radix_names = {"radix pass (hist, scan, scatter)"};
    TRY(queue_sort(c, c->vals[0].u32(), n, s, radix_names, radix_names));
    TRY(queue_bucket_offsets(c, n, ltot, s));
    HIP_TRY(hipEventRecord(c->ev[EV_SORT], st));
    // need[], cut points
    const uint32_t* d_need = nd.need_buf(c).u32();
    const bool in_regs = max_span + 64 <= 512 && !c->opt.mixed_sweep_in_lds;
    qmcp::SweepAxis ax{st, c->boff.u32(), c->poff.u64(), n_contigs, ltot};
    EventPair ev_pf(c);
    if (!ev_pf.a || !ev_pf.b) return fail(QMCP_EHIP, "event creation failed");
    HIP_TRY(hipEventRecord(ev_pf.a, st));
    {
        KernelSpan sp(c, nd.name());
        nd.launch(c, st, ltot, nd.need_buf(c).u32());
    }
    bool idle = false;  // nothing is asked for anywhere: no sweep, the zeroed mask stands
    TRY(nd.no_demand(c, st, &idle));
    const uint32_t windows =
        qmcp::plan_mixed_sweep(c->opt, n, max_span, ltot, n_contigs, nd.plan_cap(max_cap), in_regs, false).windows;
    if (windows != 0 && !idle) {
        KernelSpan sp(c, "k_profile_cuts");
        ax = qmcp::launch_profile_segments(ax, d_need, windows, c->segs.u32());
        HIP_TRY(hipMemcpyAsync(qmcp::words::sweep_iters(c->scalars.p) + qmcp::words::kStretches, ax.seg, sizeof(uint32_t),
                               hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipEventRecord(ev_pf.b, st));
    HIP_TRY(hipGetLastError());
    // the capped sweep
    bool swept = idle;
    const qmcp::SortedSpans reads{s.wide, c->keys[s.k].p, c->next_head.u32(), s.span_bits, max_span};
    const qmcp::SweepDemand demand{d_need, true};
    if (in_regs && !idle) {
        TRY(queue_run_lengths(c, n, s));
        KernelSpan sp(c, "k_sweep_general_reg(capped)");
        swept = qmcp::launch_sweep_general_reg(ax, reads, demand, 0, c->selend.u32());
    }
    if (!swept) {
        Rings rings;
        TRY(sweep_rings(c, max_span, ax.workgroups(), rings));
        KernelSpan sp(c, "k_sweep_general(capped)");
        qmcp::launch_sweep_general(ax, reads, demand, 0, c->selend.u32(), rings.size, rings.global);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[EV_SWEEP], st));
    if (!idle) queue_mark(c, ltot, s, d_mask);
    TRY(queue_result_scalars(c));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    local.n_kept = c->h_scalars[qmcp::words::kHostKept];
    local.sweep_stretches = qmcp::words::lo32(c->h_scalars[qmcp::words::kHostStretches]);
    if (ax.seg == nullptr && !idle) local.sweep_stretches += whole_contig_chains(lengths, n_contigs);
    phase_times(c, local);
    local.arena_grown_mid_solve = c->grew_mid_solve;
    nd.ms += elapsed(ev_pf.a, ev_pf.b);
    if (swept_out) *swept_out = !idle;
    if (st_out) *st_out = local;
    return QMCP_OK;
}

// a profile's need[]: the batch's regions (pf_tab: starts | ends | caps) through k_profile_need
struct ProfileNeed : CappedNeed {
    ProfileRun& pf;
    uint32_t n_reg;
    ProfileNeed(ProfileRun& run, uint32_t regions) : pf(run), n_reg(regions) {}
    const char* name() const override { return "k_profile_need"; }
    DevBuf& need_buf(qmcp_hip_ctx* c) override { return c->pf_need; }
    int reserve(qmcp_hip_ctx* c) override { return ensure(c, c->pf_tab, 3 * (size_t)n_reg * sizeof(uint32_t) + 16); }
    int upload(qmcp_hip_ctx* c, hipStream_t st) override {
        uint32_t* d_rs = c->pf_tab.u32();
        if (n_reg) {
            HIP_TRY(hipMemcpyAsync(d_rs, pf.gs.data(), (size_t)n_reg * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_rs + n_reg, pf.ge.data(), (size_t)n_reg * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_rs + 2 * (size_t)n_reg, pf.gcap.data(), (size_t)n_reg * 4, hipMemcpyHostToDevice, st));
        }
        return QMCP_OK;
    }
    void launch(qmcp_hip_ctx* c, hipStream_t st, uint32_t ltot, uint32_t* need) override {
        const uint32_t* d_rs = c->pf_tab.u32();
        qmcp::launch_profile_need(st, c->boff.u32(), c->eoff.u32(), ltot, d_rs, d_rs + n_reg,
                                  d_rs + 2 * (size_t)n_reg, n_reg, pf.default_cap, need, c->pf_stat.as<unsigned long long>());
    }
};

// a batch under its own regions' caps: the plain solve at default_cap where it has none, else the capped route
struct ProfileSolver : BatchSolver {
    ProfileRun& pf;
    explicit ProfileSolver(ProfileRun& run) : pf(run) {}
    int solve(qmcp_hip_ctx* c, BatchView& v, qmcp_hip_stats* bs) override {
        const qmcp::CapTable& tab = *pf.tab;
        const uint32_t r0 = tab.offs[v.first_contig], r1 = tab.offs[v.first_contig + v.n_contigs];
        uint32_t max_cap = pf.default_cap;
        for (uint32_t k = r0; k < r1; ++k) max_cap = std::max(max_cap, tab.cap[k]);
        if (r0 == r1 && max_cap != 0) return PlainSolver(pf.default_cap).solve(c, v, bs);
        qmcp::batch_cap_table(tab, v.lengths - v.first_contig, v.first_contig, v.n_contigs, pf.gs, pf.ge, pf.gcap);
        ProfileNeed nd(pf, r1 - r0);
        TRY(capped_solve_batch(c, nd, max_cap, c->bc_starts.u32(), c->bc_ends.u32(), v.roff.data(),
                               v.lengths, v.n_contigs, v.nb, c->bc_mask.u64(), bs));
        pf.ms_profile += nd.ms;
        return QMCP_OK;
    }
};

// the checks both entries make before anything is copied or launched, and the table
int check_profile_call(uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, const uint32_t* region_offsets,
                       const uint32_t* region_starts, const uint32_t* region_ends, const uint32_t* region_caps,
                       uint32_t default_cap, uint32_t flags, qmcp::CapTable& tab) {
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    if (!contig_lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    if (flags != 0) return fail(QMCP_EINVAL, "unknown flag bits 0x%x", flags);
    const int rc = qmcp::build_cap_table(region_offsets, region_starts, region_ends, region_caps, contig_lengths, n_contigs, tab);
    if (rc == QMCP_ERANGE) return fail(QMCP_ERANGE, "a region's cap is 2^31 or more");
    if (rc != QMCP_OK)
        return fail(QMCP_EINVAL, "region table: offsets must start at 0 and never decrease, arrays must not be null, every "
                                 "region needs start <= end, and the regions of one contig must be disjoint after clipping");
    if (default_cap >= qmcp::kCapLimit) return fail(QMCP_ERANGE, "default_cap %u is 2^31 or more", default_cap);
    return QMCP_OK;
}

int solve_profile_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                            uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, const qmcp::CapTable& tab,
                            uint32_t default_cap, uint64_t* d_mask, qmcp_hip_stats* stats, qmcp_hip_profile_stats* pstats) {
    qmcp_hip_profile_stats ps;
    std::memset(&ps, 0, sizeof(ps));
    ps.regions_in = tab.regions_in;
    ps.regions_used = tab.regions_used;
    ps.positions_in_regions = tab.positions;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (pstats) *pstats = ps;
    if (tab.regions_used == 0 && default_cap != 0)  // the fast path: the plain by-contig call
        return solve_by_contig_on_device(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, default_cap, d_mask, stats);
    TRY(ensure(c, c->pf_stat, 2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->pf_stat.p, 0, 2 * sizeof(unsigned long long), c->stream));
    ProfileRun pf;
    pf.tab = &tab;
    pf.default_cap = default_cap;
    GroupedReads g;
    TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, d_mask, g));
    ProfileSolver capped(pf);
    qmcp_hip_stats sum;
    TRY(run_batches(c, g, capped, d_mask, sum));
    HIP_TRY(hipStreamSynchronize(c->stream));
    collect_spans(c);
    if (stats) *stats = sum;
    unsigned long long counters[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(counters, c->pf_stat.p, sizeof(counters), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ps.capped_positions = counters[0];
    ps.demand = counters[1];
    ps.ms_profile = pf.ms_profile;
    if (pstats) *pstats = ps;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_profile_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                const uint32_t* region_offsets, const uint32_t* region_starts, const uint32_t* region_ends,
                                const uint32_t* region_caps, uint32_t default_cap, uint32_t flags, uint64_t* keep_mask_out,
                                qmcp_hip_stats* stats, qmcp_hip_profile_stats* pstats) {
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    qmcp::CapTable tab;
    TRY(check_profile_call(n_reads, contig_lengths, n_contigs, region_offsets, region_starts, region_ends, region_caps,
                           default_cap, flags, tab));
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
    TRY(solve_profile_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), n_reads, contig_lengths,
        n_contigs, tab, default_cap, c->mask.u64(), stats, pstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_profile_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                  const uint32_t* d_contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                  uint32_t n_contigs, const uint32_t* region_offsets, const uint32_t* region_starts,
                                  const uint32_t* region_ends, const uint32_t* region_caps, uint32_t default_cap,
                                  uint32_t flags, uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                  qmcp_hip_profile_stats* pstats) {
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    qmcp::CapTable tab;
    TRY(check_profile_call(n_reads, contig_lengths, n_contigs, region_offsets, region_starts, region_ends, region_caps,
                           default_cap, flags, tab));
    TRY(order_after(c, hip_stream));
    return solve_profile_on_device(c, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, n_contigs, tab, default_cap,
                                   d_keep_mask_out, stats, pstats);
}

}  // extern "C"
