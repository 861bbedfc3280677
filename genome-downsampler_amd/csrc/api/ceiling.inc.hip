// ceiling.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_ceiling_host / _device: kept(p) <= cap(p) everywhere with the most reads kept.  kept <= cap is dropped >=
// cov - cap, and keeping the most is dropping the fewest: the dropped set D is the canonical selection under need(p) =
// max(0, cov(p) - cap(p)), and need <= cov, so the greedy never runs dry.  The call is the profile's flow (group_by_contig,
// run_batches, the cap table and capped_solve_batch of api/profile.inc.hip) with CeilingSolver as the batch solver:
//   1. per batch, k_ceiling_need as the CappedNeed: the dual need, its cut bit where need(p) == cov(p), and the largest
//      need, which is what plans the sweep (CeilingNeed::plan_cap) -- a batch that is nowhere above its caps queues none
//   2. per batch, once k_mark has written D in grouped order: k_pair_credit_events + scan give depth_D(p), k_ceiling_check
//      holds cov - depth_D against the caps; the batch loop then ORs D into input order
//   3. once, k_ceiling_finish over the input-order mask: keep = placed & ~D, mates joined to D first under
//      QMCP_CEILING_WHOLE_PAIRS
// Buffers: the profile's pf_need / pf_tab, and cl_* (a batch's position offsets, depth_D and its spine, the counters).
namespace {

// need[] of the dropped set: the batch's regions as ProfileNeed uploads them, through k_ceiling_need
struct CeilingNeed : ProfileNeed {
    unsigned long long largest = 0;  // this batch's largest need
    CeilingNeed(ProfileRun& run, uint32_t regions) : ProfileNeed(run, regions) {}
    const char* name() const override { return "k_ceiling_need"; }
    int upload(qmcp_hip_ctx* c, hipStream_t st) override {
        HIP_TRY(hipMemsetAsync(c->cl_stat.as<unsigned long long>() + qmcp::kCeilMaxNeed, 0, sizeof(unsigned long long), st));
        return ProfileNeed::upload(c, st);
    }
    void launch(qmcp_hip_ctx* c, hipStream_t st, uint32_t ltot, uint32_t* need) override {
        const uint32_t* d_rs = c->pf_tab.u32();
        qmcp::launch_ceiling_need(st, c->boff.u32(), c->eoff.u32(), ltot, d_rs, d_rs + n_reg,
                                  d_rs + 2 * (size_t)n_reg, n_reg, pf.default_cap, need, c->cl_stat.as<unsigned long long>());
    }
    int no_demand(qmcp_hip_ctx* c, hipStream_t st, bool* none) override {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&largest, c->cl_stat.as<unsigned long long>() + qmcp::kCeilMaxNeed, sizeof(largest),
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *none = largest == 0;
        return QMCP_OK;
    }
    // under a ceiling the demand is cov - cap, not the cap (a cap of 0 is the FULL demand)
    uint32_t plan_cap(uint32_t) const override { return std::max((uint32_t)largest, 1u); }
};

// a batch's dropped set D into the batch mask, and the kept depth held against the caps
struct CeilingSolver : BatchSolver {
    ProfileRun& pf;
    float ms_check = 0.f;
    explicit CeilingSolver(ProfileRun& run) : pf(run) {}
    int solve(qmcp_hip_ctx* c, BatchView& v, qmcp_hip_stats* bs) override;
};

int CeilingSolver::solve(qmcp_hip_ctx* c, BatchView& v, qmcp_hip_stats* st_out) {
    const qmcp::CapTable& tab = *pf.tab;
    const uint32_t first_contig = v.first_contig, n_contigs = v.n_contigs, nb = v.nb;
    const uint32_t* d_starts = c->bc_starts.u32();
    const uint32_t* d_ends = c->bc_ends.u32();
    uint64_t* d_mask = c->bc_mask.u64();
    hipStream_t st = c->stream;
    qmcp::batch_cap_table(tab, v.lengths - first_contig, first_contig, n_contigs, pf.gs, pf.ge, pf.gcap);
    CeilingNeed nd(pf, tab.offs[first_contig + n_contigs] - tab.offs[first_contig]);
    bool swept = false;
    // (max_cap only short-circuits at 0 here: the windows come from CeilingNeed::plan_cap)
    TRY(capped_solve_batch(c, nd, 1u, d_starts, d_ends, v.roff.data(), v.lengths, n_contigs, nb, d_mask, st_out, &swept));
    pf.ms_profile += nd.ms;
    v.tables32();
    const uint32_t ltot = v.poff32[n_contigs];
    if (nb == 0 || ltot == 0) return QMCP_OK;
    // the depth of D on the batch's axis, and the kept depth against the caps: boff, eoff and pf_tab are the solve's
    const uint32_t pad = qmcp::pair_credit_pad();
    TRY(ensure(c, c->cl_depth, ((size_t)ltot + pad + 4) * sizeof(uint32_t)));
    TRY(ensure(c, c->cl_spine, scan_spine_bytes(ltot + pad, 1)));
    TRY(ensure(c, c->cl_poff, ((size_t)n_contigs + 1) * sizeof(uint32_t)));
    EventPair ev(c);
    if (!ev.a || !ev.b) return fail(QMCP_EHIP, "event creation failed");
    HIP_TRY(hipEventRecord(ev.a, st));
    HIP_TRY(hipMemsetAsync(c->cl_depth.p, 0, ((size_t)ltot + pad + 4) * sizeof(uint32_t), st));
    if (swept) {  // (no sweep: D is empty, the zeroed depth stands)
        HIP_TRY(hipMemcpyAsync(c->cl_poff.p, v.poff32.data(), ((size_t)n_contigs + 1) * sizeof(uint32_t),
                               hipMemcpyHostToDevice, st));
        KernelSpan sp(c, "k_pair_credit_events + scan(ceiling)");
        qmcp::launch_pair_credit_events(st, v.records, nb, d_mask, d_starts, d_ends, c->cl_poff.u32(), first_contig,
                                        c->cl_depth.u32());
        qmcp::launch_exclusive_scan(st, c->cl_depth.u32(), ltot + pad, c->cl_depth.u32(), c->cl_spine.u32(), false);
    }
    {
        KernelSpan sp(c, "k_ceiling_check");
        const uint32_t* d_rs = c->pf_tab.u32();
        qmcp::launch_ceiling_check(st, c->boff.u32(), c->eoff.u32(),
                                   c->cl_depth.u32() + pad, ltot, d_rs, d_rs + nd.n_reg,
                                   d_rs + 2 * (size_t)nd.n_reg, nd.n_reg, pf.default_cap, c->cl_stat.as<unsigned long long>());
    }
    HIP_TRY(hipEventRecord(ev.b, st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));  // (the copy of poff32 is done, the time can be read)
    ms_check += elapsed(ev.a, ev.b);
    return QMCP_OK;
}

// the checks both entries make before anything is copied or launched, and the table
int check_ceiling_call(uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, const uint32_t* region_offsets,
                       const uint32_t* region_starts, const uint32_t* region_ends, const uint32_t* region_caps,
                       uint32_t default_cap, uint32_t flags, qmcp::CapTable& tab) {
    if (flags & ~QMCP_CEILING_WHOLE_PAIRS) return fail(QMCP_EINVAL, "unknown flag bits 0x%x", flags & ~QMCP_CEILING_WHOLE_PAIRS);
    if ((flags & QMCP_CEILING_WHOLE_PAIRS) && (n_reads & 1ull))
        return fail(QMCP_EINVAL, "n_reads %llu is odd: reads (2q, 2q + 1) are pair q", (unsigned long long)n_reads);
    return check_profile_call(n_reads, contig_lengths, n_contigs, region_offsets, region_starts, region_ends, region_caps,
                              default_cap, 0u, tab);
}

int solve_ceiling_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                            uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, const qmcp::CapTable& tab,
                            uint32_t default_cap, uint32_t flags, uint64_t* d_mask, qmcp_hip_stats* stats,
                            qmcp_hip_ceiling_stats* cstats) {
    qmcp_hip_ceiling_stats cs;
    std::memset(&cs, 0, sizeof(cs));
    cs.regions_in = tab.regions_in;
    cs.regions_used = tab.regions_used;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (cstats) *cstats = cs;
    hipStream_t st = c->stream;
    TRY(ensure(c, c->cl_stat, qmcp::kCeilingStatWords * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->cl_stat.p, 0, qmcp::kCeilingStatWords * sizeof(unsigned long long), st));
    ProfileRun pf;
    pf.tab = &tab;
    pf.default_cap = default_cap;
    // the batch loop leaves d_mask holding D in input order
    GroupedReads g;
    TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, d_mask, g));
    CeilingSolver dropped(pf);
    qmcp_hip_stats sum;
    TRY(run_batches(c, g, dropped, d_mask, sum));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    if (stats) *stats = sum;
    EventPair ev(c);
    if (!ev.a || !ev.b) return fail(QMCP_EHIP, "event creation failed");
    HIP_TRY(hipEventRecord(ev.a, st));
    {
        KernelSpan sp(c, "k_ceiling_finish");
        qmcp::launch_ceiling_finish(st, d_ids, n64, (flags & QMCP_CEILING_WHOLE_PAIRS) != 0, d_mask,
                                    c->cl_stat.as<unsigned long long>());
    }
    HIP_TRY(hipEventRecord(ev.b, st));
    HIP_TRY(hipGetLastError());
    unsigned long long w[qmcp::kCeilingStatWords];
    HIP_TRY(hipMemcpyAsync(w, c->cl_stat.p, sizeof(w), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    cs.reads_placed = w[qmcp::kCeilPlaced];
    cs.reads_dropped = w[qmcp::kCeilPlaced] - w[qmcp::kCeilKept];
    cs.mates_dropped = w[qmcp::kCeilMatesDropped];
    cs.over_positions = w[qmcp::kCeilOverPositions];
    cs.over_bases = w[qmcp::kCeilOverBases];
    cs.short_positions = w[qmcp::kCeilShortPositions];
    cs.short_bases = w[qmcp::kCeilShortBases];
    cs.excess_positions = w[qmcp::kCeilExcessPositions];
    cs.max_kept_depth = (uint32_t)w[qmcp::kCeilMaxKept];
    cs.ms_ceiling = pf.ms_profile + dropped.ms_check + elapsed(ev.a, ev.b);
    if (cstats) *cstats = cs;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_ceiling_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                const uint32_t* region_offsets, const uint32_t* region_starts, const uint32_t* region_ends,
                                const uint32_t* region_caps, uint32_t default_cap, uint32_t flags, uint64_t* keep_mask_out,
                                qmcp_hip_stats* stats, qmcp_hip_ceiling_stats* cstats) {
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    qmcp::CapTable tab;
    TRY(check_ceiling_call(n_reads, contig_lengths, n_contigs, region_offsets, region_starts, region_ends, region_caps,
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
    TRY(solve_ceiling_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), n_reads, contig_lengths,
        n_contigs, tab, default_cap, flags, c->mask.u64(), stats, cstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_ceiling_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                  const uint32_t* d_contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                  uint32_t n_contigs, const uint32_t* region_offsets, const uint32_t* region_starts,
                                  const uint32_t* region_ends, const uint32_t* region_caps, uint32_t default_cap,
                                  uint32_t flags, uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                  qmcp_hip_ceiling_stats* cstats) {
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    qmcp::CapTable tab;
    TRY(check_ceiling_call(n_reads, contig_lengths, n_contigs, region_offsets, region_starts, region_ends, region_caps,
                           default_cap, flags, tab));
    TRY(order_after(c, hip_stream));
    return solve_ceiling_on_device(c, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, n_contigs, tab, default_cap,
                                   flags, d_keep_mask_out, stats, cstats);
}

}  // extern "C"
