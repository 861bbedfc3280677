// proportional.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_proportional_host / _device: keep a fraction of the depth everywhere,
//   q(p) = ceil(cov(p) * num / den),   need(p) = min(cov(p), max_coverage, max(q(p), floor)).
// need <= cov, so the call is the profile's flow (group_by_contig, run_batches and capped_solve_batch of
// api/profile.inc.hip) with ProportionalSolver as the batch solver and no table at all:
//   1. the two ends of the parameter range are the plain by-contig call: num == den or floor >= max_coverage asks for
//      min(cov, max_coverage), num == 0 for min(cov, floor, max_coverage); a cap of 0 stops behind the grouping (the
//      reads are validated, the cleared mask stands)
//   2. otherwise, per batch, k_prop_need as the CappedNeed: need[], its cut bit where need(p) == cov(p), the counters,
//      and the largest need, which is what plans the sweep (ProportionalNeed::plan_cap, as CeilingNeed does) -- a batch
//      that asks for nothing queues none
//   3. once, on every route, k_prop_tally over the input-order columns and the final mask
// Buffers: the profile's pf_need, and the PropStat words in pp_stat.
namespace {

struct ProportionalRun {
    uint32_t num = 0, den = 1, floor = 0, max_coverage = 0;
    uint32_t max_depth = 0, max_need = 0;  // over the batches
    float ms_need = 0.f;
};

// need[] from the batch's own depth, through k_prop_need
struct ProportionalNeed : CappedNeed {
    ProportionalRun& pp;
    unsigned long long maxima[2] = {0, 0};  // this batch's largest depth and largest need
    explicit ProportionalNeed(ProportionalRun& run) : pp(run) {}
    const char* name() const override { return "k_prop_need"; }
    DevBuf& need_buf(qmcp_hip_ctx* c) override { return c->pf_need; }
    int reserve(qmcp_hip_ctx*) override { return QMCP_OK; }
    int upload(qmcp_hip_ctx* c, hipStream_t st) override {
        static_assert(qmcp::kPropMaxNeed == qmcp::kPropMaxDepth + 1, "the two maxima are cleared and read as one block");
        HIP_TRY(hipMemsetAsync(c->pp_stat.as<unsigned long long>() + qmcp::kPropMaxDepth, 0, sizeof(maxima), st));
        return QMCP_OK;
    }
    void launch(qmcp_hip_ctx* c, hipStream_t st, uint32_t ltot, uint32_t* need) override {
        qmcp::launch_prop_need(st, c->boff.u32(), c->eoff.u32(), ltot, pp.num, pp.den, pp.floor, pp.max_coverage, need,
                               c->pp_stat.as<unsigned long long>());
    }
    int no_demand(qmcp_hip_ctx* c, hipStream_t st, bool* none) override {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(maxima, c->pp_stat.as<unsigned long long>() + qmcp::kPropMaxDepth, sizeof(maxima),
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *none = maxima[1] == 0;
        return QMCP_OK;
    }
    // the windows follow the largest demand the data makes, not max_coverage (which may be "none")
    uint32_t plan_cap(uint32_t) const override { return std::max((uint32_t)maxima[1], 1u); }
};

struct ProportionalSolver : BatchSolver {
    ProportionalRun& pp;
    explicit ProportionalSolver(ProportionalRun& run) : pp(run) {}
    int solve(qmcp_hip_ctx* c, BatchView& v, qmcp_hip_stats* bs) override {
        ProportionalNeed nd(pp);
        // (max_cap only short-circuits at 0 here: the windows come from ProportionalNeed::plan_cap)
        TRY(capped_solve_batch(c, nd, 1u, c->bc_starts.u32(), c->bc_ends.u32(), v.roff.data(), v.lengths, v.n_contigs, v.nb,
                               c->bc_mask.u64(), bs));
        pp.max_depth = std::max(pp.max_depth, (uint32_t)nd.maxima[0]);
        pp.max_need = std::max(pp.max_need, (uint32_t)nd.maxima[1]);
        pp.ms_need += nd.ms;
        return QMCP_OK;
    }
};

// the checks both entries make before anything is copied or launched
int check_proportional_call(uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t num, uint32_t den,
                            uint32_t max_coverage, uint32_t flags) {
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    if (!contig_lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    if (flags != 0) return fail(QMCP_EINVAL, "unknown flag bits 0x%x", flags);
    if (den == 0) return fail(QMCP_EINVAL, "the proportion's denominator is 0");
    if (den > QMCP_PROPORTION_DEN_MAX)
        return fail(QMCP_ERANGE, "the proportion's denominator %u exceeds %u", den, QMCP_PROPORTION_DEN_MAX);
    if (num > den) return fail(QMCP_EINVAL, "the proportion %u / %u is above 1", num, den);
    if (max_coverage >= qmcp::kCapLimit) return fail(QMCP_ERANGE, "max_coverage %u is 2^31 or more", max_coverage);
    return QMCP_OK;
}

int solve_proportional_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                                 uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, uint32_t num, uint32_t den,
                                 uint32_t floor, uint32_t max_coverage, uint64_t* d_mask, qmcp_hip_stats* stats,
                                 qmcp_hip_proportional_stats* pstats) {
    qmcp_hip_proportional_stats ps;
    std::memset(&ps, 0, sizeof(ps));
    ps.num = num;
    ps.den = den;
    ps.floor = floor;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (pstats) *pstats = ps;
    hipStream_t st = c->stream;
    TRY(ensure(c, c->pp_stat, qmcp::kPropStatWords * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->pp_stat.p, 0, qmcp::kPropStatWords * sizeof(unsigned long long), st));
    ProportionalRun pp;
    const bool flat = num == den || floor >= max_coverage;
    if (flat || num == 0) {
        ps.plain_route = 1;
        const uint32_t cap = flat ? max_coverage : std::min(floor, max_coverage);
        if (cap != 0) {
            TRY(solve_by_contig_on_device(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, cap, d_mask, stats));
        } else {
            GroupedReads g;
            TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, d_mask, g));
            qmcp_hip_stats sum;
            start_sum(g, sum);
            sum.n_reads = n64 - (g.offs[n_contigs + 1] - g.offs[n_contigs]);  // as the batches would have counted: placed
            if (stats) *stats = sum;
        }
    } else {
        pp.num = num;
        pp.den = den;
        pp.floor = floor;
        pp.max_coverage = max_coverage;
        GroupedReads g;
        TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, d_mask, g));
        ProportionalSolver fraction(pp);
        qmcp_hip_stats sum;
        TRY(run_batches(c, g, fraction, d_mask, sum));
        HIP_TRY(hipStreamSynchronize(st));
        collect_spans(c);
        if (stats) *stats = sum;
    }
    EventPair ev(c);
    if (!ev.a || !ev.b) return fail(QMCP_EHIP, "event creation failed");
    HIP_TRY(hipEventRecord(ev.a, st));
    {
        KernelSpan sp(c, "k_prop_tally");
        qmcp::launch_prop_tally(st, d_starts, d_ends, d_ids, n64, d_mask, c->pp_stat.as<unsigned long long>());
    }
    HIP_TRY(hipEventRecord(ev.b, st));
    HIP_TRY(hipGetLastError());
    unsigned long long w[qmcp::kPropStatWords];
    HIP_TRY(hipMemcpyAsync(w, c->pp_stat.p, sizeof(w), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    ps.reads_placed = w[qmcp::kPropPlaced];
    ps.bases_in = w[qmcp::kPropBasesIn];
    ps.bases_kept = w[qmcp::kPropBasesKept];
    ps.demand = w[qmcp::kPropDemand];
    ps.whole_positions = w[qmcp::kPropWholePositions];
    ps.floor_positions = w[qmcp::kPropFloorPositions];
    ps.capped_positions = w[qmcp::kPropCappedPositions];
    ps.max_depth = pp.max_depth;
    ps.max_need = pp.max_need;
    ps.ms_need = pp.ms_need;
    ps.ms_tally = elapsed(ev.a, ev.b);
    if (pstats) *pstats = ps;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_proportional_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends,
                                     const uint32_t* contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                     uint32_t n_contigs, uint32_t num, uint32_t den, uint32_t floor, uint32_t max_coverage,
                                     uint32_t flags, uint64_t* keep_mask_out, qmcp_hip_stats* stats,
                                     qmcp_hip_proportional_stats* pstats) {
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(check_proportional_call(n_reads, contig_lengths, n_contigs, num, den, max_coverage, flags));
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
    TRY(solve_proportional_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), n_reads, contig_lengths,
        n_contigs, num, den, floor, max_coverage, c->mask.u64(), stats, pstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_proportional_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                       const uint32_t* d_contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                       uint32_t n_contigs, uint32_t num, uint32_t den, uint32_t floor, uint32_t max_coverage,
                                       uint32_t flags, uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                       qmcp_hip_proportional_stats* pstats) {
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(check_proportional_call(n_reads, contig_lengths, n_contigs, num, den, max_coverage, flags));
    TRY(order_after(c, hip_stream));
    return solve_proportional_on_device(c, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, n_contigs, num, den,
                                        floor, max_coverage, d_keep_mask_out, stats, pstats);
}

}  // extern "C"
