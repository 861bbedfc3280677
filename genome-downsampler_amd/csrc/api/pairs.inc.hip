// pairs.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_pairs_host / _device: a staged solve that credits the mates' coverage.  Reads (2q, 2q + 1) are pair q;
// targets T_1 < ... < T_k = M.  Stage 1 is the by-contig flow at T_1 (group_by_contig, run_batches with a PlainSolver: every
// fast route) and the pair OR over its input-order mask S.  Stage j > 1 runs over ALL batches of the same grouping before
// the next stage begins -- a mate may lie in another batch, so S must be whole first -- and per batch:
//   1. k_bc_gather (the batch's columns again) and k_pair_gather_mask: S in grouped order, and its complement, the
//      stage's candidates
//   2. k_word_popcounts -> exclusive scan of the complement; k_ladder_offsets: the candidates' contig offsets, read back
//      once; k_ladder_compact: their starts, ends and input indices
//   3. k_pair_credit_events on a zeroed axis, scanned in place: credit[p], the depth of the batch's reads in S
//   4. capped_solve_batch (api/profile.inc.hip) on the candidates with k_pair_need building need[p] = min(cov_rest(p),
//      max(0, T_j - credit[p])) -- or whatever StageNeed the entry's StageNeeds hands out; its counters come back before
//      the sweep is queued, and a batch that asks for nothing queues none
//   5. k_expand_mask_reads ORs the kept candidates into S
// and after the last batch the completion (a UnitCompletion: k_complete_pairs here) over S and its popcount.  A batch
// without candidates stops after step 2.
// Buffers: all the feature's own (pr_*), apart from the by-contig call's gathered columns (bc_starts / bc_ends), which
// are refilled per batch; nothing a solve owns is held across a solve.
namespace {

// how a stage's kept set S is completed to whole units: queues S |= the rest of every unit S touches, and |S| ->
// pr_stat[2].  The pairs entry ORs inside each aligned bit pair; api/templates.inc.hip goes through a bitset of ids.
struct UnitCompletion {
    virtual int complete_and_count(qmcp_hip_ctx* c, uint64_t* d_mask, uint64_t n64) = 0;
    virtual ~UnitCompletion() = default;
};

// need[] of a stage after the first: built over the candidates from the credit of the reads already kept; need[] lives
// in pr_need, the two counters in pr_stat[0 .. 1]
struct StageNeed : CappedNeed {
    unsigned long long counters[2] = {0, 0};  // capped positions, demand: this batch's
    DevBuf& need_buf(qmcp_hip_ctx* c) override { return c->pr_need; }
    int reserve(qmcp_hip_ctx*) override { return QMCP_OK; }
    int upload(qmcp_hip_ctx* c, hipStream_t st) override {
        HIP_TRY(hipMemsetAsync(c->pr_stat.p, 0, 2 * sizeof(unsigned long long), st));
        return QMCP_OK;
    }
    int no_demand(qmcp_hip_ctx* c, hipStream_t st, bool* none) override {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(counters, c->pr_stat.p, sizeof(counters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *none = counters[1] == 0;
        return QMCP_OK;
    }
};

// one target everywhere, through k_pair_need
struct PairNeed : StageNeed {
    uint32_t target;
    explicit PairNeed(uint32_t t) : target(t) {}
    const char* name() const override { return "k_pair_need"; }
    void launch(qmcp_hip_ctx* c, hipStream_t st, uint32_t ltot, uint32_t* need) override {
        qmcp::launch_pair_need(st, c->boff.u32(), c->eoff.u32(), c->pr_credit.u32() + qmcp::pair_credit_pad(), ltot,
                               target, need, c->pr_stat.as<unsigned long long>());
    }
};

// What gives stage j (>= 1) of a batch its StageNeed, and the largest cap that need can meet: it chooses the sweep's
// windows, and a batch whose largest cap is 0 is skipped before its gather.  The pairs and templates entries ask for the
// stage's target everywhere; api/templates_profile.inc.hip scales the batch's region table to the stage.
struct StageNeeds {
    virtual ~StageNeeds() = default;
    // the returned object lives until the next call
    virtual int make(qmcp_hip_ctx* c, uint32_t j, const qmcp::ContigBatch& bt, StageNeed** need, uint32_t* max_cap) = 0;
};

struct PairRun {
    const std::vector<uint32_t>& targets;
    qmcp_hip_pair_stats ps;
    UnitCompletion* completion;  // the entry's, for the length of its call
    StageNeeds* needs;           // the entry's, for the length of its call
    PairRun(const std::vector<uint32_t>& t, UnitCompletion& whole, StageNeeds& later)
        : targets(t), completion(&whole), needs(&later) {
        std::memset(&ps, 0, sizeof(ps));
        ps.n_stages = (uint32_t)targets.size();
        for (size_t j = 0; j < targets.size(); ++j) ps.target[j] = targets[j];
    }
};

struct TargetNeeds : StageNeeds {
    const std::vector<uint32_t>& targets;
    PairNeed nd{0};
    explicit TargetNeeds(const std::vector<uint32_t>& t) : targets(t) {}
    int make(qmcp_hip_ctx*, uint32_t j, const qmcp::ContigBatch&, StageNeed** need, uint32_t* max_cap) override {
        nd = PairNeed(targets[j]);
        *need = &nd;
        *max_cap = targets[j];
        return QMCP_OK;
    }
};

// queues S |= mates and |S| -> pr_stat[2]
int pair_complete_and_count(qmcp_hip_ctx* c, uint64_t* d_mask, uint64_t n64) {
    hipStream_t st = c->stream;
    const uint32_t words = (uint32_t)((n64 + 63) / 64);
    unsigned long long* d_count = c->pr_stat.as<unsigned long long>() + 2;
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
    if (words) {
        KernelSpan sp(c, "k_complete_pairs(pairs) + k_pair_count_bits");
        qmcp::launch_complete_pairs(st, d_mask, words, n64);
        qmcp::launch_pair_count_bits(st, d_mask, words, d_count);
    }
    HIP_TRY(hipGetLastError());
    return QMCP_OK;
}

struct PairCompletion : UnitCompletion {
    int complete_and_count(qmcp_hip_ctx* c, uint64_t* d_mask, uint64_t n64) override {
        return pair_complete_and_count(c, d_mask, n64);
    }
};

// the completion of stage 1's mask, and every later stage over all batches of the grouping
int pair_later_stages(qmcp_hip_ctx* c, PairRun& pr, const GroupedReads& g, uint64_t* d_mask, const qmcp_hip_stats& first) {
    hipStream_t st = c->stream;
    qmcp_hip_pair_stats& ps = pr.ps;
    const uint32_t pad = qmcp::pair_credit_pad();
    EventPair ev_a(c), ev_b(c);
    if (!ev_a.a || !ev_a.b || !ev_b.a || !ev_b.b) return fail(QMCP_EHIP, "event creation failed");
    TRY(ensure(c, c->pr_stat, 4 * sizeof(unsigned long long)));
    unsigned long long count = 0;
    const unsigned long long* d_count = c->pr_stat.as<unsigned long long>() + 2;
    ps.n_selected[0] = first.n_kept;
    ps.ms_stage[0] = first.ms_total;
    // ev_a brackets what is queued between two host waits; `open` says its first event has been recorded
    bool open = false;
    auto begin = [&]() -> int {
        if (!open) HIP_TRY(hipEventRecord(ev_a.a, st));
        open = true;
        return QMCP_OK;
    };
    auto wait = [&]() -> int {  // close the bracket, wait, add its time
        HIP_TRY(hipEventRecord(ev_a.b, st));
        HIP_TRY(hipStreamSynchronize(st));
        ps.ms_pairs += elapsed(ev_a.a, ev_a.b);
        open = false;
        return QMCP_OK;
    };
    TRY(begin());
    TRY(pr.completion->complete_and_count(c, d_mask, g.n64));
    HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof(count), hipMemcpyDeviceToHost, st));
    TRY(wait());
    ps.n_kept[0] = count;

    std::vector<uint32_t> ranks;
    std::vector<uint64_t> cand_roff;
    BatchView v;
    for (uint32_t j = 1; j < (uint32_t)pr.targets.size(); ++j) {
        for (size_t b : g.live) {
            const qmcp::ContigBatch& bt = g.batches[b];
            StageNeed* need = nullptr;
            uint32_t max_cap = 0;
            TRY(pr.needs->make(c, j, bt, &need, &max_cap));
            if (max_cap == 0) continue;  // nothing can be asked for anywhere in this batch
            const uint32_t nb = (uint32_t)bt.n_reads;
            const uint32_t ltot = (uint32_t)bt.positions;
            const uint32_t words = (nb + 63u) / 64u;
            const size_t tab = (size_t)bt.n_contigs + 1;
            g.view(b, v);
            v.tables32();
            ranks.assign(tab, 0);
            TRY(ensure(c, c->pr_in, (size_t)words * sizeof(uint64_t)));
            TRY(ensure(c, c->pr_rest, (size_t)words * sizeof(uint64_t)));
            TRY(ensure(c, c->pr_words, ((size_t)words + 2) * sizeof(uint32_t)));
            TRY(ensure(c, c->pr_spine, scan_spine_bytes(words + 1, 1)));
            TRY(ensure(c, c->pr_offs[0], tab * sizeof(uint32_t)));
            TRY(ensure(c, c->pr_offs[1], tab * sizeof(uint32_t)));
            TRY(ensure(c, c->pr_poff, tab * sizeof(uint32_t)));
            TRY(ensure(c, c->pr_credit, ((size_t)ltot + pad + 4) * sizeof(uint32_t)));
            TRY(ensure(c, c->pr_cspine, scan_spine_bytes(ltot + pad, 1)));
            // 1 - 3: S and the candidates in grouped order, the candidates' offsets, the credit of S
            TRY(begin());
            HIP_TRY(hipMemcpyAsync(c->pr_offs[0].p, v.offs32.data(), tab * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(c->pr_poff.p, v.poff32.data(), tab * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemsetAsync(c->pr_credit.p, 0, ((size_t)ltot + pad) * sizeof(uint32_t), st));
            TRY(gather_batch(c, v, g.d_starts, g.d_ends));
            {
                KernelSpan sp(c, "k_pair_gather_mask");
                qmcp::launch_pair_gather_mask(st, v.records, nb, d_mask, c->pr_in.u64(), c->pr_rest.u64());
            }
            {
                KernelSpan sp(c, "pair candidates(popcounts, scan, k_ladder_offsets)");
                queue_mask_ranks(st, c->pr_rest.u64(), words, c->pr_words, c->pr_spine);
                qmcp::launch_ladder_offsets(st, c->pr_offs[0].u32(), bt.n_contigs, c->pr_rest.u64(),
                                            c->pr_words.u32(), c->pr_offs[1].u32());
            }
            {
                KernelSpan sp(c, "k_pair_credit_events + scan");
                qmcp::launch_pair_credit_events(st, v.records, nb, c->pr_in.u64(), c->bc_starts.u32(), c->bc_ends.u32(),
                                                c->pr_poff.u32(), bt.first_contig, c->pr_credit.u32());
                qmcp::launch_exclusive_scan(st, c->pr_credit.u32(), ltot + pad, c->pr_credit.u32(),
                                            c->pr_cspine.u32(), false);
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(ranks.data(), c->pr_offs[1].p, tab * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            TRY(wait());
            if (qmcp::pair_candidate_offsets(v.roff.data(), ranks.data(), bt.n_contigs, cand_roff) != QMCP_OK)
                return fail(QMCP_EHIP, "pair stage %u: the candidates' ranks do not fit the contig offsets", j);
            const uint32_t n_c = ranks[bt.n_contigs];
            if (n_c == 0) continue;  // every read of the batch is kept already
            const size_t cb = (size_t)n_c * sizeof(uint32_t);
            TRY(ensure(c, c->pr_starts, cb));
            TRY(ensure(c, c->pr_ends, cb));
            TRY(ensure(c, c->pr_orig, cb));
            TRY(ensure(c, c->pr_mask, (size_t)((n_c + 63u) / 64u) * sizeof(uint64_t)));
            HIP_TRY(hipEventRecord(ev_b.a, st));
            {
                KernelSpan sp(c, "k_ladder_compact(pairs)");
                qmcp::launch_ladder_compact(st, true, c->bc_starts.u32(), c->bc_ends.u32(), v.records,
                                            c->pr_rest.u64(), c->pr_words.u32(), nb,
                                            c->pr_starts.u32(), c->pr_ends.u32(), c->pr_orig.u32());
            }
            HIP_TRY(hipEventRecord(ev_b.b, st));
            HIP_TRY(hipGetLastError());
            // 4: the capped route on the candidates
            StageNeed& nd = *need;
            qmcp_hip_stats bs;
            std::memset(&bs, 0, sizeof(bs));
            bool swept = false;
            TRY(capped_solve_batch(c, nd, max_cap, c->pr_starts.u32(), c->pr_ends.u32(), cand_roff.data(), v.lengths,
                bt.n_contigs, n_c, c->pr_mask.u64(), &bs, &swept));
            ps.ms_pairs += elapsed(ev_b.a, ev_b.b) + nd.ms;
            ps.n_selected[j] += bs.n_kept;
            ps.ms_stage[j] += bs.ms_total;
            ps.sweeps[j] += swept ? 1u : 0u;
            ps.capped_positions[j] += nd.counters[0];
            ps.demand[j] += nd.counters[1];
            // 5: the kept candidates join S (the bracket stays open into the next batch, or the stage's end)
            if (bs.n_kept) {
                TRY(begin());
                KernelSpan sp(c, "k_expand_mask_reads(pairs)");
                qmcp::launch_expand_mask_reads(st, c->pr_mask.u64(), c->pr_orig.u32(), n_c, d_mask);
            }
            HIP_TRY(hipGetLastError());
        }
        TRY(begin());
        TRY(pr.completion->complete_and_count(c, d_mask, g.n64));
        HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof(count), hipMemcpyDeviceToHost, st));
        TRY(wait());
        ps.n_kept[j] = count;
    }
    return QMCP_OK;
}

// the stage list of a staged call (pairs, templates), checked before anything is copied or launched, and the schedule
int check_stage_list(const uint32_t* stages, uint32_t n_stages, uint32_t M, std::vector<uint32_t>& targets) {
    uint32_t bad = 0;
    const int rc = qmcp::pair_schedule(stages, n_stages, M, targets, &bad);
    if (rc == QMCP_OK) return QMCP_OK;
    if (M >= qmcp::kPairTargetLimit) return fail(QMCP_ERANGE, "max_coverage %u is 2^31 or more", M);
    if (rc == QMCP_ERANGE) return fail(QMCP_ERANGE, "stages[%u] = %u is 2^31 or more", bad, stages[bad]);
    if (M == 0) return fail(QMCP_EINVAL, "max_coverage is 0: a staged solve needs a target >= 1");
    if (n_stages == 0 || n_stages > QMCP_PAIR_MAX_STAGES)
        return fail(QMCP_EINVAL, "n_stages %u is not in 1 .. %u", n_stages, (unsigned)QMCP_PAIR_MAX_STAGES);
    if (stages[bad] == 0) return fail(QMCP_EINVAL, "stages[%u] is 0: every stage needs a target >= 1", bad);
    if (bad > 0 && stages[bad] <= stages[bad - 1])
        return fail(QMCP_EINVAL, "stages must rise strictly: stages[%u] = %u is not above stages[%u] = %u", bad, stages[bad],
                    bad - 1, stages[bad - 1]);
    return fail(QMCP_EINVAL, "the last stage must be max_coverage: stages[%u] = %u, max_coverage = %u", bad, stages[bad], M);
}

// what both pair entries check first
int check_pairs_call(uint64_t n_reads, const uint32_t* stages, uint32_t n_stages, uint32_t M, std::vector<uint32_t>& targets) {
    if (n_reads & 1ull)
        return fail(QMCP_EINVAL, "n_reads %llu is odd: reads (2q, 2q + 1) are pair q", (unsigned long long)n_reads);
    return check_stage_list(stages, n_stages, M, targets);
}

int solve_pairs_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                          uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, const std::vector<uint32_t>& targets,
                          uint64_t* d_mask, qmcp_hip_stats* stats, qmcp_hip_pair_stats* pstats) {
    PairCompletion mates;
    TargetNeeds needs(targets);
    PairRun pr(targets, mates, needs);
    if (pstats) *pstats = pr.ps;
    GroupedReads g;
    TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, d_mask, g));
    PlainSolver first(targets[0]);
    qmcp_hip_stats plain;
    TRY(run_batches(c, g, first, d_mask, plain));
    TRY(pair_later_stages(c, pr, g, d_mask, plain));
    HIP_TRY(hipStreamSynchronize(c->stream));
    collect_spans(c);
    if (stats) *stats = plain;
    if (pstats) *pstats = pr.ps;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_pairs_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                              uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                              const uint32_t* stages, uint32_t n_stages, uint64_t* keep_mask_out, qmcp_hip_stats* stats,
                              qmcp_hip_pair_stats* pstats) {
    std::vector<uint32_t> targets;
    TRY(check_pairs_call(n_reads, stages, n_stages, max_coverage, targets));
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
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
    TRY(solve_pairs_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(),
                              n_reads, contig_lengths, n_contigs, targets, c->mask.u64(), stats, pstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_pairs_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                const uint32_t* d_contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                uint32_t n_contigs, uint32_t max_coverage, const uint32_t* stages, uint32_t n_stages,
                                uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                qmcp_hip_pair_stats* pstats) {
    std::vector<uint32_t> targets;
    TRY(check_pairs_call(n_reads, stages, n_stages, max_coverage, targets));
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(order_after(c, hip_stream));
    return solve_pairs_on_device(c, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, n_contigs, targets,
                                 d_keep_mask_out, stats, pstats);
}

}  // extern "C"
