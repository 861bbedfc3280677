// templates_profile.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_templates_profile_host / _device: the template-aware staged solve (api/templates.inc.hip) under the
// coverage profile's region table (api/profile.inc.hip).  Stage j of the schedule T_1 < ... < T_k = M runs under
// c_j(p) = ceil(cap(p) * T_j / M); its need is min(cov_rest(p), max(0, c_j(p) - credit_j(p))).
//   1. every argument checked on the host: the templates entry's, then the profile entry's; cap_table.h builds the table
//   2. no region used and default_cap == M: solve_templates_on_device as it is (identity 1)
//   3. otherwise solve_templates_staged with
//        stage 1   a ProfileSolver over a copy of the table scaled to c_1: per batch the plain solve at the scaled default
//                  cap (no region), nothing (largest cap 0), or the profile's capped route
//        later     TemplateProfileNeeds: per stage and batch batch_cap_table, the caps scaled to c_j and uploaded into
//                  tq_tab, k_tpl_profile_need as the CappedNeed of capped_solve_batch; a batch whose largest c_j is 0 is
//                  skipped before its gather
//   4. once per call, after the stages (the segments are validated by then): k_tpl_on_cap over the unscaled table with
//      cap_positive_before's prefix counts, and k_pair_count_bits over its bitset
// Buffers: the templates', the pair stages' and the profile's own, plus tq_* (context.inc.hip).
namespace {

struct TemplateProfileNeed : StageNeed {
    std::vector<uint32_t> gs, ge, gcap;  // the batch's regions in its global positions, caps scaled to the stage
    uint32_t default_cap = 0;            // scaled as well
    const char* name() const override { return "k_tpl_profile_need"; }
    int reserve(qmcp_hip_ctx* c) override { return ensure(c, c->tq_tab, 3 * gs.size() * sizeof(uint32_t) + 16); }
    int upload(qmcp_hip_ctx* c, hipStream_t st) override {
        TRY(StageNeed::upload(c, st));
        const size_t n_reg = gs.size();
        uint32_t* d_rs = c->tq_tab.u32();
        if (n_reg) {
            HIP_TRY(hipMemcpyAsync(d_rs, gs.data(), n_reg * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_rs + n_reg, ge.data(), n_reg * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_rs + 2 * n_reg, gcap.data(), n_reg * 4, hipMemcpyHostToDevice, st));
        }
        return QMCP_OK;
    }
    void launch(qmcp_hip_ctx* c, hipStream_t st, uint32_t ltot, uint32_t* need) override {
        const size_t n_reg = gs.size();
        const uint32_t* d_rs = c->tq_tab.u32();
        qmcp::launch_tpl_profile_need(st, c->boff.u32(), c->eoff.u32(),
                                      c->pr_credit.u32() + qmcp::pair_credit_pad(), ltot, d_rs, d_rs + n_reg,
                                      d_rs + 2 * n_reg, (uint32_t)n_reg, default_cap, need, c->pr_stat.as<unsigned long long>());
    }
};

struct TemplateProfileNeeds : StageNeeds {
    const qmcp::CapTable& tab;
    const uint32_t* lengths;  // every contig's
    uint32_t default_cap, M;
    const std::vector<uint32_t>& targets;
    TemplateProfileNeed nd;
    float ms_done = 0.f;  // device time of the needs handed out before the current one
    TemplateProfileNeeds(const qmcp::CapTable& t, const uint32_t* len, uint32_t dcap, uint32_t m, const std::vector<uint32_t>& tg)
        : tab(t), lengths(len), default_cap(dcap), M(m), targets(tg) {}
    int make(qmcp_hip_ctx*, uint32_t j, const qmcp::ContigBatch& bt, StageNeed** need, uint32_t* max_cap) override {
        ms_done += nd.ms;
        nd.ms = 0.f;
        nd.counters[0] = nd.counters[1] = 0;
        qmcp::batch_cap_table(tab, lengths, bt.first_contig, bt.n_contigs, nd.gs, nd.ge, nd.gcap);
        const uint32_t T = targets[j];
        nd.default_cap = qmcp::scale_cap(default_cap, T, M);
        uint32_t top = nd.default_cap;
        for (uint32_t& cap : nd.gcap) {
            cap = qmcp::scale_cap(cap, T, M);
            top = std::max(top, cap);
        }
        *need = &nd;
        *max_cap = top;
        return QMCP_OK;
    }
    float ms_need() const { return ms_done + nd.ms; }
};

// what both entries check before the context is looked at; the schedule and the table
int check_templates_profile_call(const void* template_ids, uint64_t n_reads, uint32_t n_templates,
                                 const uint32_t* contig_lengths, uint32_t n_contigs, const uint32_t* region_offsets,
                                 const uint32_t* region_starts, const uint32_t* region_ends, const uint32_t* region_caps,
                                 uint32_t default_cap, uint32_t flags, uint32_t M, const uint32_t* stages, uint32_t n_stages,
                                 std::vector<uint32_t>& targets, qmcp::CapTable& tab) {
    TRY(check_templates_call(template_ids, n_reads, n_templates, stages, n_stages, M, targets));
    return check_profile_call(n_reads, contig_lengths, n_contigs, region_offsets, region_starts, region_ends, region_caps,
                              default_cap, flags, tab);
}

// step 4: the segments and the templates that touch a positive cap -> qs; its device time is added to *ms
int count_on_cap(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                 const uint32_t* d_tids, uint32_t n, uint32_t n_templates, uint32_t n_contigs, const qmcp::CapTable& tab,
                 uint32_t default_cap, qmcp_hip_template_profile_stats& qs, float* ms) {
    hipStream_t st = c->stream;
    std::vector<uint32_t> before;
    qmcp::cap_positive_before(tab, default_cap, before);
    const size_t n_reg = tab.rs.size(), n_offs = (size_t)n_contigs + 1;
    const size_t flag_bytes = tpl_flag_bytes(n_templates);
    EventPair ev(c);
    if (!ev.a || !ev.b) return fail(QMCP_EHIP, "event creation failed");
    TRY(ensure(c, c->tq_cap, (n_offs + 4 * n_reg) * sizeof(uint32_t) + 16));
    TRY(ensure(c, c->tq_flags, flag_bytes));
    TRY(ensure(c, c->tq_stat, 2 * sizeof(unsigned long long)));
    uint32_t* d_offs = c->tq_cap.u32();
    uint32_t* d_rs = d_offs + n_offs;
    unsigned long long* d_stat = c->tq_stat.as<unsigned long long>();
    unsigned long long h_stat[2] = {0, 0};
    HIP_TRY(hipEventRecord(ev.a, st));
    HIP_TRY(hipMemsetAsync(d_stat, 0, sizeof(h_stat), st));
    if (flag_bytes) HIP_TRY(hipMemsetAsync(c->tq_flags.p, 0, flag_bytes, st));
    HIP_TRY(hipMemcpyAsync(d_offs, tab.offs.data(), n_offs * 4, hipMemcpyHostToDevice, st));
    if (n_reg) {
        HIP_TRY(hipMemcpyAsync(d_rs, tab.rs.data(), n_reg * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_rs + n_reg, tab.re.data(), n_reg * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_rs + 2 * n_reg, tab.cap.data(), n_reg * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_rs + 3 * n_reg, before.data(), n_reg * 4, hipMemcpyHostToDevice, st));
    }
    if (n) {
        KernelSpan sp(c, "k_tpl_on_cap + k_pair_count_bits");
        qmcp::launch_tpl_on_cap(st, d_starts, d_ends, d_ids, d_tids, n, n_contigs, n_templates, d_offs, d_rs, d_rs + n_reg,
                                d_rs + 2 * n_reg, d_rs + 3 * n_reg, default_cap != 0, c->tq_flags.u32(), d_stat);
        qmcp::launch_pair_count_bits(st, c->tq_flags.u64(), (uint32_t)(flag_bytes / sizeof(uint64_t)), d_stat + 1);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_stat, d_stat, sizeof(h_stat), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev.b, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    *ms += elapsed(ev.a, ev.b);
    qs.n_segments_on_cap = h_stat[0];
    qs.n_templates_on_cap = h_stat[1];
    return QMCP_OK;
}

int solve_templates_profile_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                                      const uint32_t* d_tids, uint64_t n64, uint32_t n_templates, const uint32_t* lengths,
                                      uint32_t n_contigs, uint32_t M, const std::vector<uint32_t>& targets,
                                      const qmcp::CapTable& tab, uint32_t default_cap, uint64_t* d_mask, qmcp_hip_stats* stats,
                                      qmcp_hip_template_stats* tstats, qmcp_hip_template_profile_stats* qstats) {
    qmcp_hip_template_profile_stats qs;
    std::memset(&qs, 0, sizeof(qs));
    qs.regions_in = tab.regions_in;
    qs.regions_used = tab.regions_used;
    qs.positions_in_regions = tab.positions;
    if (qstats) *qstats = qs;
    // a failing solve leaves in *tstats what solve_templates_on_device wrote there (the schedule, no counts) and in
    // *qstats the table's counts, on either path
    qmcp_hip_template_stats ts;
    std::memset(&ts, 0, sizeof(ts));
    if (tab.regions_used == 0 && default_cap == M) {  // the fast path: the templates entry itself
        TRY(solve_templates_on_device(c, d_starts, d_ends, d_ids, d_tids, n64, n_templates, lengths, n_contigs, targets, d_mask,
                                      stats, tstats));
    } else {
        qmcp::CapTable first = tab;  // stage 1's table: the caps at c_1
        first.max_cap = 0;
        for (uint32_t& cap : first.cap) {
            cap = qmcp::scale_cap(cap, targets[0], M);
            first.max_cap = std::max(first.max_cap, cap);
        }
        ProfileRun pf;
        pf.tab = &first;
        pf.default_cap = qmcp::scale_cap(default_cap, targets[0], M);
        TRY(ensure(c, c->pf_stat, 2 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(c->pf_stat.p, 0, 2 * sizeof(unsigned long long), c->stream));
        ProfileSolver first_stage(pf);
        TemplateProfileNeeds needs(tab, lengths, default_cap, M, targets);
        TRY(solve_templates_staged(c, d_starts, d_ends, d_ids, d_tids, n64, n_templates, lengths, n_contigs, targets,
                                   first_stage, needs, d_mask, stats, tstats));
        qs.ms_need = pf.ms_profile + needs.ms_need();
    }
    if (tstats) ts = *tstats;
    TRY(count_on_cap(c, d_starts, d_ends, d_ids, d_tids, (uint32_t)n64, n_templates, n_contigs, tab, default_cap, qs,
                     &ts.ms_templates));  // (its time joins ms_templates: everything around the solves)
    if (tstats) *tstats = ts;
    if (qstats) *qstats = qs;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_templates_profile_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends,
                                          const uint32_t* contig_ids, const uint32_t* template_ids, uint64_t n_reads,
                                          uint32_t n_templates, const uint32_t* contig_lengths, uint32_t n_contigs,
                                          const uint32_t* region_offsets, const uint32_t* region_starts,
                                          const uint32_t* region_ends, const uint32_t* region_caps, uint32_t default_cap,
                                          uint32_t flags, uint32_t max_coverage, const uint32_t* stages, uint32_t n_stages,
                                          uint64_t* keep_mask_out, qmcp_hip_stats* stats, qmcp_hip_template_stats* tstats,
                                          qmcp_hip_template_profile_stats* qstats) {
    std::vector<uint32_t> targets;
    qmcp::CapTable tab;
    TRY(check_templates_profile_call(template_ids, n_reads, n_templates, contig_lengths, n_contigs, region_offsets,
                                     region_starts, region_ends, region_caps, default_cap, flags, max_coverage, stages,
                                     n_stages, targets, tab));
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    TRY(ensure(c, c->tp_ids, nb));
    TRY(ensure(c, c->mask, words * sizeof(uint64_t)));
    c->mask_reads = 0;
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->tp_ids.p, template_ids, nb, hipMemcpyHostToDevice, c->stream));
    }
    TRY(solve_templates_profile_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), c->tp_ids.u32(),
        n_reads, n_templates, contig_lengths, n_contigs, max_coverage, targets, tab, default_cap, c->mask.u64(), stats,
        tstats, qstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_templates_profile_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                            const uint32_t* d_contig_ids, const uint32_t* d_template_ids, uint64_t n_reads,
                                            uint32_t n_templates, const uint32_t* contig_lengths, uint32_t n_contigs,
                                            const uint32_t* region_offsets, const uint32_t* region_starts,
                                            const uint32_t* region_ends, const uint32_t* region_caps, uint32_t default_cap,
                                            uint32_t flags, uint32_t max_coverage, const uint32_t* stages, uint32_t n_stages,
                                            uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                            qmcp_hip_template_stats* tstats, qmcp_hip_template_profile_stats* qstats) {
    std::vector<uint32_t> targets;
    qmcp::CapTable tab;
    TRY(check_templates_profile_call(d_template_ids, n_reads, n_templates, contig_lengths, n_contigs, region_offsets,
                                     region_starts, region_ends, region_caps, default_cap, flags, max_coverage, stages,
                                     n_stages, targets, tab));
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(order_after(c, hip_stream));
    return solve_templates_profile_on_device(c, d_starts, d_ends, d_contig_ids, d_template_ids, n_reads, n_templates,
                                             contig_lengths, n_contigs, max_coverage, targets, tab, default_cap,
                                             d_keep_mask_out, stats, tstats, qstats);
}

}  // extern "C"
