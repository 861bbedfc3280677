// templates.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_templates_host / _device: the pair-aware staged solve (api/pairs.inc.hip) with the unit of selection
// generalised from the reads (2q, 2q + 1) to every segment that carries one template id.
//   1. once per call: the mask cleared, k_tpl_check (an id >= n_templates), k_tpl_sizes and k_tpl_size_hist (segments per
//      template, their histogram, the templates in use, the largest); the error word and the counts come back
//   2. group_by_contig, run_batches with the first stage's batch solver (a PlainSolver at the first target) and
//      pair_later_stages, as for pairs, with TemplateCompletion as the completion step: the bitset cleared, k_tpl_mark
//      (flags |= the ids of S), k_tpl_spread (S = the segments of flagged templates, and |S|)
//   3. after the last stage the bitset still holds the kept templates: its popcount is n_templates_kept
// api/templates_profile.inc.hip runs the same call (solve_templates_staged) under a cap per region: it hands in the
// StageNeeds of the later stages and the profile's batch solver for the first.
// Buffers: the feature's own (tp_*) and the pair stages' (pr_*).
namespace {

enum { kTplHist = 0, kTplUsed = 8, kTplLargest = 9, kTplKept = 10, kTplErr = 11, kTplStatWords = 12 };

size_t tpl_flag_bytes(uint32_t n_templates) { return (size_t)(((uint64_t)n_templates + 63) / 64) * sizeof(uint64_t); }

struct TemplateCompletion : UnitCompletion {
    const uint32_t* d_tids;
    uint32_t n_templates;
    TemplateCompletion(const uint32_t* ids, uint32_t nt) : d_tids(ids), n_templates(nt) {}
    int complete_and_count(qmcp_hip_ctx* c, uint64_t* d_mask, uint64_t n64) override {
        hipStream_t st = c->stream;
        unsigned long long* d_count = c->pr_stat.as<unsigned long long>() + 2;
        HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
        HIP_TRY(hipMemsetAsync(c->tp_flags.p, 0, tpl_flag_bytes(n_templates), st));
        if (n64) {
            KernelSpan sp(c, "k_tpl_mark + k_tpl_spread");
            qmcp::launch_tpl_mark(st, d_mask, d_tids, (uint32_t)n64, n_templates, c->tp_flags.u32());
            qmcp::launch_tpl_spread(st, d_tids, (uint32_t)n64, n_templates, c->tp_flags.u32(), d_mask, d_count);
        }
        HIP_TRY(hipGetLastError());
        return QMCP_OK;
    }
};

// what both entries check before the context is looked at, and the schedule
int check_templates_call(const void* template_ids, uint64_t n_reads, uint32_t n_templates, const uint32_t* stages,
                         uint32_t n_stages, uint32_t M, std::vector<uint32_t>& targets) {
    TRY(check_stage_list(stages, n_stages, M, targets));
    if (n_reads && !template_ids) return fail(QMCP_EINVAL, "template_ids is NULL with n_reads %llu", (unsigned long long)n_reads);
    if (n_reads && n_templates == 0)
        return fail(QMCP_EINVAL, "n_templates is 0 with n_reads %llu: every segment needs a template id", (unsigned long long)n_reads);
    return QMCP_OK;
}

void copy_stage_stats(qmcp_hip_template_stats& ts, const qmcp_hip_pair_stats& ps) {
    ts.n_stages = ps.n_stages;
    for (uint32_t j = 0; j < QMCP_PAIR_MAX_STAGES; ++j) {
        ts.n_selected[j] = ps.n_selected[j];
        ts.n_kept[j] = ps.n_kept[j];
        ts.capped_positions[j] = ps.capped_positions[j];
        ts.demand[j] = ps.demand[j];
        ts.target[j] = ps.target[j];
        ts.sweeps[j] = ps.sweeps[j];
        ts.ms_stage[j] = ps.ms_stage[j];
    }
}

// the staged call: stage 1's batches go through first_stage, the later stages ask later_needs for their need[]
int solve_templates_staged(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                           const uint32_t* d_tids, uint64_t n64, uint32_t n_templates, const uint32_t* lengths,
                           uint32_t n_contigs, const std::vector<uint32_t>& targets, BatchSolver& first_stage,
                           StageNeeds& later_needs, uint64_t* d_mask, qmcp_hip_stats* stats, qmcp_hip_template_stats* tstats) {
    hipStream_t st = c->stream;
    qmcp_hip_template_stats ts;
    std::memset(&ts, 0, sizeof(ts));
    TemplateCompletion whole(d_tids, n_templates);
    PairRun pr(targets, whole, later_needs);
    copy_stage_stats(ts, pr.ps);
    if (tstats) *tstats = ts;
    if (n64 > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n64);
    const uint32_t n = (uint32_t)n64;
    const size_t words = (size_t)((n64 + 63) / 64);

    // 1: ids, sizes, histogram
    EventPair ev(c);
    if (!ev.a || !ev.b) return fail(QMCP_EHIP, "event creation failed");
    TRY(ensure(c, c->tp_stat, kTplStatWords * sizeof(unsigned long long)));
    TRY(ensure(c, c->tp_flags, tpl_flag_bytes(n_templates)));
    TRY(ensure(c, c->tp_sizes, (size_t)n_templates * sizeof(uint32_t)));
    unsigned long long* d_tstat = c->tp_stat.as<unsigned long long>();
    unsigned long long h_tstat[kTplStatWords] = {0};
    HIP_TRY(hipEventRecord(ev.a, st));
    if (words) HIP_TRY(hipMemsetAsync(d_mask, 0, words * sizeof(uint64_t), st));
    HIP_TRY(hipMemsetAsync(d_tstat, 0, kTplStatWords * sizeof(unsigned long long), st));
    if (n) {
        HIP_TRY(hipMemsetAsync(c->tp_sizes.p, 0, (size_t)n_templates * sizeof(uint32_t), st));
        KernelSpan sp(c, "k_tpl_check + k_tpl_sizes + k_tpl_size_hist");
        qmcp::launch_tpl_check_sizes(st, d_tids, n, n_templates, (uint32_t*)(d_tstat + kTplErr), c->tp_sizes.u32(),
                                     d_tstat);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tstat, d_tstat, sizeof(h_tstat), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev.b, st));
    HIP_TRY(hipStreamSynchronize(st));
    ts.ms_templates = elapsed(ev.a, ev.b);
    if (h_tstat[kTplErr] & 1ull) {
        collect_spans(c);  // (the stream is idle: the span's events are done)
        return fail(QMCP_EINVAL, "a template id is not < n_templates (%u)", n_templates);
    }
    for (int b = 0; b < 8; ++b) ts.size_hist[b] = h_tstat[kTplHist + b];
    ts.n_templates_used = h_tstat[kTplUsed];
    ts.max_template_size = (uint32_t)h_tstat[kTplLargest];

    // 2: the stages
    GroupedReads g;
    TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, d_mask, g));
    qmcp_hip_stats plain;
    TRY(run_batches(c, g, first_stage, d_mask, plain));
    TRY(pair_later_stages(c, pr, g, d_mask, plain));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    copy_stage_stats(ts, pr.ps);
    ts.ms_templates += pr.ps.ms_pairs;

    // 3: the templates the last completion flagged
    HIP_TRY(hipEventRecord(ev.a, st));
    qmcp::launch_pair_count_bits(st, c->tp_flags.u64(), (uint32_t)(tpl_flag_bytes(n_templates) / sizeof(uint64_t)),
                                 d_tstat + kTplKept);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tstat, d_tstat + kTplKept, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev.b, st));
    HIP_TRY(hipStreamSynchronize(st));
    ts.ms_templates += elapsed(ev.a, ev.b);
    ts.n_templates_kept = h_tstat[0];
    if (stats) *stats = plain;
    if (tstats) *tstats = ts;
    return QMCP_OK;
}

// every stage at its target everywhere
int solve_templates_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                              const uint32_t* d_tids, uint64_t n64, uint32_t n_templates, const uint32_t* lengths,
                              uint32_t n_contigs, const std::vector<uint32_t>& targets, uint64_t* d_mask,
                              qmcp_hip_stats* stats, qmcp_hip_template_stats* tstats) {
    PlainSolver first(targets[0]);
    TargetNeeds needs(targets);
    return solve_templates_staged(c, d_starts, d_ends, d_ids, d_tids, n64, n_templates, lengths, n_contigs, targets, first,
                                  needs, d_mask, stats, tstats);
}

}  // namespace

extern "C" {

int qmcp_hip_solve_templates_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                  const uint32_t* template_ids, uint64_t n_reads, uint32_t n_templates,
                                  const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                  const uint32_t* stages, uint32_t n_stages, uint64_t* keep_mask_out, qmcp_hip_stats* stats,
                                  qmcp_hip_template_stats* tstats) {
    std::vector<uint32_t> targets;
    TRY(check_templates_call(template_ids, n_reads, n_templates, stages, n_stages, max_coverage, targets));
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
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
    TRY(solve_templates_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), c->tp_ids.u32(), n_reads,
        n_templates, contig_lengths, n_contigs, targets, c->mask.u64(), stats, tstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_templates_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                    const uint32_t* d_contig_ids, const uint32_t* d_template_ids, uint64_t n_reads,
                                    uint32_t n_templates, const uint32_t* contig_lengths, uint32_t n_contigs,
                                    uint32_t max_coverage, const uint32_t* stages, uint32_t n_stages,
                                    uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                    qmcp_hip_template_stats* tstats) {
    std::vector<uint32_t> targets;
    TRY(check_templates_call(d_template_ids, n_reads, n_templates, stages, n_stages, max_coverage, targets));
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(order_after(c, hip_stream));
    return solve_templates_on_device(c, d_starts, d_ends, d_contig_ids, d_template_ids, n_reads, n_templates, contig_lengths,
                                     n_contigs, targets, d_keep_mask_out, stats, tstats);
}

}  // extern "C"
