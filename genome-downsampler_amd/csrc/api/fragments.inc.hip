// fragments.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_clip_templates_host / _device and qmcp_hip_solve_fragments_host / _device: the segments of a template clipped
// where they overlap, so that depth per segment on the clipped columns is fragment depth.
//   1. k_tpl_check + k_tpl_sizes + k_tpl_size_hist (a template id >= n_templates; the largest template) and k_frag_check
//      (contig ids, reads, the placed rows and their bases): one host round trip, and every error is found here, before
//      anything is clipped or written
//   2. no template of two segments: the identity -- two device-to-device copies, no sort, no scan
//   3. otherwise fragment_plan.h picks the digits; per round k_frag_keys and radix_sort_wide, the value column carried from
//      round to round; then k_frag_tiles, k_frag_spine, k_frag_apply and the popcount of the templates that changed
// solve_fragments is step 1 - 3 into the context's own columns (fr_cs, fr_cc) followed by solve_templates_on_device on them.
// Buffers: the feature's own (fr_*), and the template entry's tp_stat / tp_sizes / tp_flags, which it sizes and clears
// again for itself.
namespace {

// what the clip entries check before the context is looked at
int check_clip_call(const void* template_ids, uint64_t n_reads, uint32_t n_templates) {
    if (n_reads && !template_ids) return fail(QMCP_EINVAL, "template_ids is NULL with n_reads %llu", (unsigned long long)n_reads);
    if (n_reads && n_templates == 0)
        return fail(QMCP_EINVAL, "n_templates is 0 with n_reads %llu: every segment needs a template id", (unsigned long long)n_reads);
    return QMCP_OK;
}

int check_clip_tables(uint64_t n_reads, const uint32_t* lengths, uint32_t n_contigs) {
    if (!lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    return QMCP_OK;
}

bool ranges_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && bytes && x < y + bytes && y < x + bytes;
}

int check_clip_outputs(const uint32_t* starts, const uint32_t* ends, const uint32_t* ids, const uint32_t* tids,
                       uint64_t n_reads, const uint32_t* out_s, const uint32_t* out_c) {
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const void* in[4] = {starts, ends, ids, tids};
    for (const void* p : in)
        if (ranges_overlap(p, out_s, nb) || ranges_overlap(p, out_c, nb))
            return fail(QMCP_EINVAL, "a clip output overlaps an input column");
    if (ranges_overlap(out_s, out_c, nb)) return fail(QMCP_EINVAL, "the two clip outputs overlap");
    return QMCP_OK;
}

int clip_templates_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                             const uint32_t* d_tids, uint64_t n64, uint32_t n_templates, const uint32_t* lengths,
                             uint32_t n_contigs, uint32_t* d_out_s, uint32_t* d_out_c, qmcp_hip_fragment_stats* fstats) {
    hipStream_t st = c->stream;
    qmcp_hip_fragment_stats fs;
    std::memset(&fs, 0, sizeof(fs));
    if (fstats) *fstats = fs;
    TRY(check_clip_tables(n64, lengths, n_contigs));
    const uint32_t n = (uint32_t)n64;
    if (n == 0) return QMCP_OK;
    const size_t nb = (size_t)n * sizeof(uint32_t);

    // 1: validation, the largest template, the placed rows
    EventPair ev(c), ev2(c);
    if (!ev.a || !ev.b || !ev2.a || !ev2.b) return fail(QMCP_EHIP, "event creation failed");
    TRY(ensure(c, c->tp_stat, kTplStatWords * sizeof(unsigned long long)));
    TRY(ensure(c, c->tp_sizes, (size_t)n_templates * sizeof(uint32_t)));
    TRY(ensure(c, c->tp_flags, tpl_flag_bytes(n_templates)));
    TRY(ensure(c, c->fr_stat, qmcp::kFragWords * sizeof(unsigned long long)));
    TRY(ensure(c, c->fr_len, (size_t)n_contigs * sizeof(uint32_t)));
    unsigned long long* d_tstat = c->tp_stat.as<unsigned long long>();
    unsigned long long* d_fstat = c->fr_stat.as<unsigned long long>();
    unsigned long long h_tstat[kTplStatWords] = {0}, h_fstat[qmcp::kFragWords] = {0};
    HIP_TRY(hipMemcpyAsync(c->fr_len.p, lengths, (size_t)n_contigs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(ev.a, st));
    HIP_TRY(hipMemsetAsync(d_tstat, 0, kTplStatWords * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(d_fstat, 0, qmcp::kFragWords * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(c->tp_sizes.p, 0, (size_t)n_templates * sizeof(uint32_t), st));
    {
        KernelSpan sp(c, "k_tpl_check + k_tpl_sizes + k_tpl_size_hist");
        qmcp::launch_tpl_check_sizes(st, d_tids, n, n_templates, (uint32_t*)(d_tstat + kTplErr), c->tp_sizes.u32(), d_tstat);
    }
    {
        KernelSpan sp(c, "k_frag_check");
        qmcp::launch_frag_check(st, d_starts, d_ends, d_ids, n, c->fr_len.u32(), n_contigs, d_fstat);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tstat, d_tstat, sizeof(h_tstat), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_fstat, d_fstat, sizeof(h_fstat), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev.b, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    if (h_tstat[kTplErr] & 1ull) return fail(QMCP_EINVAL, "a template id is not < n_templates (%u)", n_templates);
    if (h_fstat[qmcp::kFragErr] & 1ull)
        return fail(QMCP_EINVAL, "a contig id is neither < n_contigs (%u) nor QMCP_NO_CONTIG", n_contigs);
    if (h_fstat[qmcp::kFragErr] & 2ull) return fail(QMCP_EREAD, "a read has start > end or end >= its contig's length");
    fs.ms_clip = elapsed(ev.a, ev.b);
    fs.n_placed = h_fstat[qmcp::kFragPlaced];
    fs.bases_in = h_fstat[qmcp::kFragBasesIn];

    // 2: no template has two segments
    HIP_TRY(hipEventRecord(ev2.a, st));
    if (h_tstat[kTplLargest] < 2) {
        HIP_TRY(hipMemcpyAsync(d_out_s, d_starts, nb, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_out_c, d_ids, nb, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipEventRecord(ev2.b, st));
        HIP_TRY(hipStreamSynchronize(st));
        fs.ms_clip += elapsed(ev2.a, ev2.b);
        fs.max_group = fs.n_placed ? 1u : 0u;
        if (fstats) *fstats = fs;
        return QMCP_OK;
    }

    // 3: sort by (template, contig, start), scan, write back
    uint32_t longest = 0;
    for (uint32_t k = 0; k < n_contigs; ++k) longest = std::max(longest, lengths[k]);
    const qmcp::FragmentPlan plan = qmcp::plan_fragment_sort(n_templates, n_contigs, longest);
    const uint32_t n_tiles = qmcp::sort_tiles(n);
    TRY(ensure(c, c->fr_keys[0], (size_t)n * 8));
    TRY(ensure(c, c->fr_keys[1], (size_t)n * 8));
    TRY(ensure(c, c->fr_vals[0], nb));
    TRY(ensure(c, c->fr_vals[1], nb));
    TRY(ensure(c, c->fr_hist, (size_t)256 * n_tiles * sizeof(uint32_t)));
    TRY(ensure(c, c->fr_spine, std::max(scan_spine_bytes(256u * n_tiles, 1), qmcp::frag_spine_bytes(n))));
    HIP_TRY(hipMemsetAsync(c->tp_flags.p, 0, tpl_flag_bytes(n_templates), st));
    WideBufs wb;
    for (uint32_t r = 0; r < plan.n_rounds; ++r) {
        const qmcp::FragmentRound& round = plan.rounds[r];
        {
            KernelSpan sp(c, "k_frag_keys");
            qmcp::launch_frag_keys(st, d_starts, d_ids, d_tids, wb.v < 0 ? nullptr : c->fr_vals[wb.v].u32(), n,
                                   round.start_bytes, round.contig_bytes, round.template_bytes, c->fr_keys[wb.k].p);
        }
        TRY(radix_sort_wide(c, st, n, round.passes, c->fr_hist.u32(), c->fr_spine.u32(), c->fr_keys, c->fr_vals,
                            {"k_radix_hist(fragments, u64)", "scan_radix_hist(fragments, 3 kernels)",
                             "k_radix_scatter(fragments, u64)"},
                            &wb));
    }
    {
        KernelSpan sp(c, "k_frag_tiles + k_frag_spine + k_frag_apply");
        qmcp::launch_frag_scan_apply(st, c->fr_vals[wb.v].u32(), d_starts, d_ends, d_ids, d_tids, n, n_templates,
                                     c->fr_spine.p, d_out_s, d_out_c, c->tp_flags.u32(), d_fstat);
    }
    qmcp::launch_pair_count_bits(st, c->tp_flags.u64(), (uint32_t)(tpl_flag_bytes(n_templates) / sizeof(uint64_t)),
                                 d_fstat + qmcp::kFragOverlapT);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_fstat, d_fstat, sizeof(h_fstat), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev2.b, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    fs.ms_clip += elapsed(ev2.a, ev2.b);
    fs.n_clipped = h_fstat[qmcp::kFragClipped];
    fs.n_emptied = h_fstat[qmcp::kFragEmptied];
    fs.bases_removed = h_fstat[qmcp::kFragRemoved];
    fs.n_templates_overlapping = h_fstat[qmcp::kFragOverlapT];
    fs.max_group = (uint32_t)h_fstat[qmcp::kFragMaxGroup];
    if (fstats) *fstats = fs;
    return QMCP_OK;
}

// the clip into the context's own columns, then the template stages on them; the mask is cleared before the clip can fail
int solve_fragments_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                              const uint32_t* d_tids, uint64_t n64, uint32_t n_templates, const uint32_t* lengths,
                              uint32_t n_contigs, const std::vector<uint32_t>& targets, uint64_t* d_mask,
                              qmcp_hip_stats* stats, qmcp_hip_template_stats* tstats, qmcp_hip_fragment_stats* fstats) {
    const size_t nb = (size_t)n64 * sizeof(uint32_t);
    const size_t words = (size_t)((n64 + 63) / 64);
    TRY(ensure(c, c->fr_cs, nb));
    TRY(ensure(c, c->fr_cc, nb));
    if (words) HIP_TRY(hipMemsetAsync(d_mask, 0, words * sizeof(uint64_t), c->stream));
    const int rc = clip_templates_on_device(c, d_starts, d_ends, d_ids, d_tids, n64, n_templates, lengths, n_contigs,
                                            c->fr_cs.u32(), c->fr_cc.u32(), fstats);
    if (rc != QMCP_OK) {
        (void)hipStreamSynchronize(c->stream);  // (the cleared mask is the caller's to read)
        return rc;
    }
    return solve_templates_on_device(c, c->fr_cs.u32(), d_ends, c->fr_cc.u32(), d_tids, n64, n_templates, lengths, n_contigs,
                                     targets, d_mask, stats, tstats);
}

}  // namespace

extern "C" {

int qmcp_hip_clip_templates_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                 const uint32_t* template_ids, uint64_t n_reads, uint32_t n_templates,
                                 const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t* clipped_starts_out,
                                 uint32_t* clipped_contig_ids_out, qmcp_hip_fragment_stats* fstats) {
    TRY(check_clip_call(template_ids, n_reads, n_templates));
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !clipped_starts_out || !clipped_contig_ids_out))
        return fail(QMCP_EINVAL, "null buffer");
    TRY(check_clip_tables(n_reads, contig_lengths, n_contigs));
    TRY(check_clip_outputs(starts, ends, contig_ids, template_ids, n_reads, clipped_starts_out, clipped_contig_ids_out));
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    TRY(ensure(c, c->tp_ids, nb));
    TRY(ensure(c, c->fr_cs, nb));
    TRY(ensure(c, c->fr_cc, nb));
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->tp_ids.p, template_ids, nb, hipMemcpyHostToDevice, c->stream));
    }
    TRY(clip_templates_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), c->tp_ids.u32(), n_reads,
                                 n_templates, contig_lengths, n_contigs, c->fr_cs.u32(), c->fr_cc.u32(), fstats));
    if (nb) {
        HIP_TRY(hipMemcpyAsync(clipped_starts_out, c->fr_cs.p, nb, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(clipped_contig_ids_out, c->fr_cc.p, nb, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return QMCP_OK;
}

int qmcp_hip_clip_templates_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                   const uint32_t* d_contig_ids, const uint32_t* d_template_ids, uint64_t n_reads,
                                   uint32_t n_templates, const uint32_t* contig_lengths, uint32_t n_contigs,
                                   uint32_t* d_clipped_starts_out, uint32_t* d_clipped_contig_ids_out, void* hip_stream,
                                   qmcp_hip_fragment_stats* fstats) {
    TRY(check_clip_call(d_template_ids, n_reads, n_templates));
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_clipped_starts_out || !d_clipped_contig_ids_out))
        return fail(QMCP_EINVAL, "null buffer");
    TRY(check_clip_tables(n_reads, contig_lengths, n_contigs));
    TRY(check_clip_outputs(d_starts, d_ends, d_contig_ids, d_template_ids, n_reads, d_clipped_starts_out,
                           d_clipped_contig_ids_out));
    TRY(order_after(c, hip_stream));
    return clip_templates_on_device(c, d_starts, d_ends, d_contig_ids, d_template_ids, n_reads, n_templates, contig_lengths,
                                    n_contigs, d_clipped_starts_out, d_clipped_contig_ids_out, fstats);
}

int qmcp_hip_solve_fragments_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                  const uint32_t* template_ids, uint64_t n_reads, uint32_t n_templates,
                                  const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                  const uint32_t* stages, uint32_t n_stages, uint64_t* keep_mask_out, qmcp_hip_stats* stats,
                                  qmcp_hip_template_stats* tstats, qmcp_hip_fragment_stats* fstats) {
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
    TRY(solve_fragments_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), c->tp_ids.u32(), n_reads,
                                  n_templates, contig_lengths, n_contigs, targets, c->mask.u64(), stats, tstats, fstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_fragments_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                    const uint32_t* d_contig_ids, const uint32_t* d_template_ids, uint64_t n_reads,
                                    uint32_t n_templates, const uint32_t* contig_lengths, uint32_t n_contigs,
                                    uint32_t max_coverage, const uint32_t* stages, uint32_t n_stages,
                                    uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                    qmcp_hip_template_stats* tstats, qmcp_hip_fragment_stats* fstats) {
    std::vector<uint32_t> targets;
    TRY(check_templates_call(d_template_ids, n_reads, n_templates, stages, n_stages, max_coverage, targets));
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    TRY(order_after(c, hip_stream));
    return solve_fragments_on_device(c, d_starts, d_ends, d_contig_ids, d_template_ids, n_reads, n_templates, contig_lengths,
                                     n_contigs, targets, d_keep_mask_out, stats, tstats, fstats);
}

}  // extern "C"
