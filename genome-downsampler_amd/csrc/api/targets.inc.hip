// targets.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_targets_host / _device: coverage capped at M inside target regions only.  The constraints
// "cov_kept(p) >= min(cov(p), M) for every target position p of contig c" are, one for one, the ordinary constraints of
// the reads projected onto the compressed axis of c's target positions (target_table.h), so the call is the ordinary
// by-contig solve of the projected on-target reads:
//   1. target_table.h builds the table on the host (a bad table fails here, before anything is copied or launched)
//   2. k_target_project validates every read, projects it, and writes one bit per on-target read and one per placed
//      off-target read
//   3. stable compaction of the on-target reads: k_word_popcounts -> exclusive scan -> k_compact_reads, the contig ids
//      renumbered over the contigs that have target positions (the solve never sees a contig of length 0)
//   4. solve_by_contig_on_device on the compacted columns with contig lengths |T_c|; with qualities, the quality pass on
//      the same projected problem (a cell: reads of one contig with equal projected interval)
//   5. k_expand_mask_reads back to input order; QMCP_TARGETS_KEEP_OFF_TARGET ORs the placed off-target reads in
// Buffers: the projections in tg_ps / tg_pe, the off-target mask in tg_off (its scanned popcounts in tg_offw), the table
// in tg_tab, the compacted qualities in tg_q; the compaction reuses the FILTER pipeline's f_mask (on-target bits), f_words,
// f_starts / f_ends / af_ids_c (compacted columns), f_map (input index per compact read), af_err and cov (compact
// mask).  The host entry's columns go to in_starts / in_ends / in_aux0 (ids) / in_aux1 (qualities).  Neither
// solve_by_contig_on_device nor quality_pass touches any of these.
namespace {

int solve_targets_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                            const uint32_t* d_q, uint64_t n64, const uint32_t* lengths, uint32_t n_contigs,
                            const qmcp::TargetTable& tab, uint32_t M, uint32_t flags, uint64_t* d_mask,
                            qmcp_hip_stats* stats, qmcp_hip_target_stats* tstats) {
    qmcp_hip_target_stats ts;
    std::memset(&ts, 0, sizeof(ts));
    ts.target_positions = tab.positions;
    ts.regions_in = tab.regions_in;
    ts.regions_merged = tab.regions_merged;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (tstats) *tstats = ts;
    const uint32_t n = (uint32_t)n64;
    const size_t words = (size_t)((n64 + 63) / 64);
    hipStream_t st = c->stream;
    if (n == 0) return QMCP_OK;
    // the contigs that have target positions, renumbered in id order
    std::vector<uint32_t> remap(n_contigs, QMCP_NO_CONTIG), tlen;
    for (uint32_t k = 0; k < n_contigs; ++k)
        if (tab.tlen[k]) {
            remap[k] = (uint32_t)tlen.size();
            tlen.push_back(tab.tlen[k]);
        }
    const uint32_t n_reg = tab.regions_merged;
    const size_t nb = (size_t)n * sizeof(uint32_t);
    TRY(ensure(c, c->tg_ps, nb + 16));
    TRY(ensure(c, c->tg_pe, nb + 16));
    TRY(ensure(c, c->f_mask, words * 8 + 16));
    TRY(ensure(c, c->tg_off, words * 8 + 16));
    TRY(ensure(c, c->f_words, (words + 2) * 4));
    TRY(ensure(c, c->tg_offw, (words + 2) * 4));
    TRY(ensure(c, c->spine, scan_spine_bytes((uint32_t)words + 1, 1)));
    TRY(ensure(c, c->af_err, 16));
    // the table: lengths | offs | remap | rs | re | cum
    const size_t tab_words = 3 * (size_t)n_contigs + 1 + 3 * (size_t)n_reg;
    TRY(ensure(c, c->tg_tab, tab_words * 4));
    uint32_t* d_len = c->tg_tab.u32();
    uint32_t* d_offs = d_len + n_contigs;
    uint32_t* d_remap = d_offs + n_contigs + 1;
    uint32_t* d_rs = d_remap + n_contigs;
    uint32_t* d_re = d_rs + n_reg;
    uint32_t* d_cum = d_re + n_reg;
    EventPair ev_a(c), ev_b(c), ev_c(c);
    if (!ev_a.a || !ev_a.b || !ev_b.a || !ev_b.b || !ev_c.a || !ev_c.b) return fail(QMCP_EHIP, "event creation failed");
    // (the mask is cleared before the reads are validated, as solve_by_contig_on_device does)
    HIP_TRY(hipMemsetAsync(d_mask, 0, words * sizeof(uint64_t), st));
    HIP_TRY(hipMemsetAsync(c->af_err.p, 0, sizeof(uint32_t), st));
    HIP_TRY(hipMemcpyAsync(d_len, lengths, (size_t)n_contigs * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_offs, tab.offs.data(), ((size_t)n_contigs + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_remap, remap.data(), (size_t)n_contigs * 4, hipMemcpyHostToDevice, st));
    if (n_reg) {
        HIP_TRY(hipMemcpyAsync(d_rs, tab.rs.data(), (size_t)n_reg * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_re, tab.re.data(), (size_t)n_reg * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_cum, tab.cum.data(), (size_t)n_reg * 4, hipMemcpyHostToDevice, st));
    }
    // 2. validation + projection, and the counts of both masks
    HIP_TRY(hipEventRecord(ev_a.a, st));
    {
        KernelSpan sp(c, "k_target_project");
        qmcp::launch_target_project(st, d_starts, d_ends, d_ids, n, d_len, n_contigs, d_offs, d_rs, d_re, d_cum, n_reg,
                                    c->tg_ps.u32(), c->tg_pe.u32(), c->f_mask.u64(), c->tg_off.u64(), c->af_err.u32());
    }
    {
        KernelSpan sp(c, "count targets(2 x popcounts, scan)");
        queue_mask_ranks(st, c->f_mask.u64(), (uint32_t)words, c->f_words, c->spine);
        queue_mask_ranks(st, c->tg_off.u64(), (uint32_t)words, c->tg_offw, c->spine);
    }
    HIP_TRY(hipEventRecord(ev_a.b, st));
    HIP_TRY(hipGetLastError());
    uint32_t err = 0, n_on = 0, n_off = 0;
    HIP_TRY(hipMemcpyAsync(&n_on, c->f_words.u32() + words, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&n_off, c->tg_offw.u32() + words, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&err, c->af_err.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    if (err & 1u) return fail(QMCP_EINVAL, "a contig id is neither < n_contigs (%u) nor QMCP_NO_CONTIG", n_contigs);
    if (err & 2u) return fail(QMCP_EREAD, "a read has start > end or end >= its contig's length");
    ts.reads_on_target = n_on;
    ts.reads_off_target = n_off;
    ts.ms_targets = elapsed(ev_a.a, ev_a.b);
    if (n_on) {
        // 3. compaction
        const size_t cb = (size_t)n_on * sizeof(uint32_t);
        const size_t words_c = ((size_t)n_on + 63) / 64;
        TRY(ensure(c, c->f_starts, cb));
        TRY(ensure(c, c->f_ends, cb));
        TRY(ensure(c, c->af_ids_c, cb));
        TRY(ensure(c, c->f_map, cb));
        if (d_q) TRY(ensure(c, c->tg_q, cb));
        TRY(ensure(c, c->cov, words_c * 8 + 16));
        HIP_TRY(hipEventRecord(ev_b.a, st));
        {
            KernelSpan sp(c, "k_compact_reads");
            qmcp::launch_compact_reads(st, c->tg_ps.u32(), c->tg_pe.u32(), d_ids, d_q, d_remap, c->f_mask.u64(),
                                       c->f_words.u32(), n, c->f_starts.u32(), c->f_ends.u32(), c->af_ids_c.u32(),
                                       d_q ? c->tg_q.u32() : nullptr, c->f_map.u32());
        }
        HIP_TRY(hipEventRecord(ev_b.b, st));
        HIP_TRY(hipGetLastError());
        // 4. the projected problem
        const uint32_t* cs = c->f_starts.u32();
        const uint32_t* ce = c->f_ends.u32();
        const uint32_t* cid = c->af_ids_c.u32();
        uint64_t* d_mask_c = c->cov.u64();
        const uint32_t n_tc = (uint32_t)tlen.size();
        QualityRange qr;
        if (d_q) TRY(quality_range(c, c->tg_q.u32(), cid, n_on, qr));
        qmcp_hip_stats plain;
        std::memset(&plain, 0, sizeof(plain));
        TRY(solve_by_contig_on_device(c, cs, ce, cid, n_on, tlen.data(), n_tc, M, d_mask_c, &plain));
        if (d_q)
            TRY(quality_pass(c, cs, ce, c->tg_q.u32(), cid, n_on, nullptr, tlen.data(), n_tc, qr, plain,
                             d_mask_c, nullptr));
        if (stats) *stats = plain;
        // 5. back to input order
        HIP_TRY(hipEventRecord(ev_c.a, st));
        {
            KernelSpan sp(c, "k_expand_mask_reads");
            qmcp::launch_expand_mask_reads(st, d_mask_c, c->f_map.u32(), n_on, d_mask);
        }
    } else {
        HIP_TRY(hipEventRecord(ev_b.a, st));
        HIP_TRY(hipEventRecord(ev_b.b, st));
        HIP_TRY(hipEventRecord(ev_c.a, st));
    }
    if ((flags & QMCP_TARGETS_KEEP_OFF_TARGET) && n_off) {
        KernelSpan sp(c, "k_or_words(off-target reads)");
        qmcp::launch_or_words(st, d_mask, c->tg_off.u64(), (uint32_t)words);
    }
    HIP_TRY(hipEventRecord(ev_c.b, st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    ts.ms_targets += elapsed(ev_b.a, ev_b.b) + elapsed(ev_c.a, ev_c.b);
    if (tstats) *tstats = ts;
    return QMCP_OK;
}

// the checks both entries make before anything is copied or launched, and the table
int check_targets_call(uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, const uint32_t* target_offsets,
                       const uint32_t* target_starts, const uint32_t* target_ends, uint32_t padding, uint32_t flags,
                       qmcp::TargetTable& tab) {
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    if (!contig_lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    if (flags & ~QMCP_TARGETS_KEEP_OFF_TARGET) return fail(QMCP_EINVAL, "unknown flag bits 0x%x", flags);
    if (!target_offsets) return fail(QMCP_EINVAL, "target_offsets missing");
    if (qmcp::check_target_offsets(target_offsets, n_contigs) != QMCP_OK)
        return fail(QMCP_EINVAL, "target_offsets must start at 0 and never decrease (%u contigs)", n_contigs);
    if (target_offsets[n_contigs] && (!target_starts || !target_ends)) return fail(QMCP_EINVAL, "null target table");
    if (qmcp::build_target_table(target_offsets, target_starts, target_ends, padding, contig_lengths, n_contigs, tab) !=
        QMCP_OK)
        return fail(QMCP_EINVAL, "a target region has start > end");
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_targets_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                const uint32_t* qualities, uint64_t n_reads, const uint32_t* contig_lengths,
                                uint32_t n_contigs, const uint32_t* target_offsets, const uint32_t* target_starts,
                                const uint32_t* target_ends, uint32_t padding, uint32_t max_coverage, uint32_t flags,
                                uint64_t* keep_mask_out, qmcp_hip_stats* stats, qmcp_hip_target_stats* tstats) {
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    qmcp::TargetTable tab;
    TRY(check_targets_call(n_reads, contig_lengths, n_contigs, target_offsets, target_starts, target_ends, padding, flags,
                           tab));
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    if (qualities) TRY(ensure(c, c->in_aux1, nb));
    TRY(ensure(c, c->mask, words * sizeof(uint64_t)));
    c->mask_reads = 0;
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
        if (qualities) HIP_TRY(hipMemcpyAsync(c->in_aux1.p, qualities, nb, hipMemcpyHostToDevice, c->stream));
    }
    TRY(solve_targets_on_device(c, c->in_starts.u32(), c->in_ends.u32(),
                                c->in_aux0.u32(), qualities ? c->in_aux1.u32() : nullptr, n_reads,
                                contig_lengths, n_contigs, tab, max_coverage, flags, c->mask.u64(), stats, tstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_targets_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                  const uint32_t* d_contig_ids, const uint32_t* d_qualities, uint64_t n_reads,
                                  const uint32_t* contig_lengths, uint32_t n_contigs, const uint32_t* target_offsets,
                                  const uint32_t* target_starts, const uint32_t* target_ends, uint32_t padding,
                                  uint32_t max_coverage, uint32_t flags, uint64_t* d_keep_mask_out, void* hip_stream,
                                  qmcp_hip_stats* stats, qmcp_hip_target_stats* tstats) {
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    qmcp::TargetTable tab;
    TRY(check_targets_call(n_reads, contig_lengths, n_contigs, target_offsets, target_starts, target_ends, padding, flags,
                           tab));
    TRY(order_after(c, hip_stream));
    return solve_targets_on_device(c, d_starts, d_ends, d_contig_ids, d_qualities, n_reads, contig_lengths, n_contigs, tab,
                                   max_coverage, flags, d_keep_mask_out, stats, tstats);
}

}  // extern "C"
