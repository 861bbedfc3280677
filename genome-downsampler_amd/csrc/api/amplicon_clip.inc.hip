// amplicon_clip.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_amplicons_host / _device: every unit (a pair of reads, or one read) assigned to one amplicon of its
// contig, its reads clipped to that amplicon's insert, and the clipped reads solved -- pooled per contig, or one
// coverage problem per amplicon.
//   1. the checks and amplicon_assign.h's sorted table on the host, before anything is copied or launched
//   2. the table, the offsets and the contig lengths go to the device (the host entry's columns too)
//   3. k_amplicon_clip validates every read and writes the labels, one keep bit per unit and the clipped columns (the
//      rebased ones as well when the rows need them); k_ac_totals adds the blocks' counters
//   4. word popcounts of the unit mask and their scan; the one host round trip: error word, survivor count, counters
//   5. stable compaction of the surviving units with the ids carried along (k_compact_pairs_ids, or k_dd_compact for
//      single reads)
//   6. solve_by_contig_on_device on the compacted columns -- pooled: the contig lengths; per amplicon: the insert
//      lengths, the amplicon's index as contig id
//   7. optional k_complete_pairs on the compact mask, 8. k_expand_mask / k_expand_mask_reads back to input order
//   9. the rows: the depth report's pass over the rebased columns of ALL reads (unassigned and clipped-away reads are
//      unplaced there) with the final mask, one "contig" per amplicon of the insert's length
//  10. labels, rows and stats reach the caller's buffers only now
// Every buffer of the pass is its own (ac_*): neither solve_by_contig_on_device nor the depth report touches them.  The
// host entry's columns go to in_starts / in_ends / af_ids / in_aux0 (lengths) / in_aux1 (qualities), its mask to mask.
namespace {

struct AmpliconsCall {
    bool pairs = true, per_amplicon = false, complete = false, rows = false;
    uint32_t n_amp = 0;
    qmcp::AssignTable tab;
    std::vector<uint32_t> ins_start, ins_len;  // the inserts in the caller's table order: the rows' intervals and lengths
    DepthCall dc;
};

// everything that can be refused without a device
int check_amplicons_call(uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, const uint32_t* amp_offsets,
                         const uint32_t* amp_starts, const uint32_t* amp_ends, const uint32_t* ins_starts,
                         const uint32_t* ins_ends, uint32_t flags, bool want_rows, AmpliconsCall& ac) {
    const uint32_t known = QMCP_AMPLICONS_SINGLE_END | QMCP_AMPLICONS_PER_AMPLICON | QMCP_AMPLICONS_COMPLETE_PAIRS;
    if (flags & ~known) return fail(QMCP_EINVAL, "unknown flag bits 0x%x", flags);
    ac.pairs = !(flags & QMCP_AMPLICONS_SINGLE_END);
    ac.per_amplicon = (flags & QMCP_AMPLICONS_PER_AMPLICON) != 0;
    ac.complete = (flags & QMCP_AMPLICONS_COMPLETE_PAIRS) != 0;
    if (ac.complete && !ac.pairs) return fail(QMCP_EINVAL, "QMCP_AMPLICONS_COMPLETE_PAIRS needs pairs, not single reads");
    if (ac.pairs && (n_reads & 1ull)) return fail(QMCP_EINVAL, "n_reads must be even (reads come in mate pairs)");
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    if (!contig_lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    if (!amp_offsets) return fail(QMCP_EINVAL, "amp_offsets missing: this entry is about amplicons");
    const uint32_t n_amp = amp_offsets[n_contigs];
    ac.rows = want_rows && n_amp != 0;
    if ((ac.per_amplicon || want_rows) && n_amp > (1u << 24))
        return fail(QMCP_ERANGE, "%u amplicons exceed 2^24 per call (one coverage problem, or one row, each)", n_amp);
    uint64_t bad = 0;
    switch (qmcp::build_assign_table(amp_offsets, amp_starts, amp_ends, ins_starts, ins_ends, n_contigs, ac.tab, &bad)) {
        case qmcp::kAssignTableOk: break;
        case qmcp::kAssignTableOffsets:
            return fail(QMCP_EINVAL, "amp_offsets must start at 0 and never decrease (%u contigs)", n_contigs);
        case qmcp::kAssignTableNull: return fail(QMCP_EINVAL, "null amplicon table");
        case qmcp::kAssignTableInsertArrays:
            return fail(QMCP_EINVAL, "amp_insert_starts and amp_insert_ends go together");
        case qmcp::kAssignTableInsert:
            return fail(QMCP_EINVAL, "amplicon %llu: start <= insert_start <= insert_end <= end does not hold",
                        (unsigned long long)bad);
    }
    ac.n_amp = n_amp;
    ac.ins_start.resize(n_amp);
    ac.ins_len.resize(n_amp);
    for (uint32_t k = 0; k < n_amp; ++k) {
        const uint32_t ins_end = ins_ends ? ins_ends[k] : amp_ends[k];
        ac.ins_start[k] = ins_starts ? ins_starts[k] : amp_starts[k];
        if (ins_end == 0xFFFFFFFFu && ac.ins_start[k] == 0)
            return fail(QMCP_ERANGE, "amplicon %u: an insert of 2^32 positions", k);
        ac.ins_len[k] = ins_end - ac.ins_start[k] + 1;
    }
    if (ac.rows)
        TRY(check_depth_call(n_reads, false, ac.ins_len.data(), n_amp, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, ac.dc));
    return QMCP_OK;
}

int solve_amplicons_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                              const uint32_t* d_len, const uint32_t* d_q, uint64_t n_reads, const uint32_t* contig_lengths,
                              uint32_t n_contigs, const uint32_t* amp_offsets, uint32_t min_length, uint32_t min_mapq,
                              uint32_t M, const AmpliconsCall& ac, uint64_t* d_mask, uint32_t* amplicon_of_out,
                              qmcp_hip_depth_row* amplicon_rows, qmcp_hip_stats* stats, qmcp_hip_amplicons_stats* astats) {
    const uint32_t n_amp = ac.n_amp;
    const uint64_t n_units = ac.pairs ? n_reads / 2 : n_reads;
    qmcp_hip_amplicons_stats as;
    std::memset(&as, 0, sizeof(as));
    as.units = n_units;
    as.amplicons = n_amp;
    qmcp_hip_stats plain;
    std::memset(&plain, 0, sizeof(plain));
    std::vector<qmcp_hip_depth_row> rows(ac.rows ? n_amp : 0);
    auto finish_rows = [&]() {
        for (uint32_t k = 0; k < (uint32_t)rows.size(); ++k) {
            rows[k].contig = k;
            rows[k].start = ac.ins_start[k];
            rows[k].end = ac.ins_start[k] + (ac.ins_len[k] - 1);
            rows[k].positions = ac.ins_len[k];
        }
        if (amplicon_rows && !rows.empty()) std::memcpy(amplicon_rows, rows.data(), rows.size() * sizeof(rows[0]));
    };
    if (n_reads == 0) {
        as.amplicons_unused = n_amp;
        for (qmcp_hip_depth_row& r : rows) std::memset(&r, 0, sizeof(r));
        finish_rows();
        if (stats) *stats = plain;
        if (astats) *astats = as;
        return QMCP_OK;
    }
    const size_t words = (size_t)((n_reads + 63) / 64);
    const size_t uwords = (size_t)((n_units + 63) / 64);
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const bool rebased_too = ac.rows && !ac.per_amplicon;
    hipStream_t st = c->stream;
    EventPair ev(c);
    if (!ev.a || !ev.b) return fail(QMCP_EHIP, "event creation failed");
    // 2. tables: offsets | the sorted table | contig lengths
    const size_t tab_words = (size_t)n_contigs + 1 + 6 * (size_t)n_amp + n_contigs;
    TRY(ensure(c, c->ac_tab, tab_words * sizeof(uint32_t)));
    TRY(ensure(c, c->ac_label, (size_t)n_units * sizeof(uint32_t)));
    TRY(ensure(c, c->ac_keep, uwords * 8 + 16));
    TRY(ensure(c, c->ac_words, (uwords + 2) * sizeof(uint32_t)));
    TRY(ensure(c, c->ac_spine, scan_spine_bytes((uint32_t)uwords + 1, 1)));
    for (int k = 0; k < (rebased_too ? 6 : 3); ++k) TRY(ensure(c, c->ac_col[k], nb));
    for (int k = 0; k < 3; ++k) TRY(ensure(c, c->ac_comp[k], nb));
    TRY(ensure(c, c->ac_map, (size_t)n_units * sizeof(uint32_t) + 16));
    TRY(ensure(c, c->ac_maskc, words * 8 + 16));
    TRY(ensure(c, c->ac_used, (size_t)n_amp * sizeof(uint32_t)));
    TRY(ensure(c, c->ac_part, ((size_t)qmcp::ac_partial_rows() + 1) * qmcp::kAcCounts * sizeof(uint64_t)));
    TRY(ensure(c, c->ac_err, 16));
    uint32_t* d_offs = c->ac_tab.u32();
    uint32_t* d_tab = d_offs + n_contigs + 1;
    uint32_t* d_clen = d_tab + 6 * (size_t)n_amp;
    uint64_t* d_partials = c->ac_part.u64();
    uint64_t* d_totals = d_partials + (size_t)qmcp::ac_partial_rows() * qmcp::kAcCounts;
    uint32_t* cs = c->ac_col[0].u32();
    uint32_t* ce = c->ac_col[1].u32();
    uint32_t* ci = c->ac_col[2].u32();
    uint32_t* rs = rebased_too ? c->ac_col[3].u32() : nullptr;
    uint32_t* re = rebased_too ? c->ac_col[4].u32() : nullptr;
    uint32_t* ri = rebased_too ? c->ac_col[5].u32() : nullptr;
    HIP_TRY(hipMemcpyAsync(d_offs, amp_offsets, ((size_t)n_contigs + 1) * 4, hipMemcpyHostToDevice, st));
    if (n_amp) HIP_TRY(hipMemcpyAsync(d_tab, ac.tab.words.data(), 6 * (size_t)n_amp * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_clen, contig_lengths, (size_t)n_contigs * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(c->ac_err.p, 0, sizeof(uint32_t), st));
    if (n_amp) HIP_TRY(hipMemsetAsync(c->ac_used.p, 0, (size_t)n_amp * sizeof(uint32_t), st));
    // 3. assign and clip
    HIP_TRY(hipEventRecord(ev.a, st));
    {
        KernelSpan sp(c, "k_amplicon_clip");
        qmcp::launch_amplicon_clip(st, ac.pairs, d_starts, d_ends, d_ids, d_len, d_q, n_units, d_clen, n_contigs, d_offs,
                                   d_tab, n_amp, min_length, min_mapq, ac.per_amplicon, c->ac_label.u32(),
                                   c->ac_keep.u64(), cs, ce, ci, rs, re, ri, c->ac_used.u32(), d_partials, d_totals,
                                   c->ac_err.u32());
    }
    HIP_TRY(hipEventRecord(ev.b, st));
    // 4. the survivors' ranks; the round trip
    {
        KernelSpan sp(c, "compact units(popcounts, scan)");
        queue_mask_ranks(st, c->ac_keep.u64(), (uint32_t)uwords, c->ac_words, c->ac_spine);
    }
    HIP_TRY(hipGetLastError());
    uint32_t err = 0, n_surv = 0;
    uint64_t totals[qmcp::kAcCounts] = {0};
    HIP_TRY(hipMemcpyAsync(&n_surv, c->ac_words.u32() + uwords, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&err, c->ac_err.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(totals, d_totals, sizeof(totals), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    if (err & 1u) return fail(QMCP_EINVAL, "a contig id is neither < n_contigs (%u) nor QMCP_NO_CONTIG", n_contigs);
    if (err & 2u) return fail(QMCP_EREAD, "a read has start > end or end >= its contig's length");
    as.units_assigned = totals[qmcp::kAcAssigned];
    as.units_filtered = totals[qmcp::kAcFiltered];
    as.units_no_amplicon = totals[qmcp::kAcNoAmplicon];
    as.units_in_several = totals[qmcp::kAcSeveral];
    as.reads_shortened = totals[qmcp::kAcShortened];
    as.reads_clipped_away = totals[qmcp::kAcAway];
    as.bases_clipped = totals[qmcp::kAcBases];
    as.amplicons_unused = totals[qmcp::kAcUnused];
    as.ms_assign = elapsed(ev.a, ev.b);
    // 5. compaction
    uint32_t* fs = c->ac_comp[0].u32();
    uint32_t* fe = c->ac_comp[1].u32();
    uint32_t* fi = c->ac_comp[2].u32();
    if (n_surv) {
        KernelSpan sp(c, ac.pairs ? "k_compact_pairs_ids(amplicons)" : "k_dd_compact(amplicons)");
        if (ac.pairs)
            qmcp::launch_compact_pairs_ids(st, cs, ce, ci, c->ac_keep.u64(), c->ac_words.u32(), n_units, fs, fe, fi,
                                           c->ac_map.u32());
        else
            qmcp::launch_dd_compact(st, cs, ce, ci, c->ac_keep.u64(), c->ac_words.u32(), (uint32_t)n_units, fs, fe, fi,
                                    c->ac_map.u32());
    }
    HIP_TRY(hipGetLastError());
    // 6. the solve, 7. mates, 8. back to input order
    const uint64_t n_c = ac.pairs ? 2ull * n_surv : n_surv;
    uint64_t* d_mask_c = c->ac_maskc.u64();
    if (n_c) {
        if (ac.per_amplicon)
            TRY(solve_by_contig_on_device(c, fs, fe, fi, n_c, ac.ins_len.data(), n_amp, M, d_mask_c, &plain));
        else
            TRY(solve_by_contig_on_device(c, fs, fe, fi, n_c, contig_lengths, n_contigs, M, d_mask_c, &plain));
    }
    const uint32_t words_c = (uint32_t)((n_c + 63) / 64);
    if (ac.complete && words_c) {
        KernelSpan sp(c, "k_complete_pairs");
        qmcp::launch_complete_pairs(st, d_mask_c, words_c, n_c);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(d_mask, 0, words * 8, st));
    if (n_c) {
        KernelSpan sp(c, ac.pairs ? "k_expand_mask" : "k_expand_mask_reads(amplicons)");
        if (ac.pairs) qmcp::launch_expand_mask(st, d_mask_c, c->ac_map.u32(), (uint32_t)n_c, d_mask);
        else qmcp::launch_expand_mask_reads(st, d_mask_c, c->ac_map.u32(), (uint32_t)n_c, d_mask);
    }
    HIP_TRY(hipGetLastError());
    // 9. the rows
    if (ac.rows) {
        qmcp_hip_depth_stats ds;
        TRY(depth_report_on_device(c, ac.per_amplicon ? cs : rs, ac.per_amplicon ? ce : re, ac.per_amplicon ? ci : ri,
                                   d_mask, n_reads, ac.ins_len.data(), n_amp, M, ac.dc, 0, rows.data(), nullptr, nullptr,
                                   nullptr, nullptr, &ds));
        as.ms_report = ds.ms_report;
    }
    // 10. outputs
    if (amplicon_of_out)
        HIP_TRY(hipMemcpyAsync(amplicon_of_out, c->ac_label.p, (size_t)n_units * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    finish_rows();
    if (stats) *stats = plain;
    if (astats) *astats = as;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_amplicons_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends,
                                  const uint32_t* contig_ids, const uint32_t* seq_lengths, const uint32_t* qualities,
                                  uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                  const uint32_t* amp_offsets, const uint32_t* amp_starts, const uint32_t* amp_ends,
                                  const uint32_t* amp_insert_starts, const uint32_t* amp_insert_ends, uint32_t min_length,
                                  uint32_t min_mapq, uint32_t max_coverage, uint32_t flags, uint64_t* keep_mask_out,
                                  uint32_t* amplicon_of_out, qmcp_hip_depth_row* amplicon_rows, qmcp_hip_stats* stats,
                                  qmcp_hip_amplicons_stats* astats) {
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    AmpliconsCall ac;
    TRY(check_amplicons_call(n_reads, contig_lengths, n_contigs, amp_offsets, amp_starts, amp_ends, amp_insert_starts,
                             amp_insert_ends, flags, amplicon_rows != nullptr, ac));
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->af_ids, nb));
    if (seq_lengths) TRY(ensure(c, c->in_aux0, nb));
    if (qualities) TRY(ensure(c, c->in_aux1, nb));
    TRY(ensure(c, c->mask, words * sizeof(uint64_t)));
    c->mask_reads = 0;
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->af_ids.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
        if (seq_lengths) HIP_TRY(hipMemcpyAsync(c->in_aux0.p, seq_lengths, nb, hipMemcpyHostToDevice, c->stream));
        if (qualities) HIP_TRY(hipMemcpyAsync(c->in_aux1.p, qualities, nb, hipMemcpyHostToDevice, c->stream));
    }
    TRY(solve_amplicons_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->af_ids.u32(),
                                  seq_lengths ? c->in_aux0.u32() : nullptr, qualities ? c->in_aux1.u32() : nullptr, n_reads,
                                  contig_lengths, n_contigs, amp_offsets, min_length, min_mapq, max_coverage, ac,
                                  c->mask.u64(), amplicon_of_out, amplicon_rows, stats, astats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_amplicons_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                    const uint32_t* d_contig_ids, const uint32_t* d_seq_lengths,
                                    const uint32_t* d_qualities, uint64_t n_reads, const uint32_t* contig_lengths,
                                    uint32_t n_contigs, const uint32_t* amp_offsets, const uint32_t* amp_starts,
                                    const uint32_t* amp_ends, const uint32_t* amp_insert_starts,
                                    const uint32_t* amp_insert_ends, uint32_t min_length, uint32_t min_mapq,
                                    uint32_t max_coverage, uint32_t flags, uint64_t* d_keep_mask_out,
                                    uint32_t* amplicon_of_out, qmcp_hip_depth_row* amplicon_rows, void* hip_stream,
                                    qmcp_hip_stats* stats, qmcp_hip_amplicons_stats* astats) {
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    AmpliconsCall ac;
    TRY(check_amplicons_call(n_reads, contig_lengths, n_contigs, amp_offsets, amp_starts, amp_ends, amp_insert_starts,
                             amp_insert_ends, flags, amplicon_rows != nullptr, ac));
    if (ac.pairs) {
        // the kernel reads a pair as one uint2
        const uintptr_t bits = (uintptr_t)d_starts | (uintptr_t)d_ends | (uintptr_t)d_contig_ids |
                               (uintptr_t)d_seq_lengths | (uintptr_t)d_qualities;
        if (bits & 7u) return fail(QMCP_EINVAL, "with pairs the device columns must be 8-byte aligned");
    }
    TRY(order_after(c, hip_stream));
    return solve_amplicons_on_device(c, d_starts, d_ends, d_contig_ids, d_seq_lengths, d_qualities, n_reads, contig_lengths,
                                     n_contigs, amp_offsets, min_length, min_mapq, max_coverage, ac, d_keep_mask_out,
                                     amplicon_of_out, amplicon_rows, stats, astats);
}

}  // extern "C"
