// amplicon_by_contig.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_filter_solve_by_contig_host: pairs of reads on several contigs, one contig id per read, FILTERed against the
// amplicons of their own contig and solved one contig at a time.
//   1. k_amplicon_filter_by_contig validates every read and writes one bit per surviving pair (amplicon_table.h's
//      predicate; without amplicons only the length / MAPQ filters)
//   2. stable compaction of the survivors: k_word_popcounts -> exclusive scan -> k_compact_pairs_ids (ids carried along)
//   3. solve_by_contig_on_device on the compacted columns: survivors keep input order and the grouping is stable, so
//      each contig is solved on its own survivors in input order
//   4. optional k_complete_pairs on the compact mask, 5. k_expand_mask back to the original read indices
// Buffers: the columns go to in_starts / in_ends, lengths and qualities to in_aux0 / in_aux1 as in
// qmcp_hip_filter_solve_host, the ids to af_ids; the compacted columns to f_starts / f_ends / af_ids_c with f_map, the
// compact mask to cov, the final mask to mask.  solve_by_contig_on_device touches only the bc_* buffers, the spine and
// what solve_on_device owns -- none of these.
extern "C" {

int qmcp_hip_filter_solve_by_contig_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends,
                                         const uint32_t* contig_ids, const uint32_t* seq_lengths,
                                         const uint32_t* qualities, uint64_t n_reads, const uint32_t* contig_lengths,
                                         uint32_t n_contigs, const uint32_t* amp_offsets, const uint32_t* amp_starts,
                                         const uint32_t* amp_ends, uint32_t min_length, uint32_t min_mapq,
                                         uint32_t max_coverage, int complete_pairs, uint64_t* keep_mask_out,
                                         uint64_t* pairs_filtered_out, qmcp_hip_stats* stats) {
    TRY(use_device(c));
    if (pairs_filtered_out) *pairs_filtered_out = 0;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n_reads & 1ull) return fail(QMCP_EINVAL, "n_reads must be even (reads come in mate pairs)");
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    if (!contig_lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    // the amplicon table (host side: checked, sorted per contig, running maxima)
    std::vector<uint32_t> tab_starts, tab_pmax;
    uint32_t n_amp = 0;
    if (amp_offsets) {
        n_amp = amp_offsets[n_contigs];
        if (qmcp::check_amplicon_offsets(amp_offsets, n_contigs, n_amp) != QMCP_OK)
            return fail(QMCP_EINVAL, "amp_offsets must start at 0 and never decrease (%u contigs)", n_contigs);
        if (n_amp && (!amp_starts || !amp_ends)) return fail(QMCP_EINVAL, "null amplicon table");
        TRY(qmcp::build_amplicon_table(amp_offsets, amp_starts, amp_ends, n_contigs, tab_starts, tab_pmax));
    }
    if (n_reads == 0) {
        c->mask_reads = 0;
        return QMCP_OK;
    }
    const uint64_t n_pairs = n_reads / 2;
    const size_t words = (size_t)((n_reads + 63) / 64);
    const size_t pwords = (size_t)((n_pairs + 63) / 64);
    const size_t nb = (size_t)n_reads * 4;
    hipStream_t st = c->stream;
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->af_ids, nb));
    TRY(ensure(c, c->f_starts, nb));
    TRY(ensure(c, c->f_ends, nb));
    TRY(ensure(c, c->af_ids_c, nb));
    TRY(ensure(c, c->f_map, (size_t)n_pairs * 4 + 16));
    TRY(ensure(c, c->f_words, (pwords + 2) * 4));
    TRY(ensure(c, c->f_mask, pwords * 8 + 16));
    TRY(ensure(c, c->mask, words * 8));
    TRY(ensure(c, c->cov, words * 8 + 16));  // compact-index keep mask
    TRY(ensure(c, c->spine, scan_spine_bytes((uint32_t)pwords + 1, 1)));
    TRY(ensure(c, c->af_len, (size_t)n_contigs * 4));
    TRY(ensure(c, c->af_err, 16));
    TRY(ensure(c, c->af_tab, ((size_t)n_contigs + 1 + 2 * (size_t)n_amp) * 4));
    c->mask_reads = 0;
    HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->af_ids.p, contig_ids, nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->af_len.p, contig_lengths, (size_t)n_contigs * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(c->af_err.p, 0, sizeof(uint32_t), st));
    const uint32_t* d_len = nullptr;
    const uint32_t* d_q = nullptr;
    if (seq_lengths) {
        TRY(ensure(c, c->in_aux0, nb));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, seq_lengths, nb, hipMemcpyHostToDevice, st));
        d_len = c->in_aux0.u32();
    }
    if (qualities) {
        TRY(ensure(c, c->in_aux1, nb));
        HIP_TRY(hipMemcpyAsync(c->in_aux1.p, qualities, nb, hipMemcpyHostToDevice, st));
        d_q = c->in_aux1.u32();
    }
    uint32_t* d_offs = nullptr;
    uint32_t* d_tab_s = nullptr;
    uint32_t* d_tab_p = nullptr;
    if (amp_offsets) {
        d_offs = c->af_tab.u32();
        d_tab_s = d_offs + n_contigs + 1;
        d_tab_p = d_tab_s + n_amp;
        HIP_TRY(hipMemcpyAsync(d_offs, amp_offsets, ((size_t)n_contigs + 1) * 4, hipMemcpyHostToDevice, st));
        if (n_amp) {
            HIP_TRY(hipMemcpyAsync(d_tab_s, tab_starts.data(), (size_t)n_amp * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_tab_p, tab_pmax.data(), (size_t)n_amp * 4, hipMemcpyHostToDevice, st));
        }
    }
    // 1. FILTER + validation
    {
        KernelSpan sp(c, "k_amplicon_filter_by_contig");
        qmcp::launch_amplicon_filter_by_contig(st, c->in_starts.u32(), c->in_ends.u32(), c->af_ids.u32(), d_len, d_q,
                                               n_pairs, c->af_len.u32(), n_contigs, d_offs, d_tab_s, d_tab_p, n_amp,
                                               min_length, min_mapq, c->f_mask.u64(), c->af_err.u32());
    }
    // 2. compaction
    {
        KernelSpan sp(c, "compact survivors(popcounts, scan)");
        queue_mask_ranks(st, c->f_mask.u64(), (uint32_t)pwords, c->f_words, c->spine);
    }
    HIP_TRY(hipGetLastError());
    uint32_t err = 0, n_surv_pairs = 0;
    HIP_TRY(hipMemcpyAsync(&n_surv_pairs, c->f_words.u32() + pwords, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&err, c->af_err.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    if (err & 1u) return fail(QMCP_EINVAL, "a contig id is neither < n_contigs (%u) nor QMCP_NO_CONTIG", n_contigs);
    if (err & 2u) return fail(QMCP_EREAD, "a read has start > end or end >= its contig's length");
    {
        KernelSpan sp(c, "k_compact_pairs_ids");
        qmcp::launch_compact_pairs_ids(st, c->in_starts.u32(), c->in_ends.u32(), c->af_ids.u32(), c->f_mask.u64(),
                                       c->f_words.u32(), n_pairs, c->f_starts.u32(), c->f_ends.u32(), c->af_ids_c.u32(),
                                       c->f_map.u32());
    }
    HIP_TRY(hipGetLastError());
    // 3. the by-contig solve of the survivors, 4. mates, 5. back to the original indices
    const uint64_t n_c = 2ull * n_surv_pairs;
    uint64_t* d_mask_c = c->cov.u64();
    TRY(solve_by_contig_on_device(c, c->f_starts.u32(), c->f_ends.u32(), c->af_ids_c.u32(), n_c, contig_lengths,
        n_contigs, max_coverage, d_mask_c, stats));
    const uint32_t words_c = (uint32_t)((n_c + 63) / 64);
    if (complete_pairs && words_c) {
        KernelSpan sp(c, "k_complete_pairs");
        qmcp::launch_complete_pairs(st, d_mask_c, words_c, n_c);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(c->mask.p, 0, words * 8, st));
    if (n_c) {
        KernelSpan sp(c, "k_expand_mask");
        qmcp::launch_expand_mask(st, d_mask_c, c->f_map.u32(), (uint32_t)n_c, c->mask.u64());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    if (pairs_filtered_out) *pairs_filtered_out = n_pairs - n_surv_pairs;
    c->mask_reads = n_reads;
    return QMCP_OK;
}

}  // extern "C"
