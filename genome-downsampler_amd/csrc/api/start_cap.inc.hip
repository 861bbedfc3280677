// start_cap.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_start_cap_host / _device: every (contig, start, group) cell reduced to its best K reads -- priority
// descending, span descending, index ascending -- before the by-contig solve.
//   1. k_dd_range (groups as its tags, priorities as its qualities) validates every read and returns the ranges of group,
//      priority and span and the placed reads: the first host round trip (error word and ranges; a priority range above
//      65535 fails here, before anything is written)
//   2. dedup_plan.h turns the ranges into field widths, a sort form and its passes; k_sc_keys builds gstart | group -
//      group_min | prio_max - prio | span_max - span and dedup's stable sort orders them (the unplaced reads last)
//   3. head flags above the two low fields over the placed records, one exclusive scan, k_sc_heads (every cell's first
//      position), k_sc_rank (survivor and capped bits), k_dd_family_stats with K (histogram, counters)
//   4. word popcounts of the survivor mask and their scan; the second host round trip (survivor count, counters)
//   5. k_dd_compact, solve_by_contig_on_device on the survivors, k_expand_mask_reads back to input order
//   6. k_sc_kept_cells over the sorted records with the final mask: the cells in use, the largest kept pile
//   7. under QMCP_START_CAP_SHORTFALL the depth report's pass over ALL placed reads and the final mask: its deficit
//      against min(cov, M) is the shortfall (rows per contig come back, nothing per position)
// Every buffer of the pass is its own (sc_*): neither solve_by_contig_on_device nor a solve below it touches them.  The
// host entry's columns go to in_starts / in_ends / in_aux0 (ids) / in_aux1 (priorities) / sc_groups, its masks to mask
// and sc_capm.
namespace {

int solve_start_cap_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                              const uint32_t* d_groups, const uint32_t* d_prio, uint64_t n64, const uint32_t* lengths,
                              uint32_t n_contigs, uint32_t M, uint32_t cap, uint32_t flags, const DepthCall& dc,
                              uint64_t* d_mask, uint64_t* d_capped, uint64_t* hist_out, uint32_t hist_bins,
                              qmcp_hip_stats* stats, qmcp_hip_start_cap_stats* cstats) {
    const uint32_t n = (uint32_t)n64;
    const size_t words = (size_t)((n64 + 63) / 64);
    hipStream_t st = c->stream;
    qmcp_hip_start_cap_stats cs;
    std::memset(&cs, 0, sizeof(cs));
    cs.cap = cap;
    if (n == 0) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        if (hist_out) std::memset(hist_out, 0, (size_t)hist_bins * sizeof(uint64_t));
        if (cstats) *cstats = cs;
        return QMCP_OK;
    }
    EventPair ev_a(c), ev_b(c), ev_c(c);
    if (!ev_a.a || !ev_a.b || !ev_b.a || !ev_b.b || !ev_c.a || !ev_c.b) return fail(QMCP_EHIP, "event creation failed");

    // 1. ranges and validation
    const size_t tab = (size_t)n_contigs + 1;
    std::vector<uint64_t> poff(tab, 0);
    for (uint32_t k = 0; k < n_contigs; ++k) poff[k + 1] = poff[k] + lengths[k];
    const uint64_t ltot = poff[n_contigs];
    TRY(ensure(c, c->sc_tab, tab * sizeof(uint64_t) + (size_t)n_contigs * sizeof(uint32_t)));
    TRY(ensure(c, c->sc_stat, 16 * sizeof(uint64_t)));
    uint64_t* d_poff = c->sc_tab.u64();
    uint32_t* d_len = (uint32_t*)(d_poff + tab);
    uint32_t* d_range = c->sc_stat.u32();         // 9 words (of 16)
    uint64_t* d_counters = c->sc_stat.u64() + 8;  // cells, reads capped, largest cell, cells over K | cells kept, largest
    HIP_TRY(hipMemcpyAsync(d_poff, poff.data(), tab * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_len, lengths, (size_t)n_contigs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    uint32_t range[16] = {0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    HIP_TRY(hipMemcpyAsync(c->sc_stat.p, range, sizeof(range), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint64_t), st));
    HIP_TRY(hipEventRecord(ev_a.a, st));
    {
        KernelSpan sp(c, "k_dd_range(start cap)");
        qmcp::launch_dd_range(st, d_starts, d_ends, d_ids, d_groups, d_prio, n, d_len, n_contigs, false, d_range);
    }
    HIP_TRY(hipEventRecord(ev_a.b, st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(range, d_range, 9 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    if (range[6] & 1u) return fail(QMCP_EINVAL, "a contig id is neither < n_contigs (%u) nor QMCP_NO_CONTIG", n_contigs);
    if (range[6] & 2u) return fail(QMCP_EREAD, "a read has start > end or end >= its contig's length");
    const uint32_t g_lo = range[0], g_hi = range[1], p_lo = range[2], p_hi = range[3];
    const uint32_t span_lo = range[4], span_hi = range[5];
    const uint32_t n_placed = range[7];
    if (n_placed && p_hi - p_lo > 65535u) return fail(QMCP_ERANGE, "priority range %u..%u exceeds 65535", p_lo, p_hi);
    cs.reads_placed = n_placed;
    cs.ms_cap = elapsed(ev_a.a, ev_a.b);

    // buffers of the sort and of the segmented stage
    const uint32_t n_tiles = qmcp::sort_tiles(n);
    TRY(ensure(c, c->sc_bare, (size_t)n * sizeof(uint32_t)));
    TRY(ensure(c, c->sc_keys[0], (size_t)n * 8));
    TRY(ensure(c, c->sc_keys[1], (size_t)n * 8));
    TRY(ensure(c, c->sc_vals[0], (size_t)n * sizeof(uint32_t)));
    TRY(ensure(c, c->sc_vals[1], (size_t)n * sizeof(uint32_t)));
    TRY(ensure(c, c->sc_hist, (size_t)256 * n_tiles * sizeof(uint32_t)));
    const uint32_t spine_n = std::max(std::max(256u * n_tiles, n + 1), (uint32_t)words + 1);
    TRY(ensure(c, c->sc_spine, scan_spine_bytes(spine_n, 1)));
    TRY(ensure(c, c->sc_flag, ((size_t)n + 2) * sizeof(uint32_t)));
    TRY(ensure(c, c->sc_head, ((size_t)n + 2) * sizeof(uint32_t)));
    TRY(ensure(c, c->sc_cnt, ((size_t)n + 2) * sizeof(uint32_t)));
    TRY(ensure(c, c->sc_surv, words * 8 + 16));
    TRY(ensure(c, c->sc_words, (words + 2) * sizeof(uint32_t)));
    TRY(ensure(c, c->sc_histo, (size_t)std::max(hist_bins, 1u) * sizeof(uint64_t)));
    uint32_t* flag = c->sc_flag.u32();
    uint32_t* headpos = c->sc_head.u32();
    uint64_t* surv = c->sc_surv.u64();

    HIP_TRY(hipEventRecord(ev_b.a, st));
    HIP_TRY(hipMemsetAsync(surv, 0, words * 8, st));
    if (d_capped) HIP_TRY(hipMemsetAsync(d_capped, 0, words * 8, st));
    if (hist_bins) HIP_TRY(hipMemsetAsync(c->sc_histo.p, 0, (size_t)hist_bins * sizeof(uint64_t), st));

    // 2. keys and sort: {span_max - span, prio_max - prio, group - group_min, gstart}
    uint32_t bits[4];
    qmcp::dedup_read_fields(ltot, span_lo, span_hi, g_lo, g_hi, p_lo, p_hi, true, bits);
    std::swap(bits[0], bits[2]);  // (dedup's order is quality, tag, span: the cap's is span, priority, group)
    std::swap(bits[1], bits[2]);
    const qmcp::DedupSortPlan plan = qmcp::plan_dedup_sort(bits, 4);
    const uint32_t span_max = n_placed ? span_hi : 0u, g_min = n_placed ? g_lo : 0u, p_max = n_placed ? p_hi : 0u;
    DedupSorted sorted;
    const DedupSortBufs bufs{c->sc_bare, c->sc_keys, c->sc_vals, c->sc_hist, c->sc_spine};
    TRY(dedup_sort(c, bufs, n, plan,
                   [&](uint32_t r, uint32_t key_bytes, const uint32_t* idx, void* keys) {
                       KernelSpan sp(c, "k_sc_keys");
                       qmcp::launch_sc_keys(st, key_bytes, d_starts, d_ends, d_ids, d_groups, d_prio, idx, d_poff, ltot, n,
                                            span_max, p_max, g_min, plan.rounds[r].pack, keys);
                   },
                   sorted));
    cs.key_bits = plan.key_bits;
    cs.sort_passes = plan.passes;
    HIP_TRY(hipGetLastError());

    // 3. cells, ranks and masks
    {
        KernelSpan sp(c, "k_dd_heads(start cap)");
        qmcp::launch_sc_cell_flags(st, sorted.form, sorted.keys, sorted.vals, bits[0] + bits[1], n_placed, d_starts, d_ids,
                                   d_groups, flag);
    }
    if (n_placed) {
        KernelSpan sp(c, "scan_heads(start cap, 3 kernels)");
        qmcp::launch_exclusive_scan(st, flag, n_placed, flag, c->sc_spine.u32(), true);
    }
    {
        KernelSpan sp(c, "k_sc_heads");
        qmcp::launch_sc_heads(st, flag, n_placed, headpos);
    }
    {
        KernelSpan sp(c, "k_sc_rank");
        qmcp::launch_sc_rank(st, sorted.vals, sorted.stride, flag, headpos, n_placed, cap, surv, d_capped);
    }
    {
        KernelSpan sp(c, "k_dd_family_stats(start cap)");
        qmcp::launch_dd_family_stats(st, headpos, flag + n_placed, n_placed, cap, hist_bins, c->sc_histo.u64(), d_counters);
    }
    // 4. the survivors' count
    {
        KernelSpan sp(c, "count survivors(popcounts, scan)");
        queue_mask_ranks(st, surv, (uint32_t)words, c->sc_words, c->sc_spine);
    }
    HIP_TRY(hipEventRecord(ev_b.b, st));
    HIP_TRY(hipGetLastError());
    uint32_t n_surv = 0;
    uint64_t counters[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(&n_surv, c->sc_words.u32() + words, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost, st));
    if (hist_out && hist_bins)
        HIP_TRY(hipMemcpyAsync(hist_out, c->sc_histo.p, (size_t)hist_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    cs.cells = counters[0];
    cs.reads_capped = counters[1];
    cs.largest_cell = counters[2];
    cs.cells_over_cap = counters[3];
    cs.reads_survived = n_surv;
    cs.ms_cap += elapsed(ev_b.a, ev_b.b);

    // 5. the solve of the survivors, back to input order
    qmcp_hip_stats plain;
    std::memset(&plain, 0, sizeof(plain));
    if (n_surv) {
        const size_t cb = (size_t)n_surv * sizeof(uint32_t);
        TRY(ensure(c, c->sc_cs, cb));
        TRY(ensure(c, c->sc_ce, cb));
        TRY(ensure(c, c->sc_ci, cb));
        TRY(ensure(c, c->sc_map, cb));
        TRY(ensure(c, c->sc_maskc, ((size_t)n_surv + 63) / 64 * 8 + 16));
        HIP_TRY(hipEventRecord(ev_c.a, st));
        {
            KernelSpan sp(c, "k_dd_compact(start cap)");
            qmcp::launch_dd_compact(st, d_starts, d_ends, d_ids, surv, c->sc_words.u32(), n, c->sc_cs.u32(),
                                    c->sc_ce.u32(), c->sc_ci.u32(), c->sc_map.u32());
        }
        HIP_TRY(hipEventRecord(ev_c.b, st));
        HIP_TRY(hipGetLastError());
        TRY(solve_by_contig_on_device(c, c->sc_cs.u32(), c->sc_ce.u32(), c->sc_ci.u32(), n_surv, lengths, n_contigs, M,
            c->sc_maskc.u64(), &plain));
        cs.ms_cap += elapsed(ev_c.a, ev_c.b);
    }
    HIP_TRY(hipEventRecord(ev_c.a, st));
    HIP_TRY(hipMemsetAsync(d_mask, 0, words * sizeof(uint64_t), st));
    if (n_surv) {
        KernelSpan sp(c, "k_expand_mask_reads(start cap)");
        qmcp::launch_expand_mask_reads(st, c->sc_maskc.u64(), c->sc_map.u32(), n_surv, d_mask);
    }
    // 6. the cells the kept set uses
    if (n_surv) {
        HIP_TRY(hipMemsetAsync(c->sc_cnt.p, 0, (size_t)cs.cells * sizeof(uint32_t), st));
        KernelSpan sp(c, "k_sc_kept_cells");
        qmcp::launch_sc_kept_cells(st, sorted.vals, sorted.stride, flag, n_placed, d_mask, c->sc_cnt.u32(), d_counters + 4);
    }
    HIP_TRY(hipEventRecord(ev_c.b, st));
    HIP_TRY(hipGetLastError());
    uint64_t kept[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(kept, d_counters + 4, sizeof(kept), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    cs.cells_kept = kept[0];
    cs.largest_kept_cell = kept[1];
    cs.ms_cap += elapsed(ev_c.a, ev_c.b);

    // 7. the shortfall against the demand of all placed reads
    if (flags & QMCP_START_CAP_SHORTFALL) {
        std::vector<qmcp_hip_depth_row> rows(n_contigs);
        qmcp_hip_depth_stats ds;
        TRY(depth_report_on_device(c, d_starts, d_ends, d_ids, d_mask, n64, lengths, n_contigs, M, dc, 0, rows.data(),
                                   nullptr, nullptr, nullptr, nullptr, &ds));
        cs.short_positions = ds.deficit_positions;
        for (const qmcp_hip_depth_row& r : rows) cs.short_bases += r.deficit_sum;
        cs.ms_cap += ds.ms_report;
    }
    if (stats) *stats = plain;
    if (cstats) *cstats = cs;
    return QMCP_OK;
}

// the checks both entries make before anything is copied or launched; dc: the shortfall pass's position batches
int check_start_cap_call(uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t cap, uint32_t flags,
                         const uint64_t* hist_out, uint32_t hist_bins, DepthCall& dc) {
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    if (!contig_lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    if (cap == 0) return fail(QMCP_EINVAL, "cap must be at least 1");
    if (flags & ~QMCP_START_CAP_SHORTFALL) return fail(QMCP_EINVAL, "unknown flag bits 0x%x", flags);
    if (hist_bins && !hist_out) return fail(QMCP_EINVAL, "hist_out missing");
    if (hist_bins > qmcp::dedup_hist_max())
        return fail(QMCP_ERANGE, "hist_bins %u exceeds %u", hist_bins, qmcp::dedup_hist_max());
    if (flags & QMCP_START_CAP_SHORTFALL)
        TRY(check_depth_call(n_reads, false, contig_lengths, n_contigs, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, dc));
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_start_cap_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                  const uint32_t* groups, const uint32_t* priorities, uint64_t n_reads,
                                  const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage, uint32_t cap,
                                  uint32_t flags, uint64_t* keep_mask_out, uint64_t* capped_mask_out, uint64_t* hist_out,
                                  uint32_t hist_bins, qmcp_hip_stats* stats, qmcp_hip_start_cap_stats* cstats) {
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    DepthCall dc;
    TRY(check_start_cap_call(n_reads, contig_lengths, n_contigs, cap, flags, hist_out, hist_bins, dc));
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    if (priorities) TRY(ensure(c, c->in_aux1, nb));
    if (groups) TRY(ensure(c, c->sc_groups, nb));
    TRY(ensure(c, c->mask, words * sizeof(uint64_t)));
    if (capped_mask_out) TRY(ensure(c, c->sc_capm, words * sizeof(uint64_t)));
    c->mask_reads = 0;
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
        if (priorities) HIP_TRY(hipMemcpyAsync(c->in_aux1.p, priorities, nb, hipMemcpyHostToDevice, c->stream));
        if (groups) HIP_TRY(hipMemcpyAsync(c->sc_groups.p, groups, nb, hipMemcpyHostToDevice, c->stream));
    }
    TRY(solve_start_cap_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(),
        groups ? c->sc_groups.u32() : nullptr, priorities ? c->in_aux1.u32() : nullptr, n_reads, contig_lengths, n_contigs,
        max_coverage, cap, flags, dc, c->mask.u64(), capped_mask_out ? c->sc_capm.u64() : nullptr, hist_out, hist_bins,
        stats, cstats));
    if (words) {
        HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        if (capped_mask_out)
            HIP_TRY(hipMemcpyAsync(capped_mask_out, c->sc_capm.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                   c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_start_cap_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                    const uint32_t* d_contig_ids, const uint32_t* d_groups, const uint32_t* d_priorities,
                                    uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                    uint32_t max_coverage, uint32_t cap, uint32_t flags, uint64_t* d_keep_mask_out,
                                    uint64_t* d_capped_mask_out, uint64_t* hist_out, uint32_t hist_bins, void* hip_stream,
                                    qmcp_hip_stats* stats, qmcp_hip_start_cap_stats* cstats) {
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    DepthCall dc;
    TRY(check_start_cap_call(n_reads, contig_lengths, n_contigs, cap, flags, hist_out, hist_bins, dc));
    TRY(order_after(c, hip_stream));
    return solve_start_cap_on_device(c, d_starts, d_ends, d_contig_ids, d_groups, d_priorities, n_reads, contig_lengths,
                                     n_contigs, max_coverage, cap, flags, dc, d_keep_mask_out, d_capped_mask_out,
                                     hist_out, hist_bins, stats, cstats);
}

}  // extern "C"
