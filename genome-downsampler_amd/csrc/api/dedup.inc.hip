// dedup.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_dedup_host / _device: duplicate families collapsed to their representative before the by-contig solve.
//   1. k_dd_range validates every read and returns the ranges of tag, quality and span, the placed reads and the pairs
//      without a placed mate: the first host round trip (error word and ranges; a quality range above 65535 fails here,
//      before anything is written)
//   2. dedup_plan.h turns the ranges into field widths, a sort form and its passes; the keys are built and sorted by the
//      stable LSD radix of the sort-based route ({u32 key, index} records, split u64 keys, or one u64 sort per field)
//      read mode: the reads by gstart | span | tag | q_max - q
//      pair mode: the reads by gstart | span | tag, head flags -> scan -> dense cell ids back in input order; then the
//                 units by min id | max id | score_max - score
//   3. head flags over the active records (the placed reads / the units with a placed mate: they sort in front), one
//      exclusive scan, k_dd_segments (survivor and duplicate bits, family heads), k_dd_family_stats (histogram, counters)
//   4. word popcounts of the survivor mask and their scan; the second host round trip (survivor count, counters)
//   5. k_dd_compact, solve_by_contig_on_device on the survivors, k_expand_mask_reads back to input order, and
//      k_complete_pairs when asked
// Every buffer of the pass is its own (dd_*): neither solve_by_contig_on_device nor a solve below it touches them.  The host
// entry's columns go to in_starts / in_ends / in_aux0 (ids) / in_aux1 (qualities) / dd_tags, its masks to mask and dd_dupm.
namespace {

struct DedupSorted {
    uint32_t form = 0;
    const void* keys = nullptr;     // records (REC32) or u64 keys of the last round
    const uint32_t* vals = nullptr;  // the index column: vals[j * stride]
    uint32_t stride = 1;
};

// the buffers a sort works in: bare keys, two key buffers (records, or u64 keys), two index columns, histogram, spine
struct DedupSortBufs {
    const DevBuf& bare;
    const DevBuf* keys;
    const DevBuf* vals;
    const DevBuf& hist;
    const DevBuf& spine;
};

// the stable sort a plan describes, on n elements; build(round, key_bytes, idx, keys_out) queues the round's key kernel
template <typename Build>
int dedup_sort(qmcp_hip_ctx* c, const DedupSortBufs& b, uint32_t n, const qmcp::DedupSortPlan& plan, Build build,
               DedupSorted& out) {
    hipStream_t st = c->stream;
    uint32_t* hist = b.hist.u32();
    uint32_t* spine = b.spine.u32();
    out.form = plan.form;
    if (plan.form == qmcp::DEDUP_SORT_REC32) {
        build(0u, 4u, (const uint32_t*)nullptr, b.bare.p);
        int kin = 0;
        TRY(radix_sort_records(c, st, b.bare.u32(), n, plan.rounds[0].passes, hist, spine, b.keys,
                               {"k_radix_hist_rec(dedup)", "scan_radix_hist(dedup, 3 kernels)", "k_radix_scatter_rec(dedup)"},
                               &kin));
        out.keys = b.keys[kin].p;
        out.vals = b.keys[kin].u32() + 1;
        out.stride = 2;
        return QMCP_OK;
    }
    // one u64 sort per round; a later round's keys are built in the order the rounds before it left (the value column)
    WideBufs wb;
    for (uint32_t r = 0; r < plan.n_rounds; ++r) {
        build(r, 8u, wb.v < 0 ? (const uint32_t*)nullptr : b.vals[wb.v].u32(), b.keys[wb.k].p);
        TRY(radix_sort_wide(c, st, n, plan.rounds[r].passes, hist, spine, b.keys, b.vals,
                            {"k_radix_hist(dedup, u64)", "scan_radix_hist(dedup, 3 kernels)", "k_radix_scatter(dedup, u64)"},
                            &wb));
    }
    out.keys = b.keys[wb.k].p;
    out.vals = b.vals[wb.v].u32();
    out.stride = 1;
    return QMCP_OK;
}

int solve_dedup_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                          const uint32_t* d_tags, const uint32_t* d_q, uint64_t n64, const uint32_t* lengths,
                          uint32_t n_contigs, uint32_t M, uint32_t flags, uint64_t* d_mask, uint64_t* d_dup,
                          uint64_t* hist_out, uint32_t hist_bins, qmcp_hip_stats* stats, qmcp_hip_dedup_stats* dstats) {
    const bool pairs = (flags & QMCP_DEDUP_PAIRS) != 0;
    const uint32_t n = (uint32_t)n64;
    const size_t words = (size_t)((n64 + 63) / 64);
    hipStream_t st = c->stream;
    qmcp_hip_dedup_stats ds;
    std::memset(&ds, 0, sizeof(ds));
    if (n == 0) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        if (hist_out) std::memset(hist_out, 0, (size_t)hist_bins * sizeof(uint64_t));
        if (dstats) *dstats = ds;
        return QMCP_OK;
    }
    EventPair ev_a(c), ev_b(c), ev_c(c);
    if (!ev_a.a || !ev_a.b || !ev_b.a || !ev_b.b || !ev_c.a || !ev_c.b) return fail(QMCP_EHIP, "event creation failed");

    // 1. ranges and validation
    const size_t tab = (size_t)n_contigs + 1;
    std::vector<uint64_t> poff(tab, 0);
    for (uint32_t k = 0; k < n_contigs; ++k) poff[k + 1] = poff[k] + lengths[k];
    const uint64_t ltot = poff[n_contigs];
    TRY(ensure(c, c->dd_tab, tab * sizeof(uint64_t) + (size_t)n_contigs * sizeof(uint32_t)));
    TRY(ensure(c, c->dd_stat, 16 * sizeof(uint64_t)));
    uint64_t* d_poff = c->dd_tab.u64();
    uint32_t* d_len = (uint32_t*)(d_poff + tab);
    uint32_t* d_range = c->dd_stat.u32();                 // 9 words (of 16)
    uint64_t* d_counters = c->dd_stat.u64() + 8;          // families, duplicate units, largest family
    HIP_TRY(hipMemcpyAsync(d_poff, poff.data(), tab * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_len, lengths, (size_t)n_contigs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    uint32_t range[16] = {0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    HIP_TRY(hipMemcpyAsync(c->dd_stat.p, range, sizeof(range), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint64_t), st));
    HIP_TRY(hipEventRecord(ev_a.a, st));
    {
        KernelSpan sp(c, "k_dd_range");
        qmcp::launch_dd_range(st, d_starts, d_ends, d_ids, d_tags, d_q, n, d_len, n_contigs, pairs, d_range);
    }
    HIP_TRY(hipEventRecord(ev_a.b, st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(range, d_range, 9 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    if (range[6] & 1u) return fail(QMCP_EINVAL, "a contig id is neither < n_contigs (%u) nor QMCP_NO_CONTIG", n_contigs);
    if (range[6] & 2u) return fail(QMCP_EREAD, "a read has start > end or end >= its contig's length");
    const uint32_t tag_lo = range[0], tag_hi = range[1], q_lo = range[2], q_hi = range[3];
    const uint32_t span_lo = range[4], span_hi = range[5];
    const uint32_t n_placed = range[7];
    if (n_placed && q_hi - q_lo > 65535u) return fail(QMCP_ERANGE, "quality range %u..%u exceeds 65535", q_lo, q_hi);
    const uint32_t n_units = pairs ? n / 2 : n;
    const uint32_t n_act = pairs ? n_units - range[8] : n_placed;  // the units that can be in a family
    ds.units = n_act;
    ds.ms_dedup = elapsed(ev_a.a, ev_a.b);

    // buffers of the sorts and of the segmented stage
    const uint32_t n_tiles = qmcp::sort_tiles(n);
    TRY(ensure(c, c->dd_bare, (size_t)n * sizeof(uint32_t)));
    TRY(ensure(c, c->dd_keys[0], (size_t)n * 8));
    TRY(ensure(c, c->dd_keys[1], (size_t)n * 8));
    TRY(ensure(c, c->dd_vals[0], (size_t)n * sizeof(uint32_t)));
    TRY(ensure(c, c->dd_vals[1], (size_t)n * sizeof(uint32_t)));
    TRY(ensure(c, c->dd_hist, (size_t)256 * n_tiles * sizeof(uint32_t)));
    const uint32_t spine_n = std::max(std::max(256u * n_tiles, n + 1), (uint32_t)words + 1);
    TRY(ensure(c, c->dd_spine, scan_spine_bytes(spine_n, 1)));
    TRY(ensure(c, c->dd_flag, ((size_t)n + 2) * sizeof(uint32_t)));
    TRY(ensure(c, c->dd_head, ((size_t)n + 2) * sizeof(uint32_t)));
    TRY(ensure(c, c->dd_surv, words * 8 + 16));
    TRY(ensure(c, c->dd_words, (words + 2) * sizeof(uint32_t)));
    TRY(ensure(c, c->dd_histo, (size_t)std::max(hist_bins, 1u) * sizeof(uint64_t)));
    if (pairs) TRY(ensure(c, c->dd_cid, ((size_t)n + 2) * sizeof(uint32_t)));
    uint32_t* flag = c->dd_flag.u32();
    uint32_t* headpos = c->dd_head.u32();
    uint32_t* cid = pairs ? c->dd_cid.u32() : nullptr;
    uint64_t* surv = c->dd_surv.u64();
    uint32_t* spine = c->dd_spine.u32();

    HIP_TRY(hipEventRecord(ev_b.a, st));
    HIP_TRY(hipMemsetAsync(surv, 0, words * 8, st));
    if (d_dup) HIP_TRY(hipMemsetAsync(d_dup, 0, words * 8, st));
    if (hist_bins) HIP_TRY(hipMemsetAsync(c->dd_histo.p, 0, (size_t)hist_bins * sizeof(uint64_t), st));

    // 2. keys and sorts
    uint32_t rbits[4];
    qmcp::dedup_read_fields(ltot, span_lo, span_hi, tag_lo, tag_hi, q_lo, q_hi, !pairs, rbits);
    const qmcp::DedupSortPlan rplan = qmcp::plan_dedup_sort(rbits, 4);
    const uint32_t min_span = n_placed ? span_lo : 0u, tag_min = n_placed ? tag_lo : 0u, q_max = n_placed ? q_hi : 0u;
    DedupSorted sorted;
    const DedupSortBufs bufs{c->dd_bare, c->dd_keys, c->dd_vals, c->dd_hist, c->dd_spine};
    TRY(dedup_sort(c, bufs, n, rplan,
                   [&](uint32_t r, uint32_t key_bytes, const uint32_t* idx, void* keys) {
                       KernelSpan sp(c, "k_dd_read_keys");
                       qmcp::launch_dd_read_keys(st, key_bytes, d_starts, d_ends, d_ids, d_tags, pairs ? nullptr : d_q, idx,
                                                 d_poff, ltot, n, min_span, tag_min, q_max, rplan.rounds[r].pack, keys);
                   },
                   sorted));
    ds.key_bits = rplan.key_bits;
    ds.sort_passes = rplan.passes;
    uint32_t low_bits = rbits[0];
    if (pairs) {
        // stage 1: dense cell ids in input order; stage 2: the units by signature and score
        {
            KernelSpan sp(c, "k_dd_heads(cells)");
            qmcp::launch_dd_heads(st, sorted.form, sorted.keys, sorted.vals, 0, n_placed, d_starts, d_ends, d_ids, d_tags,
                                  nullptr, flag);
        }
        if (n_placed) {
            KernelSpan sp(c, "scan_heads(dedup, 3 kernels)");
            qmcp::launch_exclusive_scan(st, flag, n_placed, flag, spine, true);
        }
        {
            KernelSpan sp(c, "k_dd_cell_ids");
            qmcp::launch_dd_cell_ids(st, sorted.vals, sorted.stride, flag, n_placed, n, n_placed, cid);
        }
        uint32_t pbits[3];
        qmcp::dedup_pair_fields(n_placed, n_placed ? q_lo : 1u, n_placed ? q_hi : 0u, pbits);
        if (!d_q) pbits[0] = 0;
        const qmcp::DedupSortPlan pplan = qmcp::plan_dedup_sort(pbits, 3);
        const uint32_t score_max = n_placed ? 2u * (q_hi - q_lo) : 0u;
        TRY(dedup_sort(c, bufs, n_units, pplan,
                       [&](uint32_t r, uint32_t key_bytes, const uint32_t* idx, void* keys) {
                           KernelSpan sp(c, "k_dd_pair_keys");
                           qmcp::launch_dd_pair_keys(st, key_bytes, cid, d_q, idx, n_units, n_placed, q_lo, score_max,
                                                     pplan.rounds[r].pack, keys);
                       },
                       sorted));
        ds.key_bits = pplan.key_bits;
        ds.sort_passes += pplan.passes;
        low_bits = pbits[0];
    }
    HIP_TRY(hipGetLastError());

    // 3. families
    {
        KernelSpan sp(c, "k_dd_heads");
        qmcp::launch_dd_heads(st, sorted.form, sorted.keys, sorted.vals, low_bits, n_act, d_starts, d_ends, d_ids, d_tags,
                              cid, flag);
    }
    if (n_act) {
        KernelSpan sp(c, "scan_heads(dedup, 3 kernels)");
        qmcp::launch_exclusive_scan(st, flag, n_act, flag, spine, true);
    }
    {
        KernelSpan sp(c, "k_dd_segments");
        qmcp::launch_dd_segments(st, pairs, sorted.vals, sorted.stride, flag, n_act, surv, d_dup, headpos);
    }
    {
        KernelSpan sp(c, "k_dd_family_stats");
        qmcp::launch_dd_family_stats(st, headpos, flag + n_act, n_act, 1u, hist_bins, c->dd_histo.u64(), d_counters);
    }
    // 4. the survivors' count
    {
        KernelSpan sp(c, "count survivors(popcounts, scan)");
        queue_mask_ranks(st, surv, (uint32_t)words, c->dd_words, c->dd_spine);
    }
    HIP_TRY(hipEventRecord(ev_b.b, st));
    HIP_TRY(hipGetLastError());
    uint32_t n_surv = 0;
    uint64_t counters[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(&n_surv, c->dd_words.u32() + words, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost, st));
    if (hist_out && hist_bins)
        HIP_TRY(hipMemcpyAsync(hist_out, c->dd_histo.p, (size_t)hist_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    ds.families = counters[0];
    ds.duplicate_units = counters[1];
    ds.largest_family = counters[2];
    ds.reads_survived = n_surv;
    ds.ms_dedup += elapsed(ev_b.a, ev_b.b);

    // 5. the solve of the survivors, back to input order
    qmcp_hip_stats plain;
    std::memset(&plain, 0, sizeof(plain));
    if (n_surv) {
        const size_t cb = (size_t)n_surv * sizeof(uint32_t);
        TRY(ensure(c, c->dd_cs, cb));
        TRY(ensure(c, c->dd_ce, cb));
        TRY(ensure(c, c->dd_ci, cb));
        TRY(ensure(c, c->dd_map, cb));
        TRY(ensure(c, c->dd_maskc, ((size_t)n_surv + 63) / 64 * 8 + 16));
        HIP_TRY(hipEventRecord(ev_c.a, st));
        {
            KernelSpan sp(c, "k_dd_compact");
            qmcp::launch_dd_compact(st, d_starts, d_ends, d_ids, surv, c->dd_words.u32(), n, c->dd_cs.u32(),
                                    c->dd_ce.u32(), c->dd_ci.u32(), c->dd_map.u32());
        }
        HIP_TRY(hipEventRecord(ev_c.b, st));
        HIP_TRY(hipGetLastError());
        TRY(solve_by_contig_on_device(c, c->dd_cs.u32(), c->dd_ce.u32(), c->dd_ci.u32(), n_surv, lengths, n_contigs, M,
            c->dd_maskc.u64(), &plain));
        ds.ms_dedup += elapsed(ev_c.a, ev_c.b);
    }
    HIP_TRY(hipEventRecord(ev_c.a, st));
    HIP_TRY(hipMemsetAsync(d_mask, 0, words * sizeof(uint64_t), st));
    if (n_surv) {
        KernelSpan sp(c, "k_expand_mask_reads(dedup)");
        qmcp::launch_expand_mask_reads(st, c->dd_maskc.u64(), c->dd_map.u32(), n_surv, d_mask);
    }
    if ((flags & QMCP_DEDUP_COMPLETE_PAIRS) && n_surv) {
        KernelSpan sp(c, "k_complete_pairs(dedup)");
        qmcp::launch_complete_pairs(st, d_mask, (uint32_t)words, n64);
    }
    HIP_TRY(hipEventRecord(ev_c.b, st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    ds.ms_dedup += elapsed(ev_c.a, ev_c.b);
    if (stats) *stats = plain;
    if (dstats) *dstats = ds;
    return QMCP_OK;
}

// the checks both entries make before anything is copied or launched
int check_dedup_call(uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t flags,
                     const uint64_t* hist_out, uint32_t hist_bins) {
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    if (!contig_lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    if (flags & ~(QMCP_DEDUP_PAIRS | QMCP_DEDUP_COMPLETE_PAIRS)) return fail(QMCP_EINVAL, "unknown flag bits 0x%x", flags);
    if ((flags & QMCP_DEDUP_COMPLETE_PAIRS) && !(flags & QMCP_DEDUP_PAIRS))
        return fail(QMCP_EINVAL, "QMCP_DEDUP_COMPLETE_PAIRS needs QMCP_DEDUP_PAIRS");
    if (flags && (n_reads & 1ull)) return fail(QMCP_EINVAL, "pair mode needs an even n_reads (%llu)", (unsigned long long)n_reads);
    if (hist_bins && !hist_out) return fail(QMCP_EINVAL, "hist_out missing");
    if (hist_bins > qmcp::dedup_hist_max())
        return fail(QMCP_ERANGE, "hist_bins %u exceeds %u", hist_bins, qmcp::dedup_hist_max());
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_dedup_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                              const uint32_t* tags, const uint32_t* qualities, uint64_t n_reads,
                              const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage, uint32_t flags,
                              uint64_t* keep_mask_out, uint64_t* dup_mask_out, uint64_t* hist_out, uint32_t hist_bins,
                              qmcp_hip_stats* stats, qmcp_hip_dedup_stats* dstats) {
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(check_dedup_call(n_reads, contig_lengths, n_contigs, flags, hist_out, hist_bins));
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    if (qualities) TRY(ensure(c, c->in_aux1, nb));
    if (tags) TRY(ensure(c, c->dd_tags, nb));
    TRY(ensure(c, c->mask, words * sizeof(uint64_t)));
    if (dup_mask_out) TRY(ensure(c, c->dd_dupm, words * sizeof(uint64_t)));
    c->mask_reads = 0;
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
        if (qualities) HIP_TRY(hipMemcpyAsync(c->in_aux1.p, qualities, nb, hipMemcpyHostToDevice, c->stream));
        if (tags) HIP_TRY(hipMemcpyAsync(c->dd_tags.p, tags, nb, hipMemcpyHostToDevice, c->stream));
    }
    TRY(solve_dedup_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(),
        tags ? c->dd_tags.u32() : nullptr, qualities ? c->in_aux1.u32() : nullptr, n_reads, contig_lengths, n_contigs,
        max_coverage, flags, c->mask.u64(), dup_mask_out ? c->dd_dupm.u64() : nullptr, hist_out, hist_bins, stats,
        dstats));
    if (words) {
        HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        if (dup_mask_out)
            HIP_TRY(hipMemcpyAsync(dup_mask_out, c->dd_dupm.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_dedup_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                const uint32_t* d_contig_ids, const uint32_t* d_tags, const uint32_t* d_qualities,
                                uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                uint32_t flags, uint64_t* d_keep_mask_out, uint64_t* d_dup_mask_out, uint64_t* hist_out,
                                uint32_t hist_bins, void* hip_stream, qmcp_hip_stats* stats, qmcp_hip_dedup_stats* dstats) {
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(check_dedup_call(n_reads, contig_lengths, n_contigs, flags, hist_out, hist_bins));
    TRY(order_after(c, hip_stream));
    return solve_dedup_on_device(c, d_starts, d_ends, d_contig_ids, d_tags, d_qualities, n_reads, contig_lengths, n_contigs,
                                 max_coverage, flags, d_keep_mask_out, d_dup_mask_out, hist_out, hist_bins, stats, dstats);
}

}  // extern "C"
