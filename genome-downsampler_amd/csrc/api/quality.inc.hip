// quality.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_quality_host / _device / _by_contig_host: the plain (or by-contig) solve, unchanged, then the quality
// pass of kernels/quality_cells.inc.hip on its mask, on the same stream:
//   1. the quality range of the placed reads, read back BEFORE the solve: a range above 65535 fails at once and leaves
//      the caller's mask untouched; after the solve, equal qualities (or a mask with nothing to choose) end here
//   2. composite keys gstart | span - min_span | q_max - q (the span field only where the call has several spans)
//   3. the stable LSD radix of the sort-based route: records {u32 key, index} when the key fits 32 bits, split u64 keys
//      and indices otherwise -- the records enter in index order, so equal keys stay in index order
//   4. segment marks, one exclusive scan (K bits) and two reverse min-scans (segment ends and starts), the choice, which
//      flips the mask bits that change
// The pass is a function of (K, start, end, contig, quality) alone: no route of the solve is touched.
namespace {

// the quality range of the placed reads (d_ids == NULL: every read), before the solve; ms: its device time
struct QualityRange {
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    float ms = 0.f;
    bool any() const { return lo <= hi; }
};

int quality_range(qmcp_hip_ctx* c, const uint32_t* d_q, const uint32_t* d_ids, uint64_t n64, QualityRange& r) {
    hipStream_t st = c->stream;
    EventPair ev(c);
    if (!ev.a || !ev.b) return fail(QMCP_EHIP, "event creation failed");
    HIP_TRY(hipEventRecord(ev.a, st));
    TRY(ensure(c, c->qc_words, 4 * sizeof(uint64_t)));
    const uint32_t init[2] = {0xFFFFFFFFu, 0u};
    HIP_TRY(hipMemcpyAsync(c->qc_words.p, init, sizeof(init), hipMemcpyHostToDevice, st));
    {
        KernelSpan sp(c, "k_qc_range");
        qmcp::launch_qc_range(st, d_q, d_ids, (uint32_t)n64, c->qc_words.u32());
    }
    HIP_TRY(hipGetLastError());
    uint32_t range[2] = {0xFFFFFFFFu, 0u};
    HIP_TRY(hipMemcpyAsync(range, c->qc_words.p, sizeof(range), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev.b, st));
    HIP_TRY(hipStreamSynchronize(st));
    r.lo = range[0];
    r.hi = range[1];
    r.ms = elapsed(ev.a, ev.b);
    if (r.any() && r.hi - r.lo > 65535u)
        return fail(QMCP_ERANGE, "quality range %u..%u exceeds 65535", r.lo, r.hi);
    return QMCP_OK;
}

// the pass on the plain mask in d_mask; ms_quality = the range's device time + the pass's
int quality_pass(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_q,
                 const uint32_t* d_ids, uint64_t n64, const uint64_t* roff, const uint32_t* lengths, uint32_t n_contigs,
                 const QualityRange& qr, const qmcp_hip_stats& plain, uint64_t* d_mask, qmcp_hip_quality_stats* qstats) {
    qmcp_hip_quality_stats qs;
    std::memset(&qs, 0, sizeof(qs));
    const uint32_t n = (uint32_t)n64;
    hipStream_t st = c->stream;
    EventPair ev(c);
    if (!ev.a || !ev.b) return fail(QMCP_EHIP, "event creation failed");
    hipEvent_t e0 = ev.a, e1 = ev.b;
    HIP_TRY(hipEventRecord(e0, st));
    const uint32_t range[2] = {qr.lo, qr.hi};
    const bool any_placed = qr.any();
    qs.quality_min = any_placed ? range[0] : 0u;
    qs.quality_max = any_placed ? range[1] : 0u;
    // nothing to choose: one quality, or no cell holds both a kept and a dropped read
    const uint64_t placed = plain.n_reads;
    const bool trivial = !any_placed || range[0] == range[1] || plain.n_kept == 0 || plain.n_kept == placed;
    if (!trivial) {
        const uint32_t q_bits = bit_width(range[1] - range[0]);
        const uint32_t span_bits = bit_width(plain.max_span - plain.min_span);
        // contig tables: read offsets (plain calls) and position offsets
        const size_t tab = (size_t)n_contigs + 1;
        std::vector<uint64_t> h_tab(2 * tab, 0);
        for (uint32_t k = 0; k < n_contigs; ++k) h_tab[tab + k + 1] = h_tab[tab + k] + lengths[k];
        if (roff) std::memcpy(h_tab.data(), roff, tab * sizeof(uint64_t));
        const uint64_t ltot = h_tab[tab + n_contigs];
        uint32_t g_bits = 0;
        while (g_bits < 64 && (ltot >> g_bits) != 0) ++g_bits;  // gstart <= ltot (the unplaced reads' cell)
        const uint32_t key_bits = g_bits + span_bits + q_bits;
        if (key_bits > 64)
            return fail(QMCP_ERANGE, "quality key of %u bits (positions %u, spans %u, qualities %u) exceeds 64", key_bits,
                        g_bits, span_bits, q_bits);
        const bool wide = key_bits > 32;
        const uint32_t passes = (key_bits + 7) / 8;
        qs.key_bits = key_bits;
        qs.sort_passes = passes;

        const uint32_t n_tiles = qmcp::sort_tiles(n);
        TRY(ensure(c, c->qc_tab, 2 * tab * sizeof(uint64_t)));
        TRY(ensure(c, c->qc_keys[0], (size_t)n * 8));
        TRY(ensure(c, c->qc_keys[1], (size_t)n * 8));
        if (wide) {
            TRY(ensure(c, c->qc_vals[0], (size_t)n * sizeof(uint32_t)));
            TRY(ensure(c, c->qc_vals[1], (size_t)n * sizeof(uint32_t)));
        } else {
            TRY(ensure(c, c->qc_bare, (size_t)n * sizeof(uint32_t)));
        }
        TRY(ensure(c, c->qc_hist, (size_t)256 * n_tiles * sizeof(uint32_t)));
        const uint32_t spine_n = std::max(256u * n_tiles, n + 1);
        TRY(ensure(c, c->qc_spine, scan_spine_bytes(spine_n)));
        TRY(ensure(c, c->qc_kb, ((size_t)n + 1) * sizeof(uint32_t)));
        TRY(ensure(c, c->qc_end, (size_t)n * sizeof(uint32_t)));
        TRY(ensure(c, c->qc_head, (size_t)n * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(c->qc_tab.p, h_tab.data(), 2 * tab * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(c->qc_words.u64() + 2, 0, 2 * sizeof(uint64_t), st));
        const uint64_t* d_roff = c->qc_tab.u64();
        const uint64_t* d_poff = d_roff + tab;

        // 2: keys
        {
            KernelSpan sp(c, "k_qc_keys");
            qmcp::launch_qc_keys(st, wide, d_starts, d_ends, d_q, d_ids, d_roff, d_poff, n_contigs, ltot, n,
                                 plain.min_span, span_bits, range[1], q_bits, wide ? c->qc_keys[0].p : c->qc_bare.p);
        }
        HIP_TRY(hipGetLastError());
        // 3: stable LSD radix
        const void* sorted = nullptr;
        const uint32_t* svals = nullptr;
        if (!wide) {
            int kin = 0;
            TRY(radix_sort_records(c, st, c->qc_bare.u32(), n, passes, c->qc_hist.u32(),
                                   c->qc_spine.u32(), c->qc_keys,
                                   {"k_radix_hist_rec(quality)", "scan_radix_hist(quality, 3 kernels)",
                                    "k_radix_scatter_rec(quality)"},
                                   &kin));
            sorted = c->qc_keys[kin].p;
        } else {
            WideBufs wb;
            TRY(radix_sort_wide(c, st, n, passes, c->qc_hist.u32(), c->qc_spine.u32(), c->qc_keys, c->qc_vals,
                                {"k_radix_hist(quality, u64)", "scan_radix_hist(quality, 3 kernels)",
                                 "k_radix_scatter(quality, u64)"},
                                &wb));
            sorted = c->qc_keys[wb.k].p;
            svals = c->qc_vals[wb.v].u32();
        }
        // 4: segments and the choice
        uint32_t* kb = c->qc_kb.u32();
        uint32_t* seg_end = c->qc_end.u32();
        uint32_t* seg_head = c->qc_head.u32();
        {
            KernelSpan sp(c, "k_qc_marks");
            qmcp::launch_qc_marks(st, wide, sorted, svals, n, q_bits, d_mask, kb, seg_end, seg_head);
        }
        {
            KernelSpan sp(c, "scan_kept(quality, 3 kernels)");
            qmcp::launch_exclusive_scan(st, kb, n, kb, c->qc_spine.u32(), true);
        }
        {
            KernelSpan sp(c, "k_rmin_*(quality segment bounds, 2 x 3 kernels)");
            qmcp::launch_reverse_min_scan(st, seg_end, n, c->qc_spine.u32());
            qmcp::launch_reverse_min_scan(st, seg_head, n, c->qc_spine.u32());
        }
        {
            KernelSpan sp(c, "k_qc_choose");
            qmcp::launch_qc_choose(st, wide, sorted, svals, n, kb, seg_end, seg_head, d_mask,
                                   c->qc_words.as<unsigned long long>() + 2);
        }
        HIP_TRY(hipGetLastError());
        uint64_t counters[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(counters, c->qc_words.u64() + 2, sizeof(counters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(e1, st));
        HIP_TRY(hipStreamSynchronize(st));
        qs.cells_contested = counters[0];
        qs.reads_swapped = counters[1];
    } else {
        HIP_TRY(hipEventRecord(e1, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    qs.ms_quality = qr.ms + elapsed(e0, e1);
    collect_spans(c);
    if (qstats) *qstats = qs;
    return QMCP_OK;
}

int solve_quality_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_q,
                            uint64_t n64, const uint64_t* roff, const uint32_t* lengths, uint32_t n_contigs,
                            uint32_t M, uint64_t* d_mask, qmcp_hip_stats* stats, qmcp_hip_quality_stats* qstats) {
    if (n64 > (1ull << 30)) return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^30 per call", (unsigned long long)n64);
    QualityRange qr;
    TRY(quality_range(c, d_q, nullptr, n64, qr));
    qmcp_hip_stats plain;
    std::memset(&plain, 0, sizeof(plain));
    TRY(solve_on_device(c, d_starts, d_ends, roff, lengths, n_contigs, n64, M, d_mask, &plain));
    TRY(quality_pass(c, d_starts, d_ends, d_q, nullptr, n64, roff, lengths, n_contigs, qr, plain, d_mask, qstats));
    if (stats) *stats = plain;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_quality_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends,
                                const uint32_t* qualities, uint64_t n_reads, const uint64_t* contig_read_offsets,
                                const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                uint64_t* keep_mask_out, qmcp_hip_stats* stats, qmcp_hip_quality_stats* qstats) {
    if (!qualities) return fail(QMCP_EINVAL, "qualities missing");
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    if (n_reads > (1ull << 30)) return fail(QMCP_ERANGE, "n_reads exceeds 2^30 per call");
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux1, nb));
    TRY(ensure(c, c->mask, words * sizeof(uint64_t)));
    c->mask_reads = 0;
    uint32_t sent_columns = 2;
    if (nb) {
        TRY(upload_columns(c, starts, ends, n_reads, &sent_columns));
        HIP_TRY(hipMemcpyAsync(c->in_aux1.p, qualities, nb, hipMemcpyHostToDevice, c->stream));
    }
    TRY(solve_quality_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux1.u32(), n_reads, contig_read_offsets,
        contig_lengths, n_contigs, max_coverage, c->mask.u64(), stats, qstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    if (stats) stats->columns_sent = sent_columns;
    return QMCP_OK;
}

int qmcp_hip_solve_quality_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                  const uint32_t* d_qualities, uint64_t n_reads, const uint64_t* contig_read_offsets,
                                  const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                  uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                  qmcp_hip_quality_stats* qstats) {
    if (!d_qualities) return fail(QMCP_EINVAL, "qualities missing");
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(order_after(c, hip_stream));
    return solve_quality_on_device(c, d_starts, d_ends, d_qualities, n_reads, contig_read_offsets, contig_lengths,
                                   n_contigs, max_coverage, d_keep_mask_out, stats, qstats);
}

int qmcp_hip_solve_quality_by_contig_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends,
                                          const uint32_t* contig_ids, const uint32_t* qualities, uint64_t n_reads,
                                          const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                          uint64_t* keep_mask_out, qmcp_hip_stats* stats,
                                          qmcp_hip_quality_stats* qstats) {
    if (!qualities) return fail(QMCP_EINVAL, "qualities missing");
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !keep_mask_out)) return fail(QMCP_EINVAL, "null buffer");
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    TRY(ensure(c, c->in_aux1, nb));
    TRY(ensure(c, c->mask, words * sizeof(uint64_t)));
    c->mask_reads = 0;
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux1.p, qualities, nb, hipMemcpyHostToDevice, c->stream));
    }
    QualityRange qr;
    TRY(quality_range(c, c->in_aux1.u32(), c->in_aux0.u32(), n_reads, qr));
    qmcp_hip_stats plain;
    std::memset(&plain, 0, sizeof(plain));
    TRY(solve_by_contig_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), n_reads, contig_lengths,
        n_contigs, max_coverage, c->mask.u64(), &plain));
    TRY(quality_pass(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux1.u32(), c->in_aux0.u32(), n_reads, nullptr,
        contig_lengths, n_contigs, qr, plain, c->mask.u64(), qstats));
    if (words) HIP_TRY(hipMemcpyAsync(keep_mask_out, c->mask.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    if (stats) *stats = plain;
    return QMCP_OK;
}

}  // extern "C"
