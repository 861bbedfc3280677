// depth_report.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_depth_report_host / _device: depth of the reads (cov) and of the kept reads (kept) summarised per contig and per
// merged region, histograms of both over the positions in scope, and the positions that violate kept >= min(cov, M).
//   1. the checks, target_table.h's merged regions and the position batches (by_contig_plan.h with read counts of 0: whole
//      contigs, at most kBatchMaxPositions positions each) on the host, before anything is copied or launched
//   2. per batch: the event words zeroed, k_depth_events over ALL reads (it validates every read and skips those of other
//      batches' contigs), chunk sums + spine, k_depth_consume into the rows' accumulators and the histograms
//   3. the validation word, the read counts, the accumulators and the histograms come back; the rows are assembled on the
//      host (interval, positions; a row without positions is all zero) and only then are the caller's buffers written
// Buffers: dr_ev (a batch's positions + 1 event words), dr_tab (lengths | offsets | contig intervals | region intervals),
// dr_acc (5 x rows 64-bit sums, then 4 x rows extrema), dr_hist, dr_sums (chunk sums), dr_cnt (placed, kept, error word).
// The host entry's columns go to in_starts / in_ends / in_aux0 and its mask to in_aux1; the context's own keep mask
// (c->mask) is not touched.
namespace {

struct DepthCall {
    qmcp::TargetTable tab;
    bool has_regions = false;
    std::vector<qmcp::ContigBatch> batches;
};

// everything that can be refused without a device, in the order of the targets entries
int check_depth_call(uint64_t n_reads, bool null_column, const uint32_t* contig_lengths, uint32_t n_contigs,
                     const uint32_t* target_offsets, const uint32_t* target_starts, const uint32_t* target_ends,
                     uint32_t padding, uint32_t n_bins, const qmcp_hip_depth_row* region_rows, uint64_t region_capacity,
                     DepthCall& dc) {
    if (n_reads && null_column) return fail(QMCP_EINVAL, "null buffer");
    if (n_reads >= (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 - 1 per depth report", (unsigned long long)n_reads);
    if (!contig_lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    if (n_bins > 4096u) return fail(QMCP_EINVAL, "n_bins %u exceeds 4096", n_bins);
    dc.has_regions = target_offsets != nullptr;
    if (dc.has_regions) {
        if (qmcp::check_target_offsets(target_offsets, n_contigs) != QMCP_OK)
            return fail(QMCP_EINVAL, "target_offsets must start at 0 and never decrease (%u contigs)", n_contigs);
        if (target_offsets[n_contigs] && (!target_starts || !target_ends)) return fail(QMCP_EINVAL, "null target table");
        if (qmcp::build_target_table(target_offsets, target_starts, target_ends, padding, contig_lengths, n_contigs,
                                     dc.tab) != QMCP_OK)
            return fail(QMCP_EINVAL, "a target region has start > end");
        if (region_rows && region_capacity < dc.tab.regions_merged)
            return fail(QMCP_EINVAL, "region_capacity %llu is too small: %u merged regions", (unsigned long long)region_capacity,
                        dc.tab.regions_merged);
    }
    const std::vector<uint64_t> no_reads(n_contigs, 0);
    uint32_t bad = 0;
    if (qmcp::plan_contig_batches(no_reads.data(), contig_lengths, n_contigs, dc.batches, &bad) != QMCP_OK)
        return fail(QMCP_ERANGE, "contig %u alone exceeds one position batch: %u positions (at most 2^31 - 2)", bad,
                    contig_lengths[bad]);
    return QMCP_OK;
}

int depth_report_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                           const uint64_t* d_mask, uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, uint32_t M,
                           const DepthCall& dc, uint32_t n_bins, qmcp_hip_depth_row* contig_rows,
                           qmcp_hip_depth_row* region_rows, uint64_t* n_region_rows_out, uint64_t* hist_in,
                           uint64_t* hist_kept, qmcp_hip_depth_stats* stats) {
    const uint32_t n = (uint32_t)n64;
    const uint32_t n_reg = dc.has_regions ? dc.tab.regions_merged : 0u;
    const uint32_t n_rows = n_contigs + n_reg;
    if (!hist_in && !hist_kept) n_bins = 0;
    hipStream_t st = c->stream;
    uint64_t most = 0;
    for (const qmcp::ContigBatch& bt : dc.batches) most = std::max(most, bt.positions);
    // tables: lengths | offsets | contig intervals (lo, hi, row) | region intervals (lo, hi, row)
    const size_t tab_words = 5 * (size_t)n_contigs + 3 * (size_t)n_reg;
    TRY(ensure(c, c->dr_tab, tab_words * 4 + 16));
    TRY(ensure(c, c->dr_ev, ((size_t)most + 1) * 8));
    TRY(ensure(c, c->dr_acc, (size_t)n_rows * (5 * 8 + 4 * 4)));
    TRY(ensure(c, c->dr_hist, 2 * (size_t)n_bins * 8 + 16));
    TRY(ensure(c, c->dr_sums, (size_t)qmcp::depth_chunks((uint32_t)most) * 8 + 16));
    TRY(ensure(c, c->dr_cnt, 32));
    uint32_t* d_len = c->dr_tab.u32();
    uint32_t* d_boff = d_len + n_contigs;
    uint32_t* d_ci = d_boff + n_contigs;      // 3 x n_contigs
    uint32_t* d_ri = d_ci + 3 * (size_t)n_contigs;  // 3 x n_reg
    uint64_t* d_acc64 = c->dr_acc.u64();
    uint32_t* d_acc32 = (uint32_t*)(d_acc64 + 5 * (size_t)n_rows);
    uint64_t* d_cnt = c->dr_cnt.u64();
    uint32_t* d_err = (uint32_t*)(d_cnt + 2);
    EventPair ev(c);
    if (!ev.a || !ev.b) return fail(QMCP_EHIP, "event creation failed");
    HIP_TRY(hipMemcpyAsync(d_len, lengths, (size_t)n_contigs * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(ev.a, st));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 32, st));
    HIP_TRY(hipMemsetAsync(d_acc64, 0, 5 * (size_t)n_rows * 8, st));
    HIP_TRY(hipMemsetAsync(d_acc32, 0, 4 * (size_t)n_rows * 4, st));
    HIP_TRY(hipMemsetAsync(d_acc32, 0xFF, (size_t)n_rows * 4, st));                          // min_in
    HIP_TRY(hipMemsetAsync(d_acc32 + 2 * (size_t)n_rows, 0xFF, (size_t)n_rows * 4, st));     // min_kept
    if (n_bins) HIP_TRY(hipMemsetAsync(c->dr_hist.p, 0, 2 * (size_t)n_bins * 8, st));
    // a batch's host tables stay untouched until its copies have completed: the stream is drained between batches
    std::vector<uint32_t> boff(n_contigs, 0), ci, rlo, rhi, rrow;
    for (const qmcp::ContigBatch& bt : dc.batches) {
        const uint32_t c0 = bt.first_contig, c1 = bt.first_contig + bt.n_contigs;
        const uint32_t P = (uint32_t)bt.positions;
        if (P == 0) continue;  // (only contigs of length 0: their rows stay zero, and they can hold no valid read;
                               //  a read on them is found by whichever batch runs -- or by the check below)
        uint32_t n_ci = 0, n_ri = 0;
        ci.assign(3 * (size_t)bt.n_contigs, 0);
        rlo.clear();
        rhi.clear();
        rrow.clear();
        uint32_t off = 0;
        for (uint32_t k = c0; k < c1; ++k) {
            boff[k] = off;
            if (lengths[k]) {
                ci[n_ci] = off;
                ci[bt.n_contigs + n_ci] = off + lengths[k] - 1;
                ci[2 * (size_t)bt.n_contigs + n_ci] = k;
                n_ci++;
            }
            if (n_reg)
                for (uint32_t r = dc.tab.offs[k]; r < dc.tab.offs[k + 1]; ++r) {
                    rlo.push_back(off + dc.tab.rs[r]);
                    rhi.push_back(off + dc.tab.re[r]);
                    rrow.push_back(n_contigs + r);
                }
            off += lengths[k];
        }
        n_ri = (uint32_t)rlo.size();
        HIP_TRY(hipMemcpyAsync(d_boff, boff.data(), (size_t)n_contigs * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_ci, ci.data(), ci.size() * 4, hipMemcpyHostToDevice, st));
        if (n_ri) {
            HIP_TRY(hipMemcpyAsync(d_ri, rlo.data(), (size_t)n_ri * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_ri + n_ri, rhi.data(), (size_t)n_ri * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_ri + 2 * (size_t)n_ri, rrow.data(), (size_t)n_ri * 4, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemsetAsync(c->dr_ev.p, 0, ((size_t)P + 1) * 8, st));
        {
            KernelSpan sp(c, "k_depth_events");
            qmcp::launch_depth_events(st, d_starts, d_ends, d_ids, n, d_mask, d_len, d_boff, n_contigs, c0, c1,
                                      c->dr_ev.u64(), d_cnt, d_err);
        }
        {
            KernelSpan sp(c, "k_depth_chunk_sums + k_depth_spine");
            qmcp::launch_depth_sums(st, c->dr_ev.u64(), P, c->dr_sums.u64());
        }
        {
            KernelSpan sp(c, "k_depth_consume");
            qmcp::launch_depth_consume(st, c->dr_ev.u64(), P, c->dr_sums.u64(), M, d_ci,
                                       d_ci + bt.n_contigs, d_ci + 2 * (size_t)bt.n_contigs, n_ci, d_ri, d_ri + n_ri,
                                       d_ri + 2 * (size_t)n_ri, n_ri, dc.has_regions, n_rows, d_acc64, d_acc32, n_bins,
                                       c->dr_hist.u64());
        }
        HIP_TRY(hipGetLastError());
        if (dc.batches.size() > 1) HIP_TRY(hipStreamSynchronize(st));
    }
    // every contig has length 0: no batch ran, the reads are still validated (each placed one is then a bad read)
    if (most == 0 && n) {
        HIP_TRY(hipMemcpyAsync(d_boff, boff.data(), (size_t)n_contigs * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(c->dr_ev.p, 0, 8, st));
        KernelSpan sp(c, "k_depth_events");
        qmcp::launch_depth_events(st, d_starts, d_ends, d_ids, n, d_mask, d_len, d_boff, n_contigs, 0, 0,
                                  c->dr_ev.u64(), d_cnt, d_err);
    }
    HIP_TRY(hipEventRecord(ev.b, st));
    HIP_TRY(hipGetLastError());
    uint64_t cnt[4] = {0, 0, 0, 0};
    std::vector<uint64_t> acc64(5 * (size_t)n_rows), hist(2 * (size_t)n_bins);
    std::vector<uint32_t> acc32(4 * (size_t)n_rows);
    HIP_TRY(hipMemcpyAsync(cnt, d_cnt, 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(acc64.data(), d_acc64, acc64.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(acc32.data(), d_acc32, acc32.size() * 4, hipMemcpyDeviceToHost, st));
    if (n_bins) HIP_TRY(hipMemcpyAsync(hist.data(), c->dr_hist.p, hist.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    const uint32_t err = (uint32_t)cnt[2];
    if (err & 1u) return fail(QMCP_EINVAL, "a contig id is neither < n_contigs (%u) nor QMCP_NO_CONTIG", n_contigs);
    if (err & 2u) return fail(QMCP_EREAD, "a read has start > end or end >= its contig's length");
    // 3. rows and statistics; the caller's buffers are written from here on only
    auto make_row = [&](uint32_t row, uint32_t contig, uint32_t start, uint32_t end, uint64_t positions) {
        qmcp_hip_depth_row r;
        std::memset(&r, 0, sizeof(r));
        r.contig = contig;
        if (positions == 0) return r;
        r.start = start;
        r.end = end;
        r.positions = positions;
        r.sum_in = acc64[row];
        r.sum_kept = acc64[(size_t)n_rows + row];
        r.capped_positions = acc64[2 * (size_t)n_rows + row];
        r.deficit_positions = acc64[3 * (size_t)n_rows + row];
        r.deficit_sum = acc64[4 * (size_t)n_rows + row];
        r.min_in = acc32[row];
        r.max_in = acc32[(size_t)n_rows + row];
        r.min_kept = acc32[2 * (size_t)n_rows + row];
        r.max_kept = acc32[3 * (size_t)n_rows + row];
        return r;
    };
    qmcp_hip_depth_stats ds;
    std::memset(&ds, 0, sizeof(ds));
    ds.reads_placed = cnt[0];
    ds.reads_kept = cnt[1];
    ds.regions_in = dc.has_regions ? dc.tab.regions_in : 0u;
    ds.regions_merged = n_reg;
    ds.position_batches = (uint32_t)dc.batches.size();
    ds.ms_report = elapsed(ev.a, ev.b);
    for (uint32_t k = 0; k < n_contigs; ++k) {
        const qmcp_hip_depth_row r = make_row(k, k, 0, lengths[k] ? lengths[k] - 1 : 0, lengths[k]);
        if (!dc.has_regions) {
            ds.scope_positions += r.positions;
            ds.deficit_positions += r.deficit_positions;
        }
        if (contig_rows) contig_rows[k] = r;
    }
    if (dc.has_regions) {
        ds.scope_positions = dc.tab.positions;
        for (uint32_t k = 0; k < n_contigs; ++k)
            for (uint32_t g = dc.tab.offs[k]; g < dc.tab.offs[k + 1]; ++g) {
                const qmcp_hip_depth_row r =
                    make_row(n_contigs + g, k, dc.tab.rs[g], dc.tab.re[g], (uint64_t)dc.tab.re[g] - dc.tab.rs[g] + 1);
                ds.deficit_positions += r.deficit_positions;
                if (region_rows) region_rows[g] = r;
            }
    }
    if (n_region_rows_out) *n_region_rows_out = n_reg;
    if (n_bins) {
        if (hist_in) std::memcpy(hist_in, hist.data(), (size_t)n_bins * 8);
        if (hist_kept) std::memcpy(hist_kept, hist.data() + n_bins, (size_t)n_bins * 8);
    }
    if (stats) *stats = ds;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_depth_report_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                               uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                               const uint64_t* keep_mask, uint32_t max_coverage, const uint32_t* target_offsets,
                               const uint32_t* target_starts, const uint32_t* target_ends, uint32_t padding, uint32_t n_bins,
                               qmcp_hip_depth_row* contig_rows, qmcp_hip_depth_row* region_rows, uint64_t region_capacity,
                               uint64_t* n_region_rows_out, uint64_t* hist_in, uint64_t* hist_kept,
                               qmcp_hip_depth_stats* stats) {
    DepthCall dc;
    TRY(check_depth_call(n_reads, !starts || !ends || !contig_ids, contig_lengths, n_contigs, target_offsets, target_starts,
                         target_ends, padding, n_bins, region_rows, region_capacity, dc));
    TRY(use_device(c));
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    if (keep_mask) TRY(ensure(c, c->in_aux1, words * sizeof(uint64_t)));
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
        if (keep_mask)
            HIP_TRY(hipMemcpyAsync(c->in_aux1.p, keep_mask, words * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    }
    return depth_report_on_device(c, c->in_starts.u32(), c->in_ends.u32(),
                                  c->in_aux0.u32(), keep_mask ? c->in_aux1.u64() : nullptr, n_reads,
                                  contig_lengths, n_contigs, max_coverage, dc, n_bins, contig_rows, region_rows,
                                  n_region_rows_out, hist_in, hist_kept, stats);
}

int qmcp_hip_depth_report_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                 const uint32_t* d_contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                 uint32_t n_contigs, const uint64_t* d_keep_mask, uint32_t max_coverage,
                                 const uint32_t* target_offsets, const uint32_t* target_starts, const uint32_t* target_ends,
                                 uint32_t padding, uint32_t n_bins, qmcp_hip_depth_row* contig_rows,
                                 qmcp_hip_depth_row* region_rows, uint64_t region_capacity, uint64_t* n_region_rows_out,
                                 uint64_t* hist_in, uint64_t* hist_kept, void* hip_stream, qmcp_hip_depth_stats* stats) {
    DepthCall dc;
    TRY(check_depth_call(n_reads, !d_starts || !d_ends || !d_contig_ids, contig_lengths, n_contigs, target_offsets,
                         target_starts, target_ends, padding, n_bins, region_rows, region_capacity, dc));
    TRY(use_device(c));
    TRY(order_after(c, hip_stream));
    return depth_report_on_device(c, d_starts, d_ends, d_contig_ids, d_keep_mask, n_reads, contig_lengths, n_contigs,
                                  max_coverage, dc, n_bins, contig_rows, region_rows, n_region_rows_out, hist_in, hist_kept,
                                  stats);
}

}  // extern "C"
