// depth_track.inc.hip -- part of qmcp_api.hip (one translation unit; after depth_report.inc.hip, whose checks, batches,
// tables and buffers it shares).
// qmcp_hip_depth_track_host / _device: per-base depth before and after a keep mask as runs of equal depth.
//   1. the flags, then check_depth_call: everything the report refuses on the host, in its order
//   2. per position batch: the report's tables, zeroed event words, k_depth_events, chunk sums + spine -- unchanged --
//      then k_track_count + k_track_spine over the same chunks, the batch's three totals and the validation word read
//      back (the stream is drained here in every batch: the run buffer is sized from the count), and, when records are
//      wanted and still fit the caller's capacity, k_track_emit into dt_runs and a copy to host staging
//   3. the device-found errors, then the capacity (QMCP_ERANGE with *n_runs_out set, nothing else written), then the
//      caller's buffers
// Buffers: the report's dr_ev, dr_tab, dr_sums, dr_cnt; dt_cnt (3 x chunks words, then 3 totals), dt_runs (a batch's
// records).
namespace {

int depth_track_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                          const uint64_t* d_mask, uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, uint32_t M,
                          const DepthCall& dc, uint32_t flags, uint32_t depth_cap, qmcp_hip_track_run* runs,
                          uint64_t run_capacity, uint64_t* n_runs_out, qmcp_hip_track_stats* stats) {
    const uint32_t n = (uint32_t)n64;
    const uint32_t n_reg = dc.has_regions ? dc.tab.regions_merged : 0u;
    hipStream_t st = c->stream;
    uint64_t most = 0;
    for (const qmcp::ContigBatch& bt : dc.batches) most = std::max(most, bt.positions);
    const size_t tab_words = 5 * (size_t)n_contigs + 3 * (size_t)n_reg;
    const uint32_t max_chunks = qmcp::depth_chunks((uint32_t)most);
    TRY(ensure(c, c->dr_tab, tab_words * 4 + 16));
    TRY(ensure(c, c->dr_ev, ((size_t)most + 1) * 8));
    TRY(ensure(c, c->dr_sums, (size_t)max_chunks * 8 + 16));
    TRY(ensure(c, c->dr_cnt, 32));
    TRY(ensure(c, c->dt_cnt, ((size_t)3 * max_chunks + 2) / 2 * 8 + 24));
    uint32_t* d_len = c->dr_tab.u32();
    uint32_t* d_boff = d_len + n_contigs;
    uint32_t* d_ci = d_boff + n_contigs;            // 3 x n_contigs
    uint32_t* d_ri = d_ci + 3 * (size_t)n_contigs;  // 3 x n_reg
    uint64_t* d_cnt = c->dr_cnt.u64();
    uint32_t* d_err = (uint32_t*)(d_cnt + 2);
    uint32_t* d_tc = c->dt_cnt.u32();
    uint64_t* d_tot = c->dt_cnt.u64() + ((size_t)3 * max_chunks + 2) / 2;  // (8-byte aligned, behind the counts)
    EventPair ev(c);
    if (!ev.a || !ev.b) return fail(QMCP_EHIP, "event creation failed");
    HIP_TRY(hipMemcpyAsync(d_len, lengths, (size_t)n_contigs * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(ev.a, st));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 32, st));
    std::vector<uint32_t> boff(n_contigs, 0), ci, rlo, rhi, rrow;
    std::vector<qmcp_hip_track_run> staged;
    uint64_t total_runs = 0, emitted = 0, short_positions = 0;
    bool fits = runs != nullptr;
    uint32_t err = 0;
    for (const qmcp::ContigBatch& bt : dc.batches) {
        const uint32_t c0 = bt.first_contig, c1 = bt.first_contig + bt.n_contigs;
        const uint32_t P = (uint32_t)bt.positions;
        if (P == 0) continue;  // (only contigs of length 0: no position, no run)
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
        // the scope's intervals: the merged regions when the call has regions (none in this batch: nothing is in scope)
        const uint32_t* s_lo = dc.has_regions ? d_ri : d_ci;
        const uint32_t* s_hi = dc.has_regions ? d_ri + n_ri : d_ci + bt.n_contigs;
        const uint32_t n_s = dc.has_regions ? n_ri : n_ci;
        {
            KernelSpan sp(c, "k_track_count + k_track_spine");
            qmcp::launch_track_count(st, c->dr_ev.u64(), P, c->dr_sums.u64(), M, flags, depth_cap,
                                     s_lo, s_hi, n_s, d_tc, d_tot);
        }
        HIP_TRY(hipGetLastError());
        uint64_t tot[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(tot, d_tot, 24, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (err) break;
        if (fits && total_runs + tot[0] > run_capacity) fits = false;
        if (fits && tot[0]) {
            TRY(ensure(c, c->dt_runs, (size_t)tot[0] * sizeof(qmcp_hip_track_run)));
            {
                KernelSpan sp(c, "k_track_emit");
                qmcp::launch_track_emit(st, c->dr_ev.u64(), P, c->dr_sums.u64(), M, flags,
                                        depth_cap, s_lo, s_hi, n_s, d_ci, d_ci + bt.n_contigs,
                                        d_ci + 2 * (size_t)bt.n_contigs, n_ci, d_tc, c->dt_runs.as<qmcp_hip_track_run>());
            }
            HIP_TRY(hipGetLastError());
            staged.resize((size_t)(total_runs + tot[0]));
            HIP_TRY(hipMemcpyAsync(staged.data() + total_runs, c->dt_runs.p, (size_t)tot[0] * sizeof(qmcp_hip_track_run),
                                   hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        total_runs += tot[0];
        emitted += tot[1];
        short_positions += tot[2];
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
    HIP_TRY(hipMemcpyAsync(cnt, d_cnt, 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    collect_spans(c);
    err = (uint32_t)cnt[2];
    if (err & 1u) return fail(QMCP_EINVAL, "a contig id is neither < n_contigs (%u) nor QMCP_NO_CONTIG", n_contigs);
    if (err & 2u) return fail(QMCP_EREAD, "a read has start > end or end >= its contig's length");
    if (runs && !fits) {
        if (n_runs_out) *n_runs_out = total_runs;
        return fail(QMCP_ERANGE, "run_capacity %llu is too small: %llu runs", (unsigned long long)run_capacity,
                    (unsigned long long)total_runs);
    }
    // 3. the caller's buffers are written from here on only
    qmcp_hip_track_stats ts;
    std::memset(&ts, 0, sizeof(ts));
    ts.n_runs = total_runs;
    ts.positions_in_runs = emitted;
    ts.short_positions = short_positions;
    ts.reads_placed = cnt[0];
    ts.reads_kept = cnt[1];
    ts.regions_in = dc.has_regions ? dc.tab.regions_in : 0u;
    ts.regions_merged = n_reg;
    ts.position_batches = (uint32_t)dc.batches.size();
    ts.ms_track = elapsed(ev.a, ev.b);
    if (dc.has_regions) {
        ts.scope_positions = dc.tab.positions;
    } else {
        for (uint32_t k = 0; k < n_contigs; ++k) ts.scope_positions += lengths[k];
    }
    if (runs && total_runs) std::memcpy(runs, staged.data(), (size_t)total_runs * sizeof(qmcp_hip_track_run));
    if (n_runs_out) *n_runs_out = total_runs;
    if (stats) *stats = ts;
    return QMCP_OK;
}

int check_track_flags(uint32_t flags) {
    const uint32_t known = QMCP_TRACK_IN | QMCP_TRACK_KEPT | QMCP_TRACK_SHORT_ONLY | QMCP_TRACK_SKIP_ZERO;
    if (flags & ~known) return fail(QMCP_EINVAL, "unknown track flags 0x%x", flags & ~known);
    if (!(flags & (QMCP_TRACK_IN | QMCP_TRACK_KEPT)))
        return fail(QMCP_EINVAL, "track flags 0x%x select neither QMCP_TRACK_IN nor QMCP_TRACK_KEPT", flags);
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_depth_track_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                              uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, const uint64_t* keep_mask,
                              uint32_t max_coverage, const uint32_t* target_offsets, const uint32_t* target_starts,
                              const uint32_t* target_ends, uint32_t padding, uint32_t flags, uint32_t depth_cap,
                              qmcp_hip_track_run* runs, uint64_t run_capacity, uint64_t* n_runs_out,
                              qmcp_hip_track_stats* stats) {
    DepthCall dc;
    TRY(check_track_flags(flags));
    TRY(check_depth_call(n_reads, !starts || !ends || !contig_ids, contig_lengths, n_contigs, target_offsets, target_starts,
                         target_ends, padding, 0, nullptr, 0, dc));
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
    return depth_track_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(),
                                 keep_mask ? c->in_aux1.u64() : nullptr, n_reads, contig_lengths, n_contigs,
                                 max_coverage, dc, flags, depth_cap, runs, run_capacity, n_runs_out, stats);
}

int qmcp_hip_depth_track_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                const uint32_t* d_contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                uint32_t n_contigs, const uint64_t* d_keep_mask, uint32_t max_coverage,
                                const uint32_t* target_offsets, const uint32_t* target_starts, const uint32_t* target_ends,
                                uint32_t padding, uint32_t flags, uint32_t depth_cap, qmcp_hip_track_run* runs,
                                uint64_t run_capacity, uint64_t* n_runs_out, void* hip_stream, qmcp_hip_track_stats* stats) {
    DepthCall dc;
    TRY(check_track_flags(flags));
    TRY(check_depth_call(n_reads, !d_starts || !d_ends || !d_contig_ids, contig_lengths, n_contigs, target_offsets,
                         target_starts, target_ends, padding, 0, nullptr, 0, dc));
    TRY(use_device(c));
    TRY(order_after(c, hip_stream));
    return depth_track_on_device(c, d_starts, d_ends, d_contig_ids, d_keep_mask, n_reads, contig_lengths, n_contigs,
                                 max_coverage, dc, flags, depth_cap, runs, run_capacity, n_runs_out, stats);
}

}  // extern "C"
