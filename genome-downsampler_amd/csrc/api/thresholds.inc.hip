// thresholds.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_thresholds_host / _device: every read's smallest coverage in coverage_lo .. coverage_hi whose by-contig
// solve keeps it (QMCP_THRESHOLD_NEVER where none does), and the reads kept at every coverage of the range.
//   1. group_by_contig (api/by_contig.inc.hip): once per call; a call of one batch with reads gathers its columns once
//   2. the thresholds filled with QMCP_THRESHOLD_NEVER, `seen` and the accumulators cleared
//   3. M = coverage_lo, coverage_lo + 1, ...: a whole solve at M into the cleared probe mask (ProbeSolve,
//      api/cap_search.inc.hip), k_thresholds_step, and the two accumulator words read back; the loop ends after the
//      first M at which every placed read has a threshold, or at coverage_hi
//   4. k_thresholds_finish (the mates' minimum under the flag, the histogram), k_thresholds_counts, one copy of the counts
// Buffers, all its own: th_mask (the probe mask; the grouping clears it, so a refused call leaves the caller's array
// alone), th_seen, th_acc (ThresholdsAccWord words | histogram), th_thr (the host entry's thresholds).
namespace {

// the checks both entries make before anything is copied or launched
int check_thresholds_call(uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t lo, uint32_t hi,
                          uint32_t flags, const uint64_t* counts_out, uint32_t counts_capacity) {
    switch (qmcp::thresholds_check(n_reads, lo, hi, flags, counts_out != nullptr, counts_capacity)) {
        case qmcp::kThresholdsOk: break;
        case qmcp::kThresholdsBadFlags:
            return fail(QMCP_EINVAL, "unknown flag bits 0x%x", flags & ~QMCP_THRESHOLDS_WHOLE_PAIRS);
        case qmcp::kThresholdsOddReads:
            return fail(QMCP_EINVAL, "n_reads %llu is odd: reads (2q, 2q + 1) are pair q", (unsigned long long)n_reads);
        case qmcp::kThresholdsZeroLo: return fail(QMCP_EINVAL, "coverage_lo == 0: the range starts at 1 or above");
        case qmcp::kThresholdsLoAboveHi: return fail(QMCP_EINVAL, "coverage_lo %u > coverage_hi %u", lo, hi);
        case qmcp::kThresholdsCapacityOnly:
            return fail(QMCP_EINVAL, "counts_capacity %u without counts_out", counts_capacity);
        case qmcp::kThresholdsHiTooLarge:
            return fail(QMCP_ERANGE, "coverage_hi %u exceeds %u", hi, (unsigned)QMCP_THRESHOLDS_COVERAGE_MAX);
    }
    if (!contig_lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig_lengths missing or n_contigs == 0");
    if (n_contigs > (1u << 24)) return fail(QMCP_ERANGE, "n_contigs %u exceeds 2^24 per by-contig call", n_contigs);
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    return QMCP_OK;
}

int solve_thresholds_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                               uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, uint32_t lo, uint32_t hi,
                               uint32_t flags, uint16_t* d_thr, uint64_t* counts_out, uint32_t counts_capacity,
                               qmcp_hip_stats* stats, qmcp_hip_thresholds_stats* tstats) {
    qmcp_hip_thresholds_stats ts;
    std::memset(&ts, 0, sizeof(ts));
    ts.coverage_lo = lo;
    ts.coverage_hi = hi;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (tstats) *tstats = ts;
    const size_t words = (size_t)((n64 + 63) / 64);
    const bool whole_pairs = (flags & QMCP_THRESHOLDS_WHOLE_PAIRS) != 0;
    hipStream_t st = c->stream;
    TRY(ensure(c, c->th_mask, words * sizeof(uint64_t)));
    TRY(ensure(c, c->th_seen, words * sizeof(uint64_t)));

    // 1: the grouping (the mask it clears is the call's own: a refused call leaves d_thr alone)
    GroupedReads g;
    TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, c->th_mask.u64(), g));
    const uint64_t placed = g.offs[n_contigs];
    ts.reads_placed = placed;
    ProbeSolve probe{g};
    if (g.live.size() == 1) TRY(probe.gather(c, g.live.front()));  // its columns stay in bc_starts / bc_ends for every solve

    // 2: nothing seen, every threshold NEVER (0xFFFF: both bytes 0xFF)
    if (words) HIP_TRY(hipMemsetAsync(c->th_seen.p, 0, words * sizeof(uint64_t), st));
    if (n64) HIP_TRY(hipMemsetAsync(d_thr, 0xFF, (size_t)n64 * sizeof(uint16_t), st));
    TRY(ensure(c, c->th_acc, ((size_t)qmcp::kThWords + (size_t)(hi - lo) + 1) * sizeof(unsigned long long)));
    unsigned long long* d_acc = c->th_acc.as<unsigned long long>();
    unsigned long long* d_hist = d_acc + qmcp::kThWords;
    HIP_TRY(hipMemsetAsync(d_acc, 0, (size_t)qmcp::kThWords * sizeof(unsigned long long), st));

    // 3: the solves
    TimedLaunches timed{c};
    unsigned long long back[qmcp::kThWords] = {0, 0};
    qmcp_hip_stats last;
    std::memset(&last, 0, sizeof(last));
    uint32_t M = lo;
    for (;; ++M) {
        uint64_t* pm = c->th_mask.u64();
        if (words && M != lo) HIP_TRY(hipMemsetAsync(pm, 0, words * sizeof(uint64_t), st));  // (k_bc_scatter_mask ORs)
        qmcp_hip_stats sum;
        TRY(probe.solve(c, M, pm, sum));
        TRY(timed.run([&] {
            KernelSpan sp(c, "k_thresholds_step");
            qmcp::launch_thresholds_step(st, pm, c->th_seen.u64(), n64, M, d_thr, d_acc);
        }));
        HIP_TRY(hipMemcpyAsync(back, d_acc, sizeof(back), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        ts.ms_thresholds += timed.total();
        ts.ms_solves += sum.ms_total;
        ts.solves += 1;
        last = sum;
        if (back[qmcp::kThSeen] >= placed || M == hi) break;
    }
    ts.top = M;
    ts.nesting_violations = back[qmcp::kThViolations];
    ts.saturated = back[qmcp::kThSeen] >= placed ? 1u : 0u;

    // 4: the mates' minimum, the histogram over lo .. top, its running sum
    const uint32_t n_bins = ts.top - lo + 1u;
    std::vector<unsigned long long> counts(n_bins, 0ull);
    HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)n_bins * sizeof(unsigned long long), st));
    TRY(timed.run([&] {
        {
            KernelSpan sp(c, "k_thresholds_finish");
            qmcp::launch_thresholds_finish(st, d_ids, n64, whole_pairs, lo, n_bins, d_thr, d_hist);
        }
        KernelSpan sp(c, "k_thresholds_counts");
        qmcp::launch_thresholds_counts(st, d_hist, n_bins);
    }));
    HIP_TRY(hipMemcpyAsync(counts.data(), d_hist, (size_t)n_bins * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ts.ms_thresholds += timed.total();
    collect_spans(c);
    ts.n_kept = counts[n_bins - 1];
    if (counts_out && counts_capacity) {  // (no threshold lies above top: the counts stay there)
        ts.count_entries = (uint32_t)std::min<uint64_t>((uint64_t)hi - lo + 1u, counts_capacity);
        for (uint32_t k = 0; k < ts.count_entries; ++k) counts_out[k] = counts[std::min(k, n_bins - 1u)];
    }
    if (stats) *stats = last;
    if (tstats) *tstats = ts;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_thresholds_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends,
                                   const uint32_t* contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                   uint32_t n_contigs, uint32_t coverage_lo, uint32_t coverage_hi, uint32_t flags,
                                   uint16_t* thresholds_out, uint64_t* counts_out, uint32_t counts_capacity,
                                   qmcp_hip_stats* stats, qmcp_hip_thresholds_stats* tstats) {
    // (the refusals need no device: they come before the context is looked at)
    if (n_reads && (!starts || !ends || !contig_ids || !thresholds_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(check_thresholds_call(n_reads, contig_lengths, n_contigs, coverage_lo, coverage_hi, flags, counts_out,
                              counts_capacity));
    TRY(use_device(c));
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    TRY(ensure(c, c->th_thr, (size_t)n_reads * sizeof(uint16_t)));
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
    }
    TRY(solve_thresholds_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), n_reads, contig_lengths,
        n_contigs, coverage_lo, coverage_hi, flags, c->th_thr.as<uint16_t>(), counts_out, counts_capacity, stats, tstats));
    if (n_reads)
        HIP_TRY(hipMemcpyAsync(thresholds_out, c->th_thr.p, (size_t)n_reads * sizeof(uint16_t), hipMemcpyDeviceToHost,
                               c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return QMCP_OK;
}

int qmcp_hip_solve_thresholds_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                     const uint32_t* d_contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                     uint32_t n_contigs, uint32_t coverage_lo, uint32_t coverage_hi, uint32_t flags,
                                     uint16_t* d_thresholds_out, uint64_t* counts_out, uint32_t counts_capacity,
                                     void* hip_stream, qmcp_hip_stats* stats, qmcp_hip_thresholds_stats* tstats) {
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_thresholds_out)) return fail(QMCP_EINVAL, "null buffer");
    TRY(check_thresholds_call(n_reads, contig_lengths, n_contigs, coverage_lo, coverage_hi, flags, counts_out,
                              counts_capacity));
    TRY(use_device(c));
    TRY(order_after(c, hip_stream));
    return solve_thresholds_on_device(c, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, n_contigs, coverage_lo,
                                      coverage_hi, flags, d_thresholds_out, counts_out, counts_capacity, stats, tstats);
}

}  // extern "C"
