// ladder.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_ladder_host / _device: the by-contig solve at coverages[0], then level j + 1 solved on the reads level j
// kept, down the list; one byte per read says how many levels keep it.  group_by_contig runs once per call; the batch loop
// solves level 0, and the further levels run after each batch (LadderSolver::after_batch), on its gathered columns:
//   1. k_ladder_levels writes levels[origin] = j + 1 for the reads level j kept (the byte array was zeroed first)
//   2. k_word_popcounts -> exclusive scan of the level's mask; k_ladder_offsets evaluates the kept rank at each contig's
//      offset: the next level's contig_read_offsets, n_contigs + 1 values, read back once per level
//   3. k_ladder_compact writes the kept reads' starts, ends and origins (input indices) into the other set of buffers
//   4. solve_on_device on the compacted columns at the next coverage; its mask goes to bc_mask again
// Buffers, all the ladder's own: two sets of compacted columns (ld_starts / ld_ends / ld_orig) that ping-pong from
// level to level, the scanned popcounts (ld_words) and their spine (ld_spine), two offset tables (ld_offs), the host
// entry's level bytes (ld_levels) and the device entry's first-level mask (ld_mask0).  Nothing solve_on_device owns is
// touched: a solve sizes and frees its arena as it likes.  bc_mask is the by-contig solve's and holds a batch's mask from
// one solve to the next; every use of it here is queued on the stream between the two.
namespace {

// level 0 is the plain solve of the batch; the further levels follow once its mask is scattered
struct LadderSolver : PlainSolver {
    const uint32_t* coverages;
    uint32_t n_levels;
    uint8_t* d_levels;
    qmcp_hip_ladder_stats ls;
    LadderSolver(const uint32_t* cov, uint32_t levels, uint8_t* bytes)
        : PlainSolver(cov[0]), coverages(cov), n_levels(levels), d_levels(bytes) {}
    int after_batch(qmcp_hip_ctx* c, BatchView& v) override;
};

int LadderSolver::after_batch(qmcp_hip_ctx* c, BatchView& v) {
    hipStream_t st = c->stream;
    const uint32_t nb = v.nb, n_contigs = v.n_contigs;
    EventPair ev_a(c), ev_b(c);
    if (!ev_a.a || !ev_a.b || !ev_b.a || !ev_b.b) return fail(QMCP_EHIP, "event creation failed");
    const size_t tab = (size_t)n_contigs + 1;
    std::vector<uint32_t> ranks(tab);
    std::vector<uint64_t> cur(v.roff), next;
    if (n_levels > 1) {
        TRY(ensure(c, c->ld_offs[0], tab * sizeof(uint32_t)));
        TRY(ensure(c, c->ld_offs[1], tab * sizeof(uint32_t)));
        const size_t words0 = ((size_t)nb + 63) / 64;
        TRY(ensure(c, c->ld_words, (words0 + 2) * sizeof(uint32_t)));
        TRY(ensure(c, c->ld_spine, scan_spine_bytes((uint32_t)words0 + 1, 1)));
        v.tables32();
        HIP_TRY(hipMemcpyAsync(c->ld_offs[0].p, v.offs32.data(), tab * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    // the level whose mask is in bc_mask: its reads, their columns and their origins
    uint32_t n = nb;
    const uint32_t* d_s = c->bc_starts.u32();
    const uint32_t* d_e = c->bc_ends.u32();
    const void* d_o = v.records;
    const uint64_t* d_m = c->bc_mask.u64();
    bool compact_timed = false;
    for (uint32_t j = 0; j < n_levels; ++j) {
        const bool first = j == 0;
        const bool last = j + 1 == n_levels;
        HIP_TRY(hipEventRecord(ev_a.a, st));
        {
            KernelSpan sp(c, "k_ladder_levels");
            qmcp::launch_ladder_levels(st, first, d_m, d_o, n, j + 1, d_levels);
        }
        if (!last) {
            const uint32_t words = (n + 63u) / 64u;
            KernelSpan sp(c, "ladder offsets(popcounts, scan, k_ladder_offsets)");
            queue_mask_ranks(st, d_m, words, c->ld_words, c->ld_spine);
            qmcp::launch_ladder_offsets(st, c->ld_offs[j & 1u].u32(), n_contigs, d_m,
                                        c->ld_words.u32(), c->ld_offs[(j & 1u) ^ 1u].u32());
        }
        HIP_TRY(hipEventRecord(ev_a.b, st));
        HIP_TRY(hipGetLastError());
        if (!last)
            HIP_TRY(hipMemcpyAsync(ranks.data(), c->ld_offs[(j & 1u) ^ 1u].p, tab * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                   st));
        HIP_TRY(hipStreamSynchronize(st));
        ls.ms_ladder += elapsed(ev_a.a, ev_a.b);
        if (compact_timed) ls.ms_ladder += elapsed(ev_b.a, ev_b.b);
        compact_timed = false;
        if (last) break;
        if (qmcp::ladder_next_offsets(cur.data(), ranks.data(), n_contigs, next) != QMCP_OK)
            return fail(QMCP_EHIP, "ladder level %u: the kept ranks do not fit the contig offsets", j);
        const uint32_t n_next = ranks[n_contigs];
        if (n_next == 0) break;  // (n == 0 only: a level at >= 1 keeps a read of every contig that has one)
        const uint32_t set = j & 1u;
        const size_t cb = (size_t)n_next * sizeof(uint32_t);
        TRY(ensure(c, c->ld_starts[set], cb));
        TRY(ensure(c, c->ld_ends[set], cb));
        TRY(ensure(c, c->ld_orig[set], cb));
        HIP_TRY(hipEventRecord(ev_b.a, st));
        {
            KernelSpan sp(c, "k_ladder_compact");
            qmcp::launch_ladder_compact(st, first, d_s, d_e, d_o, d_m, c->ld_words.u32(), n, c->ld_starts[set].u32(),
                                        c->ld_ends[set].u32(), c->ld_orig[set].u32());
        }
        HIP_TRY(hipEventRecord(ev_b.b, st));
        HIP_TRY(hipGetLastError());
        compact_timed = true;
        n = n_next;
        d_s = c->ld_starts[set].u32();
        d_e = c->ld_ends[set].u32();
        d_o = c->ld_orig[set].p;
        cur.swap(next);
        qmcp_hip_stats bs;
        std::memset(&bs, 0, sizeof(bs));
        TRY(solve_on_device(c, d_s, d_e, cur.data(), v.lengths, n_contigs, n, coverages[j + 1], c->bc_mask.u64(), &bs));
        ls.n_kept[j + 1] += bs.n_kept;
        ls.ms_level[j + 1] += bs.ms_total;
    }
    return QMCP_OK;
}

// what both entries check before anything is copied or launched
int check_ladder_call(const uint32_t* coverages, uint32_t n_levels) {
    uint32_t bad = 0;
    if (qmcp::check_ladder_coverages(coverages, n_levels, &bad) == QMCP_OK) return QMCP_OK;
    if (!coverages) return fail(QMCP_EINVAL, "coverages missing");
    if (n_levels == 0 || n_levels > QMCP_LADDER_MAX_LEVELS)
        return fail(QMCP_EINVAL, "n_levels %u is not in 1 .. %u", n_levels, (unsigned)QMCP_LADDER_MAX_LEVELS);
    if (coverages[bad] == 0) return fail(QMCP_EINVAL, "coverages[%u] is 0: every level needs a coverage >= 1", bad);
    return fail(QMCP_EINVAL, "coverages must fall strictly: coverages[%u] = %u is not below coverages[%u] = %u", bad,
                coverages[bad], bad - 1, coverages[bad - 1]);
}

int solve_ladder_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                           uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, const uint32_t* coverages,
                           uint32_t n_levels, uint64_t* d_mask0, uint8_t* d_levels, qmcp_hip_stats* stats,
                           qmcp_hip_ladder_stats* lstats) {
    LadderSolver ld(coverages, n_levels, d_levels);
    std::memset(&ld.ls, 0, sizeof(ld.ls));
    ld.ls.n_levels = n_levels;
    if (lstats) *lstats = ld.ls;
    // (the bytes are cleared before the reads are validated, as group_by_contig clears the mask)
    if (n64 && n64 <= (1ull << 31)) HIP_TRY(hipMemsetAsync(d_levels, 0, (size_t)n64, c->stream));
    GroupedReads g;
    TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, d_mask0, g));
    qmcp_hip_stats plain;
    TRY(run_batches(c, g, ld, d_mask0, plain));
    HIP_TRY(hipStreamSynchronize(c->stream));
    collect_spans(c);
    ld.ls.n_kept[0] = plain.n_kept;
    ld.ls.ms_level[0] = plain.ms_total;
    if (stats) *stats = plain;
    if (lstats) *lstats = ld.ls;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_ladder_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                               uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                               const uint32_t* coverages, uint32_t n_levels, uint8_t* levels_out, qmcp_hip_stats* stats,
                               qmcp_hip_ladder_stats* lstats) {
    TRY(check_ladder_call(coverages, n_levels));
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !levels_out)) return fail(QMCP_EINVAL, "null buffer");
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    TRY(ensure(c, c->mask, words * sizeof(uint64_t)));
    TRY(ensure(c, c->ld_levels, (size_t)n_reads));
    c->mask_reads = 0;
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
    }
    TRY(solve_ladder_on_device(c, c->in_starts.u32(), c->in_ends.u32(), c->in_aux0.u32(), n_reads, contig_lengths,
        n_contigs, coverages, n_levels, c->mask.u64(), c->ld_levels.as<uint8_t>(), stats, lstats));
    if (n_reads) HIP_TRY(hipMemcpyAsync(levels_out, c->ld_levels.p, (size_t)n_reads, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_ladder_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                 const uint32_t* d_contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                 uint32_t n_contigs, const uint32_t* coverages, uint32_t n_levels, uint8_t* d_levels_out,
                                 void* hip_stream, qmcp_hip_stats* stats, qmcp_hip_ladder_stats* lstats) {
    TRY(check_ladder_call(coverages, n_levels));
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_levels_out)) return fail(QMCP_EINVAL, "null buffer");
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    TRY(ensure(c, c->ld_mask0, (size_t)((n_reads + 63) / 64) * sizeof(uint64_t)));
    TRY(order_after(c, hip_stream));
    return solve_ladder_on_device(c, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, n_contigs, coverages,
                                  n_levels, c->ld_mask0.u64(), d_levels_out, stats, lstats);
}

}  // extern "C"
