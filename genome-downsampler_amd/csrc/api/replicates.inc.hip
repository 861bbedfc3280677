// replicates.inc.hip -- part of qmcp_api.hip (one translation unit).
// qmcp_hip_solve_replicates_host / _device: one read set split into disjoint downsamples.  Replicate 1 is the by-contig
// flow at coverages[0] (group_by_contig, run_batches with a PlainSolver: every fast route); replicate r + 1 is the ordinary
// multi-contig solve of the reads replicates 1 .. r left free.  The grouping runs once per call; what follows
// (replicates_later) walks replicate-major over its batches -- a mate may lie in another batch -- and per batch:
//   1. the candidates' taken bits: the last solve's mask (one batch, no pairs flag), or the input-order taken mask
//      gathered through the candidates' origins (k_rep_gather_taken)
//   2. k_word_popcounts -> exclusive scan of the taken bits; k_rep_offsets: the free rank at each contig's offset, the
//      next replicate's contig_read_offsets, n_contigs + 1 values, read back once (replicates_plan.h checks them)
//   3. k_rep_split: the free candidates' starts, ends and origins into the other set of columns; with the solve's mask
//      as the taken bits it also writes the taken candidates' labels
//   4. solve_on_device on the free reads at the replicate's coverage; its mask goes to bc_mask
//   5. otherwise k_rep_mark: the kept candidates' labels and their bits in the input-order taken mask
// and, under QMCP_REPLICATES_WHOLE_PAIRS, k_rep_complete_pairs once a replicate's labels are in for every batch.
// A call of one batch keeps its candidates from replicate to replicate (two sets of columns that ping-pong; they only
// shrink); a call of several batches gathers a batch's columns from the grouping's records again (k_bc_gather) and
// splits off what the taken mask leaves.  QMCP_REPLICATES_SHORTFALL: per replicate k_rep_label_mask and the depth
// report (depth_report_on_device) at the replicate's coverage; its deficit columns are the shortfall.
// Buffers, all the feature's own (rp_*), apart from the by-contig call's gathered columns and mask (bc_starts / bc_ends
// / bc_mask); nothing solve_on_device owns is held across a solve.
namespace {

struct ReplicatesRun {
    const uint32_t* coverages = nullptr;
    uint32_t n_replicates = 0, flags = 0;
    uint8_t* d_labels = nullptr;
    qmcp_hip_replicates_stats rs;
    qmcp_hip_stats rep[QMCP_REPLICATES_MAX];
};

// a batch's candidates: the reads no replicate has taken yet, in grouped order
struct RepCands {
    const uint32_t* s = nullptr;
    const uint32_t* e = nullptr;
    const void* o = nullptr;  // the grouping's {key, index} records (first), or a column of input indices
    bool first = true;
    uint32_t n = 0;
    std::vector<uint64_t> offs;  // contig_read_offsets of the candidates
};

// every replicate after the first, over all batches of the grouping; d_mask holds replicate 1
int replicates_later(qmcp_hip_ctx* c, ReplicatesRun& rp, const GroupedReads& g, uint64_t* d_mask, const qmcp_hip_stats& first) {
    hipStream_t st = c->stream;
    const std::vector<qmcp::ContigBatch>& batches = g.batches;
    const std::vector<size_t>& live = g.live;
    const uint64_t n64 = g.n64;
    qmcp_hip_replicates_stats& rs = rp.rs;
    const uint32_t K = rp.n_replicates;
    const bool pairs = (rp.flags & QMCP_REPLICATES_WHOLE_PAIRS) != 0;
    EventPair ev_a(c), ev_b(c);
    if (!ev_a.a || !ev_a.b || !ev_b.a || !ev_b.b) return fail(QMCP_EHIP, "event creation failed");
    rs.n_offered[0] = first.n_reads;
    rs.n_kept[0] = first.n_kept;
    rs.ms_replicate[0] = first.ms_total;
    rp.rep[0] = first;
    const uint64_t most = live.empty() ? 0 : batches[g.largest].n_reads;
    uint32_t tab_max = 1;
    for (size_t b : live) tab_max = std::max(tab_max, batches[b].n_contigs + 1);
    const bool single = live.size() == 1;
    const bool by_mask = single && !pairs;  // the candidates' taken bits are the last solve's mask
    const size_t words_in = (size_t)((n64 + 63) / 64);
    const size_t words_b = (size_t)((most + 63) / 64);
    TRY(ensure(c, c->rp_stat, QMCP_REPLICATES_MAX * sizeof(unsigned long long)));
    unsigned long long* d_mates = c->rp_stat.as<unsigned long long>();  // per replicate: the reads that joined as mates
    TRY(ensure(c, c->rp_words, (words_b + 2) * sizeof(uint32_t)));
    TRY(ensure(c, c->rp_spine, scan_spine_bytes((uint32_t)words_b + 1, 1)));
    TRY(ensure(c, c->rp_offs[0], (size_t)tab_max * sizeof(uint32_t)));
    TRY(ensure(c, c->rp_offs[1], (size_t)tab_max * sizeof(uint32_t)));
    if (!by_mask) {
        TRY(ensure(c, c->rp_kept, words_b * sizeof(uint64_t)));
        TRY(ensure(c, c->rp_taken, words_in * sizeof(uint64_t)));
    }
    uint64_t* d_taken = c->rp_taken.u64();
    // ev_a brackets what is queued between two host waits; ev_b a split, whose time is added at the next wait
    bool open = false, split_timed = false;
    auto begin = [&]() -> int {
        if (!open) HIP_TRY(hipEventRecord(ev_a.a, st));
        open = true;
        return QMCP_OK;
    };
    auto wait = [&]() -> int {
        TRY(begin());
        HIP_TRY(hipEventRecord(ev_a.b, st));
        HIP_TRY(hipStreamSynchronize(st));
        rs.ms_split += elapsed(ev_a.a, ev_a.b);
        if (split_timed) rs.ms_split += elapsed(ev_b.a, ev_b.b);
        open = split_timed = false;
        return QMCP_OK;
    };
    TRY(begin());
    HIP_TRY(hipMemsetAsync(c->rp_stat.p, 0, QMCP_REPLICATES_MAX * sizeof(unsigned long long), st));
    if (!by_mask && n64) {
        // replicate 1 is whole in d_mask: its labels, the taken mask, its mates
        HIP_TRY(hipMemcpyAsync(d_taken, d_mask, words_in * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        {
            KernelSpan sp(c, "k_rep_label_input");
            qmcp::launch_rep_label_input(st, d_mask, n64, 1, rp.d_labels);
        }
        if (pairs) {
            KernelSpan sp(c, "k_rep_complete_pairs");
            qmcp::launch_rep_complete_pairs(st, g.d_ids, n64, 1, rp.d_labels, d_taken, d_mates);
            HIP_TRY(hipMemcpyAsync(d_mask, d_taken, words_in * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        }
        HIP_TRY(hipGetLastError());
    }

    std::vector<uint32_t> ranks;
    std::vector<uint64_t> next;
    BatchView v;
    uint32_t cur = 0;  // which of rp_offs holds the candidates' offsets
    uint32_t set = 0;  // which set of columns the next split fills
    // steps 2 and 3 for one batch: cd becomes the candidates `taken` leaves free
    auto advance = [&](RepCands& cd, const uint64_t* taken, uint32_t n_contigs, uint32_t label) -> int {
        const size_t tab = (size_t)n_contigs + 1;
        const uint32_t words = (cd.n + 63u) / 64u;
        ranks.assign(tab, 0);
        TRY(begin());
        {
            KernelSpan sp(c, "replicate offsets(popcounts, scan, k_rep_offsets)");
            queue_mask_ranks(st, taken, words, c->rp_words, c->rp_spine);
            qmcp::launch_rep_offsets(st, c->rp_offs[cur].u32(), n_contigs, taken, c->rp_words.u32(),
                                     c->rp_offs[cur ^ 1u].u32());
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ranks.data(), c->rp_offs[cur ^ 1u].p, tab * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        TRY(wait());
        if (qmcp::replicates_next_offsets(cd.offs.data(), ranks.data(), n_contigs, next) != QMCP_OK)
            return fail(QMCP_EHIP, "replicates: the free ranks do not fit the contig offsets");
        const uint32_t n_next = ranks[n_contigs];
        const size_t cb = (size_t)n_next * sizeof(uint32_t);
        TRY(ensure(c, c->rp_starts[set], cb));
        TRY(ensure(c, c->rp_ends[set], cb));
        TRY(ensure(c, c->rp_orig[set], cb));
        if (n_next || label) {
            HIP_TRY(hipEventRecord(ev_b.a, st));
            {
                KernelSpan sp(c, "k_rep_split");
                qmcp::launch_rep_split(st, cd.first, cd.s, cd.e, cd.o, taken, c->rp_words.u32(), cd.n, label,
                                       rp.d_labels, c->rp_starts[set].u32(), c->rp_ends[set].u32(),
                                       c->rp_orig[set].u32());
            }
            HIP_TRY(hipEventRecord(ev_b.b, st));
            HIP_TRY(hipGetLastError());
            split_timed = true;
        }
        cd.s = c->rp_starts[set].u32();
        cd.e = c->rp_ends[set].u32();
        cd.o = c->rp_orig[set].p;
        cd.first = false;
        cd.n = n_next;
        cd.offs.swap(next);
        cur ^= 1u;
        set ^= 1u;
        return QMCP_OK;
    };
    // a batch's candidates before any split: its gathered columns (in bc_starts / bc_ends) and the grouping's records
    auto whole_batch = [&](size_t b, RepCands& cd) -> int {
        g.view(b, v);
        v.tables32();
        cd.s = c->bc_starts.u32();
        cd.e = c->bc_ends.u32();
        cd.o = v.records;
        cd.first = true;
        cd.n = v.nb;
        cd.offs = v.roff;
        TRY(begin());
        // (v stays untouched until the next wait: every use of it is followed by one)
        HIP_TRY(hipMemcpyAsync(c->rp_offs[0].p, v.offs32.data(), v.offs32.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                               st));
        cur = 0;
        return QMCP_OK;
    };
    // step 4, and what it adds to replicate j's numbers
    auto solve = [&](const RepCands& cd, const qmcp::ContigBatch& bt, uint32_t j, bool first_of_j, bool is_largest) -> int {
        qmcp_hip_stats bs;
        std::memset(&bs, 0, sizeof(bs));
        TRY(solve_on_device(c, cd.s, cd.e, cd.offs.data(), g.lengths + bt.first_contig, bt.n_contigs, cd.n, rp.coverages[j],
                            c->bc_mask.u64(), &bs));
        add_batch_stats(rp.rep[j], bs, first_of_j, is_largest);
        rp.rep[j].n_contigs += bt.n_contigs;
        rp.rep[j].total_length += bt.positions;
        rs.n_offered[j] += cd.n;
        rs.n_kept[j] += bs.n_kept;
        rs.ms_replicate[j] += bs.ms_total;
        return QMCP_OK;
    };

    if (by_mask) {
        const qmcp::ContigBatch& bt = batches[live[0]];
        RepCands cd;
        TRY(whole_batch(live[0], cd));
        uint32_t unlabelled = 1;  // the replicate whose mask is in bc_mask and whose labels are not written yet
        for (uint32_t j = 1; j < K; ++j) {
            TRY(advance(cd, c->bc_mask.u64(), bt.n_contigs, j));
            unlabelled = 0;
            if (cd.n == 0) break;  // no read left: this replicate and every later one are empty
            TRY(solve(cd, bt, j, true, true));
            unlabelled = j + 1;
        }
        if (unlabelled) {
            TRY(begin());
            KernelSpan sp(c, "k_ladder_levels(replicates)");
            qmcp::launch_ladder_levels(st, cd.first, c->bc_mask.u64(), cd.o, cd.n, unlabelled, rp.d_labels);
        }
        HIP_TRY(hipGetLastError());
    } else if (!live.empty()) {
        RepCands cd;
        if (single) TRY(whole_batch(live[0], cd));
        for (uint32_t j = 1; j < K; ++j) {
            bool first_of_j = true;
            for (size_t b : live) {
                const qmcp::ContigBatch& bt = batches[b];
                if (!single) {
                    TRY(whole_batch(b, cd));
                    TRY(gather_batch(c, v, g.d_starts, g.d_ends));
                    set = 0;
                }
                if (cd.n == 0) continue;
                {
                    KernelSpan sp(c, "k_rep_gather_taken");
                    qmcp::launch_rep_gather_taken(st, cd.first, cd.o, cd.n, d_taken, c->rp_kept.u64());
                }
                TRY(advance(cd, c->rp_kept.u64(), bt.n_contigs, 0));
                if (cd.n == 0) continue;
                TRY(solve(cd, bt, j, first_of_j, b == g.largest));
                first_of_j = false;
                TRY(begin());
                KernelSpan sp(c, "k_rep_mark");
                qmcp::launch_rep_mark(st, c->bc_mask.u64(), (const uint32_t*)cd.o, cd.n, j + 1, rp.d_labels, d_taken);
            }
            HIP_TRY(hipGetLastError());
            if (rs.n_offered[j] == 0) break;  // no read left anywhere
            if (pairs) {
                TRY(begin());
                KernelSpan sp(c, "k_rep_complete_pairs");
                qmcp::launch_rep_complete_pairs(st, g.d_ids, n64, j + 1, rp.d_labels, d_taken, d_mates + j);
            }
            HIP_TRY(hipGetLastError());
        }
    }
    unsigned long long mates[QMCP_REPLICATES_MAX];
    HIP_TRY(hipMemcpyAsync(mates, d_mates, sizeof(mates), hipMemcpyDeviceToHost, st));
    TRY(wait());
    for (uint32_t j = 0; j < K; ++j) {
        rs.n_mates[j] = mates[j];
        rs.n_kept[j] += mates[j];
    }

    if (rp.flags & QMCP_REPLICATES_SHORTFALL) {
        DepthCall dc;
        TRY(check_depth_call(n64, false, g.lengths, g.n_contigs, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, dc));
        TRY(ensure(c, c->rp_lmask, words_in * sizeof(uint64_t)));
        std::vector<qmcp_hip_depth_row> rows(g.n_contigs);
        for (uint32_t j = 0; j < K; ++j) {
            {
                KernelSpan sp(c, "k_rep_label_mask");
                qmcp::launch_rep_label_mask(st, rp.d_labels, n64, j + 1, c->rp_lmask.u64());
            }
            HIP_TRY(hipGetLastError());
            qmcp_hip_depth_stats ds;
            TRY(depth_report_on_device(c, g.d_starts, g.d_ends, g.d_ids, c->rp_lmask.u64(), n64, g.lengths, g.n_contigs,
                                       rp.coverages[j], dc, 0, rows.data(), nullptr, nullptr, nullptr, nullptr, &ds));
            for (const qmcp_hip_depth_row& row : rows) {
                rs.short_positions[j] += row.deficit_positions;
                rs.short_bases[j] += row.deficit_sum;
            }
            rs.ms_split += ds.ms_report;
        }
        rs.n_full = qmcp::replicates_n_full(rs.short_positions, K);
    }
    return QMCP_OK;
}

// what both entries check before anything is copied or launched
int check_replicates_entry(const uint32_t* coverages, uint32_t n_replicates, uint32_t flags, uint64_t n_reads) {
    uint32_t bad = 0;
    const int rc = qmcp::check_replicates_call(coverages, n_replicates, flags, n_reads, &bad);
    if (rc == QMCP_OK) return QMCP_OK;
    if (!coverages) return fail(QMCP_EINVAL, "coverages missing");
    if (n_replicates == 0 || n_replicates > QMCP_REPLICATES_MAX)
        return fail(QMCP_EINVAL, "n_replicates %u is not in 1 .. %u", n_replicates, (unsigned)QMCP_REPLICATES_MAX);
    if (flags & ~qmcp::kReplicateFlags) return fail(QMCP_EINVAL, "unknown flag bits 0x%x", flags & ~qmcp::kReplicateFlags);
    if (rc == QMCP_ERANGE) return fail(QMCP_ERANGE, "coverages[%u] = %u is 2^31 or more", bad, coverages[bad]);
    if (coverages[bad] == 0) return fail(QMCP_EINVAL, "coverages[%u] is 0: every replicate needs a coverage >= 1", bad);
    return fail(QMCP_EINVAL, "n_reads %llu is odd: reads (2q, 2q + 1) are pair q", (unsigned long long)n_reads);
}

int solve_replicates_on_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_ids,
                               uint64_t n64, const uint32_t* lengths, uint32_t n_contigs, const uint32_t* coverages,
                               uint32_t n_replicates, uint32_t flags, uint64_t* d_mask0, uint8_t* d_labels,
                               qmcp_hip_stats* stats, qmcp_hip_stats* rep_stats, qmcp_hip_replicates_stats* rstats) {
    // (heap: the run carries a qmcp_hip_stats per replicate)
    std::unique_ptr<ReplicatesRun> rp(new ReplicatesRun);
    rp->coverages = coverages;
    rp->n_replicates = n_replicates;
    rp->flags = flags;
    rp->d_labels = d_labels;
    std::memset(&rp->rs, 0, sizeof(rp->rs));
    std::memset(rp->rep, 0, sizeof(rp->rep));
    rp->rs.n_replicates = n_replicates;
    rp->rs.flags = flags;
    if (rstats) *rstats = rp->rs;
    if (rep_stats) std::memset(rep_stats, 0, (size_t)n_replicates * sizeof(qmcp_hip_stats));
    // (the bytes are cleared before the reads are validated, as group_by_contig clears the mask)
    if (n64 && n64 <= (1ull << 31)) HIP_TRY(hipMemsetAsync(d_labels, 0, (size_t)n64, c->stream));
    GroupedReads g;
    TRY(group_by_contig(c, d_starts, d_ends, d_ids, n64, lengths, n_contigs, d_mask0, g));
    PlainSolver first(coverages[0]);
    qmcp_hip_stats plain;
    TRY(run_batches(c, g, first, d_mask0, plain));
    TRY(replicates_later(c, *rp, g, d_mask0, plain));
    HIP_TRY(hipStreamSynchronize(c->stream));
    collect_spans(c);
    if (stats) *stats = plain;
    if (rep_stats) std::memcpy(rep_stats, rp->rep, (size_t)n_replicates * sizeof(qmcp_hip_stats));
    if (rstats) *rstats = rp->rs;
    return QMCP_OK;
}

}  // namespace

extern "C" {

int qmcp_hip_solve_replicates_host(qmcp_hip_ctx* c, const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                   uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                   const uint32_t* coverages, uint32_t n_replicates, uint32_t flags, uint8_t* labels_out,
                                   qmcp_hip_stats* stats, qmcp_hip_stats* rep_stats, qmcp_hip_replicates_stats* rstats) {
    TRY(check_replicates_entry(coverages, n_replicates, flags, n_reads));
    TRY(use_device(c));
    if (n_reads && (!starts || !ends || !contig_ids || !labels_out)) return fail(QMCP_EINVAL, "null buffer");
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    const size_t nb = (size_t)n_reads * sizeof(uint32_t);
    const size_t words = (size_t)((n_reads + 63) / 64);
    TRY(ensure(c, c->in_starts, nb));
    TRY(ensure(c, c->in_ends, nb));
    TRY(ensure(c, c->in_aux0, nb));
    TRY(ensure(c, c->mask, words * sizeof(uint64_t)));
    TRY(ensure(c, c->rp_labels, (size_t)n_reads));
    c->mask_reads = 0;
    if (nb) {
        HIP_TRY(hipMemcpyAsync(c->in_starts.p, starts, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_ends.p, ends, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->in_aux0.p, contig_ids, nb, hipMemcpyHostToDevice, c->stream));
    }
    TRY(solve_replicates_on_device(c, c->in_starts.u32(), c->in_ends.u32(),
                                   c->in_aux0.u32(), n_reads, contig_lengths, n_contigs, coverages, n_replicates,
                                   flags, c->mask.u64(), c->rp_labels.as<uint8_t>(), stats, rep_stats, rstats));
    if (n_reads) HIP_TRY(hipMemcpyAsync(labels_out, c->rp_labels.p, (size_t)n_reads, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask_reads = n_reads;
    return QMCP_OK;
}

int qmcp_hip_solve_replicates_device(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                                     const uint32_t* d_contig_ids, uint64_t n_reads, const uint32_t* contig_lengths,
                                     uint32_t n_contigs, const uint32_t* coverages, uint32_t n_replicates, uint32_t flags,
                                     uint8_t* d_labels_out, void* hip_stream, qmcp_hip_stats* stats,
                                     qmcp_hip_stats* rep_stats, qmcp_hip_replicates_stats* rstats) {
    TRY(check_replicates_entry(coverages, n_replicates, flags, n_reads));
    TRY(use_device(c));
    if (n_reads && (!d_starts || !d_ends || !d_contig_ids || !d_labels_out)) return fail(QMCP_EINVAL, "null buffer");
    if (n_reads > (1ull << 31))
        return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^31 per by-contig call", (unsigned long long)n_reads);
    TRY(ensure(c, c->rp_mask0, (size_t)((n_reads + 63) / 64) * sizeof(uint64_t)));
    TRY(order_after(c, hip_stream));
    return solve_replicates_on_device(c, d_starts, d_ends, d_contig_ids, n_reads, contig_lengths, n_contigs, coverages,
                                      n_replicates, flags, c->rp_mask0.u64(), d_labels_out, stats, rep_stats, rstats);
}

}  // extern "C"
