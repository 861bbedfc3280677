// context.inc.hip -- part of qmcp_api.hip (one translation unit).
// The solver context and the owning types of its device arena, pinned blocks, events and streams; per-kernel timing
// spans, problem checks, contig tables, small stage helpers.
namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return fail(_e == hipErrorOutOfMemory ? QMCP_ENOMEM : QMCP_EHIP, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(_e), __FILE__, __LINE__);                 \
    } while (0)

// Ownership: every device buffer, pinned block, event and stream of a context is a member of one of the four types
// below and frees itself when the context is deleted.  A feature declares its members in qmcp_hip_ctx and sizes them
// with ensure / ensure_pinned; there is no list to add them to.

// A device buffer of the arena.  Only ensure() allocates, grows or frees one; everything else reads p (an identity
// check, a void* parameter) or takes a typed pointer.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <class T> T* as() const { return static_cast<T*>(p); }
    uint32_t* u32() const { return as<uint32_t>(); }
    uint64_t* u64() const { return as<uint64_t>(); }
};

// A pinned host block (staging, landing zones); only ensure_pinned() allocates or grows one.
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t cap = 0;  // bytes
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    operator T*() const { return p; }
};

// An event or a stream: move-only, destroyed with its owner.  Created in place (hipEventCreate(&e.h)).
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    explicit Handle(H raw) : h(raw) {}
    Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
    Handle& operator=(Handle&&) = delete;
    ~Handle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
    H release() { H raw = h; h = nullptr; return raw; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

enum Ev { EV_BEGIN = 0, EV_PREP, EV_SCAN, EV_SORT, EV_SWEEP, EV_MARK, EV_COUNT };

struct Problem {
    uint64_t n = 0;
    uint32_t n_contigs = 0;
    uint64_t ltot = 0;
    std::vector<uint64_t> poff;
};

// A call's shape: what a context's memories of earlier calls are keyed by.  A memory that does not depend on a field
// leaves it 0 on both sides; n == 0 is no call's shape (such a call is trivial), so Shape() matches nothing.
struct Shape {
    uint64_t n = 0, ltot = 0;
    uint32_t M = 0, ell = 0;  // ell: the dominant span (near-uniform route)
    bool operator==(const Shape& o) const { return n == o.n && ltot == o.ltot && M == o.M && ell == o.ell; }
};
// "A call of this shape did X last time": what a context remembers about earlier calls.
struct Memories {
    // {n, ltot}: positions that start no read, as counted by the last range-ranked solve (picks the sweep kernel of the next)
    Shape spiky;
    bool spiky_known = false;
    uint32_t spiky_empty = 0;
    // {n, ltot, M}: the mixed-span route's speculative boundaries disagreed nearly everywhere (data that forgets its state
    // slowly: one dominant read length, deep): the next call of the shape does not speculate
    Shape spec_hopeless;
    // {n, ltot, M, ell}: the near-uniform route did not settle within its budget of rounds (or met a run the replay does
    // not model): the next call goes straight to the mixed-span route instead of burning the budget again
    Shape nu_failed;
    // {n, ltot, M, ell}: ... and it settled within this many queued rounds: the next call queues them -- and the ranking
    // behind them -- without waiting for the device in between (qmcp_hip_solve_device_begin returns at once; the state
    // words are looked at when the solve is collected, and a call that turns out to need more is solved again the
    // blocking way)
    Shape nu_need;
    uint32_t nu_need_rounds = 0;
    // qmcp_hip_set_options: what was learnt under other options.  nu_need (and the context's nu_ell) stay, as they always
    // have -- ADVICE.md round 4, finding 2; dropping them too changes what the next call queues.
    void forget() { spiky_known = false; spec_hopeless = nu_failed = Shape(); }
};

// what the two halves of a solve's enqueue share (see enqueue_head)
struct SolveRun {
    const uint32_t* d_starts = nullptr;
    const uint32_t* d_ends = nullptr;
    const uint64_t* roff = nullptr;     // host; valid until enqueue_tail has returned
    const uint32_t* lengths = nullptr;  // host; likewise
    uint32_t n_contigs = 0, M = 0;
    uint64_t n64 = 0;
    uint64_t* d_mask = nullptr;
    Problem pr;
    qmcp_hip_stats local;
    bool trivial = false, head_done = false, may_rank = false, two_level = false, have_gstart = true;
    bool ranked_counted = false, wait_empty = false;
    bool pm = false;                    // range-ranked route in its pass-major form (kernels/pass_major.inc.hip)
    uint32_t range_shift = 0;
    uint32_t pm_ranges = 0;             // ... the ranges of the grid it cuts (pm_grid_plan.h), and whether that is the aligned one
    bool pm_aligned = false;
    uint32_t nu_filter = 0;             // near-uniform route: the span the head's producer treated as regular (0: every read)
};

}  // namespace

struct qmcp_hip_ctx {
    int device = 0;
    qmcp_hip_options opt = {};      // which kernels and routes a solve takes where the data would decide (qmcp_hip_set_options)
    // (members are destroyed last to first: the main stream outlives everything queued on it)
    Stream stream;
    Event ev[EV_COUNT];
    Event ev_in;
    Stream stream2;  // side stream: small read-backs beside the work queued on `stream`
    Event ev_fork;  // main stream -> side stream: statistics and heaviest load are final
    // arena (grow-only, reused across solves like a reference solver instance's members)
    DevBuf roff, poff, stats, cstart, boff, ecnt, eoff, selend, spine, hist, spine2, hist2, specsnap, specflags;
    DevBuf keys[2], vals[2];
    DevBuf in_starts, in_ends, in_aux0, in_aux1, mask, cov, amp, next_head;
    DevBuf f_starts, f_ends, f_map, f_words, f_mask;  // filter -> solve pipeline
    DevBuf ranges;     // range-ranked path: range starts, heaviest load, level-2 tables (solve_words.h: Ranges)
    DevBuf rankamb;    // range-ranked path: per-range lists of quota-crossing groups, settled in the walk's tail
    // pass-major form (kernels/pass_major.inc.hip): one descriptor word per wave-slot; the table stage's working words
    DevBuf pm_desc, pm_work;
    // ... and the grid's tables (pm_grid_plan.h): on the device, in pinned staging, and as last uploaded
    DevBuf pm_grid;
    PinnedBuf<uint32_t> h_pm_grid;
    std::vector<uint32_t> pm_grid_sent;
    void* pm_grid_dev = nullptr;
    // near-uniform route (kernels/near_uniform.inc.hip): the dominant span of the last call that took it -- the next
    // call's head filters on it at once -- and the route's buffers
    uint32_t nu_ell = 0;
    Memories mem;                   // what earlier calls taught the context, by shape
    bool nu_deferred = false;       // the pending solve's rounds were queued unseen
    DevBuf nu_exc, nu_nadj, nu_ce, nu_state, nu_sus, nu_ckpt, nu_prev;
    PinnedBuf<uint32_t> h_nu;  // pinned landing zone of the route's state words (solve_words.h: NearUniform)
    PinnedBuf<uint64_t> h_tables;  // pinned staging for the contig tables (2 x (n_contigs + 1))
    PinnedBuf<unsigned long long> h_scalars;  // pinned landing zone of the solve's result scalars (solve_words.h: HostScalars)
    // qmcp_hip_solve_host64: pinned staging, two slots per narrowing thread, and a pinned mask landing zone
    PinnedBuf<uint32_t> h_stage;
    PinnedBuf<uint64_t> h_mask;
    std::vector<Event> stage_ev;
    std::vector<Stream> stage_streams;  // copy streams: one DMA engine moves ~29 GB/s, PCIe twice that
    std::vector<Event> stage_done;
    // a solve that has been enqueued but not yet completed (qmcp_hip_solve_device_begin / _end)
    bool pending = false;
    qmcp_hip_stats pend_stats;
    uint32_t pend_whole_contig_chains = 0;  // mixed spans without cut points: one chain per non-empty contig
    bool pend_spiky = false;                // ... and its head counted the positions that start no read (mem.spiky)
    uint32_t pend_M = 0;
    DevBuf scalars;  // popcount + sweep iteration counters + speculation words (solve_words.h)
    DevBuf segs;     // cut-point windows and the sweep's stretch table
    DevBuf rings;    // mixed spans beyond 16 383: the plain event sweep's rings, in global memory
    DevBuf kidx;          // qmcp_hip_kept_indices_host: the expanded index list
    // by-contig solves (api/by_contig.inc.hip): sort keys, the two record buffers of the grouping, its histogram and scan
    // spine, the contigs' bounds, the validation word, the contig lengths, a batch's gathered columns and its mask
    DevBuf bc_key, bc_rec[2], bc_hist, bc_spine, bc_offs, bc_err, bc_len, bc_starts, bc_ends, bc_mask;
    // FILTER -> by-contig solve (api/amplicon_by_contig.inc.hip): the input ids, the compacted ids, the contig lengths,
    // the amplicon table (offsets, sorted starts, running maxima of the ends) and the validation word
    DevBuf af_ids, af_ids_c, af_len, af_tab, af_err;
    // quality pass (api/quality.inc.hip): the quality range and counters, the contig tables, bare keys, the sort's two
    // key buffers (records, or u64 keys) and two index buffers (u64 keys only), its histogram and spine, the scanned K
    // bits and the segment bounds
    DevBuf qc_words, qc_tab, qc_bare, qc_keys[2], qc_vals[2], qc_hist, qc_spine, qc_kb, qc_end, qc_head;
    // target solves (api/targets.inc.hip): every read's projection, the mask of the placed off-target reads and the scan
    // of its popcounts, the compacted qualities, and the table (lengths, region offsets, remap, bounds, cum); the
    // compaction itself lives in the FILTER pipeline's buffers (f_*, af_ids_c, af_err, cov)
    DevBuf tg_ps, tg_pe, tg_off, tg_offw, tg_q, tg_tab;
    // depth report (api/depth_report.inc.hip): a batch's event words, its tables (lengths, offsets, the two interval
    // tables), the rows' accumulators, the histograms, the chunk sums, and the read counts + validation word
    DevBuf dr_ev, dr_tab, dr_acc, dr_hist, dr_sums, dr_cnt;
    // depth track (api/depth_track.inc.hip; the events, tables, chunk sums and counters are the report's): the chunks'
    // counts with the batch's three totals behind them, and a batch's records
    DevBuf dt_cnt, dt_runs;
    // coverage ladder (api/ladder.inc.hip): the two sets of compacted columns (starts, ends, input indices) that
    // ping-pong between levels, the scanned word popcounts of a level's mask and their spine, the two offset tables, the
    // host entry's level bytes and the device entry's first-level mask
    DevBuf ld_starts[2], ld_ends[2], ld_orig[2], ld_words, ld_spine, ld_offs[2], ld_levels, ld_mask0;
    // stratified solves (api/stratified.inc.hip): the host entry's strata column and the per-stratum rows (the grouping
    // and the batches use the by-contig buffers)
    DevBuf st_strata, st_rows;
    // duplicate-aware solves (api/dedup.inc.hip), all its own: the position offsets and contig lengths, the range words
    // and counters, bare keys, the sorts' two key buffers (records, or u64 keys) and two index columns, their histogram
    // and spine, the scanned head flags, the families' first positions, the reads' cell ids (pair mode), the survivor
    // mask and its scanned word popcounts, the size histogram, the survivors' columns, input indices and keep mask, and
    // the host entry's tag column and duplicate mask
    DevBuf dd_tab, dd_stat, dd_bare, dd_keys[2], dd_vals[2], dd_hist, dd_spine, dd_flag, dd_head, dd_cid, dd_surv, dd_words,
        dd_histo, dd_cs, dd_ce, dd_ci, dd_map, dd_maskc, dd_tags, dd_dupm;
    // start cap (api/start_cap.inc.hip), all its own, as the dd_* above: tables, range words and counters, the sort's
    // buffers, the scanned head flags, the cells' first positions, the kept members per cell, the survivor mask and its
    // scanned word popcounts, the size histogram, the survivors' columns, input indices and keep mask, and the host
    // entry's group column and capped mask
    DevBuf sc_tab, sc_stat, sc_bare, sc_keys[2], sc_vals[2], sc_hist, sc_spine, sc_flag, sc_head, sc_cnt, sc_surv, sc_words,
        sc_histo, sc_cs, sc_ce, sc_ci, sc_map, sc_maskc, sc_groups, sc_capm;
    // amplicon assignment and clipping (api/amplicon_clip.inc.hip), all its own: the tables (offsets, the sorted table,
    // contig lengths), the units' labels, the unit mask with its scanned word popcounts and their spine, the solve
    // columns and the rebased columns (3 + 3), the compacted columns, the survivors' input units, the compact keep mask,
    // the amplicons in use, the blocks' counters with their totals behind them, and the validation word
    DevBuf ac_tab, ac_label, ac_keep, ac_words, ac_spine, ac_col[6], ac_comp[3], ac_map, ac_maskc, ac_used, ac_part, ac_err;
    // coverage profile (api/profile.inc.hip): a batch's need[] (min(cov, cap) per position, top bit = cut position), its
    // regions in global positions (starts | ends | caps), and the call's two counters (capped positions, demand)
    DevBuf pf_need, pf_tab, pf_stat;
    // pair-aware solves (api/pairs.inc.hip), all its own: the kept set's bits in a batch's grouped order and their
    // complement (the candidates), the complement's scanned word popcounts and their spine, the batch's read offsets and
    // the candidates' ranks at them, its position offsets, the credit events and their scan with its spine, the
    // candidates' columns, input indices and keep mask, need[], and the counters (capped positions, demand, |S|)
    DevBuf pr_in, pr_rest, pr_words, pr_spine, pr_offs[2], pr_poff, pr_credit, pr_cspine, pr_starts, pr_ends, pr_orig,
        pr_mask, pr_need, pr_stat;
    // tiered solves (api/tiers.inc.hip), all its own: the host entry's tier column, the per-tier rows, the counters
    // (capped positions, demand, asked positions, reads without a tier), the kept list, the scanned word popcounts of a
    // batch's mask and their spine, a batch's position offsets, the credit events and their scan with its spine, need[]
    DevBuf tr_tiers, tr_rows, tr_stat, tr_list, tr_words, tr_spine, tr_poff, tr_credit, tr_cspine, tr_need;
    // template-aware solves (api/templates.inc.hip): the host entry's id column, the bitset of template ids a completion
    // goes through, the segments per template, and the counters (size histogram, templates in use, largest, kept, error)
    DevBuf tp_ids, tp_flags, tp_sizes, tp_stat;
    // template-aware solves under a cap table (api/templates_profile.inc.hip): a later stage's scaled regions of a batch
    // (starts | ends | caps), the call's table for the on-cap pass (offsets | starts | ends | caps | positive positions
    // before), the bitset of templates that touch a positive cap, and the two on-cap counters (segments, templates)
    DevBuf tq_tab, tq_cap, tq_flags, tq_stat;
    // fragment depth (api/fragments.inc.hip; the id check, the template sizes and the bitset are the template entry's
    // tp_*): the counters (qmcp_kernels.h: FragWord), the contig lengths, the sort's two key buffers and two index
    // columns, its histogram, the spine of its scans and of the segmented scan, and the clipped starts and contig ids of
    // the host entries and of the solve
    DevBuf fr_stat, fr_len, fr_keys[2], fr_vals[2], fr_hist, fr_spine, fr_cs, fr_cc;
    // ceiling solves (api/ceiling.inc.hip; need[] and the batch's regions are the profile's pf_need / pf_tab): a batch's
    // position offsets, the events of its dropped reads and their scan with its spine, and the call's counters
    DevBuf cl_poff, cl_depth, cl_spine, cl_stat;
    // proportional solves (api/proportional.inc.hip; need[] is the profile's pf_need): the call's counters
    // (qmcp_kernels.h: PropStat)
    DevBuf pp_stat;
    // budget and mean-depth solves (api/budget.inc.hip, api/mean_depth.inc.hip; laid out and searched by
    // api/cap_search.inc.hip), their own: the accumulators, the curve and the depth histogram in one buffer (CapAcc:
    // BudgetWord words | curve | histogram | mean-depth's MeanDepthWord words), and the second input-order mask of the probes
    DevBuf bg_acc, bg_mask;
    // mean-depth solves alone: the merged region table in contig coordinates (offs | rs | re | cum) followed by the
    // batches' form of it (rpos | rcum), and the reads' weights
    DevBuf md_tab, md_w;
    // coverage thresholds (api/thresholds.inc.hip), all its own: the input-order mask a coverage's solve (ProbeSolve,
    // api/cap_search.inc.hip) scatters into, the reads that have a threshold, the accumulators with the histogram behind
    // them (ThresholdsAccWord words | bins), and the host entry's thresholds
    DevBuf th_mask, th_seen, th_acc, th_thr;
    // disjoint replicates (api/replicates.inc.hip), all its own: the two sets of free reads' columns (starts, ends, input
    // indices) that ping-pong between replicates, the scanned word popcounts of the taken candidates and their spine, the
    // two offset tables, the candidates' taken bits, the input-order taken mask (whole pairs, several batches), the packed
    // mask of one label, the mates' counters, the host entry's label bytes and the device entry's first mask
    DevBuf rp_starts[2], rp_ends[2], rp_orig[2], rp_words, rp_spine, rp_offs[2], rp_kept, rp_taken, rp_lmask, rp_stat,
        rp_labels, rp_mask0;
    uint64_t mask_reads = 0;  // reads the context's own mask buffer (c->mask) currently describes
    DevBuf evpk, evlast;  // event-driven uniform sweep: packed block words, last-changed-block index per block
    uint32_t last_iters = 0, last_blocks = 0;
    // the two halves of a solve's enqueue (enqueue_head / enqueue_tail) and what they share
    SolveRun run;
    PinnedBuf<uint32_t> h_head;       // pinned landing zone of the read-back that picks the route (solve_words.h: Head)
    uint32_t* h_stats_init = nullptr; // in h_head, behind those words: the statistics' initial values (~0, then zeros)
    Event ev_head;                    // the solve's head (prepare, partition, bucket offsets) has been queued up to here
    Event ev_done;                    // everything of the solve has been queued up to here
    bool mixed_seen = false;          // a call took the mixed-span route: its arrays are sized up front from then on
    bool sized = false;               // the arena block of the current solve is behind us (growth now is growth mid-solve)
    uint32_t grew_mid_solve = 0;      // buffers that had to grow after the solve's first launch (stats.arena_grown_mid_solve)
    // optional per-kernel timing (qmcp_hip_set_profiling): one event pair per launch group
    int profiling = 0;  // 0 off, 1 every kernel, 2 the selection sweep only
    size_t tables_count = 0;          // contig tables currently on the device (upload_tables)
    void* tables_dev_roff = nullptr;
    void* tables_dev_poff = nullptr;
    struct Span { const char* name; Event a, b; };
    std::vector<Span> spans;          // spans of the solve in flight
    std::vector<Event> ev_pool;       // recycled events
    struct Acc { std::string name; uint64_t launches; double ms; };
    std::vector<Acc> acc;             // accumulated since the last reset
};

namespace {

hipEvent_t pool_event(qmcp_hip_ctx* c) {
    if (!c->ev_pool.empty()) {
        hipEvent_t e = c->ev_pool.back().release();
        c->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// two pooled events, returned to the pool when the scope ends
struct EventPair {
    qmcp_hip_ctx* c;
    hipEvent_t a, b;
    explicit EventPair(qmcp_hip_ctx* ctx) : c(ctx), a(pool_event(ctx)), b(pool_event(ctx)) {}
    ~EventPair() {
        if (a) c->ev_pool.emplace_back(a);
        if (b) c->ev_pool.emplace_back(b);
    }
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
};

// RAII bracket around one kernel (or one kernel + its helper launches) when profiling is on
struct KernelSpan {
    qmcp_hip_ctx* c;
    hipEvent_t a = nullptr, b = nullptr;
    const char* name;
    hipStream_t st;
    KernelSpan(qmcp_hip_ctx* ctx, const char* nm, hipStream_t stream = nullptr)
        : c(ctx), name(nm), st(stream ? stream : ctx->stream) {
        if (!c->profiling || !nm) return;  // (no name: no span -- a helper whose caller brackets differently)
        if (c->profiling == 2 && std::strncmp(nm, "k_sweep", 7) != 0) return;
        a = pool_event(c);
        b = pool_event(c);
        if (a) (void)hipEventRecord(a, st);
    }
    ~KernelSpan() {
        if (!c->profiling || !a || !b) return;
        (void)hipEventRecord(b, st);
        c->spans.push_back({name, Event(a), Event(b)});
    }
};

void collect_spans(qmcp_hip_ctx* c) {
    for (auto& sp : c->spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
            bool found = false;
            for (auto& a : c->acc)
                if (a.name == sp.name) { a.launches++; a.ms += ms; found = true; break; }
            if (!found) c->acc.push_back({sp.name, 1, ms});
        }
        c->ev_pool.push_back(std::move(sp.a));
        c->ev_pool.push_back(std::move(sp.b));
    }
    c->spans.clear();
}

int ensure(qmcp_hip_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return QMCP_OK;
    if (b.p) {
        if (c->sized) c->grew_mid_solve++;  // (after the solve's arena block: a stall on work already queued)
        // growing a buffer frees it: nothing queued on this context may still be using the old one
        // (hipFree would wait for the whole device anyway -- this names the wait and keeps it to the
        // one case where a later call is larger than every earlier one)
        if (c->stream) HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->stream2) HIP_TRY(hipStreamSynchronize(c->stream2));
        HIP_TRY(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    HIP_TRY(hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return QMCP_OK;
}

// The pinned counterpart: grow-only, no floor (a block nobody asked bytes for stays unallocated).  A regrown block
// holds nothing of the old one: what was last sent is compared on the host side of upload_tables / upload_pm_grid.
template <class T>
int ensure_pinned(qmcp_hip_ctx*, PinnedBuf<T>& b, size_t bytes) {
    if (b.cap >= bytes) return QMCP_OK;
    if (b.p) HIP_TRY(hipHostFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    HIP_TRY(hipHostMalloc((void**)&b.p, bytes, hipHostMallocDefault));
    b.cap = bytes;
    return QMCP_OK;
}

#define TRY(expr)                      \
    do {                               \
        int _rc = (expr);              \
        if (_rc != QMCP_OK) return _rc; \
    } while (0)

uint32_t bit_width(uint32_t v) { return v == 0 ? 0u : 32u - (uint32_t)__builtin_clz(v); }

int check_problem(const uint64_t* roff, const uint32_t* lengths, uint32_t n_contigs, uint64_t n,
                  Problem& pr) {
    if (!roff || !lengths || n_contigs == 0) return fail(QMCP_EINVAL, "contig tables missing or n_contigs == 0");
    if (roff[0] != 0 || roff[n_contigs] != n)
        return fail(QMCP_EINVAL, "contig_read_offsets must start at 0 and end at n_reads");
    pr.poff.assign((size_t)n_contigs + 1, 0);
    for (uint32_t c = 0; c < n_contigs; ++c) {
        if (roff[c + 1] < roff[c]) return fail(QMCP_EINVAL, "contig_read_offsets not monotone at %u", c);
        pr.poff[c + 1] = pr.poff[c] + lengths[c];
    }
    pr.n = n;
    pr.n_contigs = n_contigs;
    pr.ltot = pr.poff[n_contigs];
    if (n > (1ull << 30)) return fail(QMCP_ERANGE, "n_reads %llu exceeds 2^30 per call", (unsigned long long)n);
    if (pr.ltot > (1ull << 31) - 2)
        return fail(QMCP_ERANGE, "total contig length %llu exceeds 2^31-2", (unsigned long long)pr.ltot);
    return QMCP_OK;
}

int upload_tables(qmcp_hip_ctx* c, const uint64_t* roff, const Problem& pr) {
    const size_t count = (size_t)pr.n_contigs + 1;
    const size_t bytes = count * sizeof(uint64_t);
    TRY(ensure(c, c->roff, bytes));
    TRY(ensure(c, c->poff, bytes));
    // staged through pinned memory owned by the context: the copies are truly asynchronous and
    // nothing has to wait for them on the host (the previous solve has fully completed)
    TRY(ensure_pinned(c, c->h_tables, 2 * bytes));
    // the device copies stay valid across solves: skip the upload when nothing changed (a caller
    // that solves the same genome repeatedly saves two small copies per call)
    if (c->tables_count == count && c->tables_dev_roff == c->roff.p && c->tables_dev_poff == c->poff.p &&
        std::memcmp(c->h_tables, roff, bytes) == 0 &&
        std::memcmp(c->h_tables + count, pr.poff.data(), bytes) == 0)
        return QMCP_OK;
    std::memcpy(c->h_tables, roff, bytes);
    std::memcpy(c->h_tables + count, pr.poff.data(), bytes);
    c->tables_count = count;
    c->tables_dev_roff = c->roff.p;
    c->tables_dev_poff = c->poff.p;
    HIP_TRY(hipMemcpyAsync(c->roff.p, c->h_tables, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->poff.p, c->h_tables + count, bytes, hipMemcpyHostToDevice, c->stream));
    return QMCP_OK;
}

// The pass-major grid's tables, with the contig tables: one small copy, skipped while the grid stays what it was.
int upload_pm_grid(qmcp_hip_ctx* c, const qmcp::PmGridPlan& grid) {
    const size_t words = grid.words.size(), bytes = words * sizeof(uint32_t);
    TRY(ensure(c, c->pm_grid, bytes));
    TRY(ensure_pinned(c, c->h_pm_grid, bytes));
    if (c->pm_grid_dev == c->pm_grid.p && c->pm_grid_sent == grid.words) return QMCP_OK;
    std::memcpy(c->h_pm_grid, grid.words.data(), bytes);
    c->pm_grid_sent = grid.words;
    c->pm_grid_dev = c->pm_grid.p;
    HIP_TRY(hipMemcpyAsync(c->pm_grid.p, c->h_pm_grid, bytes, hipMemcpyHostToDevice, c->stream));
    return QMCP_OK;
}

// prepare + host round trip.  Leaves gstart (global start position per read) in vals[1] when
// want_keys; counts reads per start position into cstart (global atomics) only when
// want_counts -- the solve derives its bucket offsets from the sorted keys instead.
int run_prepare(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends,
                const Problem& pr, const uint64_t* d_keep_mask, bool want_keys, bool want_counts,
                bool want_part_hist, uint32_t part_shift, uint32_t* d_global_digit_hist,
                uint32_t host_stats[3]) {
    const uint32_t n = (uint32_t)pr.n;
    TRY(ensure(c, c->stats, 4 * sizeof(uint32_t)));
    if (want_counts) TRY(ensure(c, c->cstart, ((size_t)pr.ltot + 1) * sizeof(uint32_t)));
    if (want_keys) TRY(ensure(c, c->vals[1], (size_t)n * sizeof(uint32_t)));
    const uint32_t init[4] = {0xFFFFFFFFu, 0u, 0u, 0u};
    HIP_TRY(hipMemcpyAsync(c->stats.p, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    if (want_counts)
        HIP_TRY(hipMemsetAsync(c->cstart.p, 0, ((size_t)pr.ltot + 1) * sizeof(uint32_t), c->stream));
    {
        KernelSpan sp(c, "k_prepare");
        qmcp::launch_prepare(c->stream, d_starts, d_ends, n, c->roff.u64(), c->poff.u64(), pr.n_contigs, d_keep_mask,
                             want_keys ? c->vals[1].u32() : nullptr, want_counts ? c->cstart.u32() : nullptr,
                             c->stats.u32(), part_shift, want_part_hist ? c->hist2.u32() : nullptr, nullptr,
                             d_global_digit_hist, nullptr);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_stats, c->stats.p, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (host_stats[2] != 0)
        return fail(QMCP_EREAD, "a read has start > end or end >= its contig length");
    return QMCP_OK;
}

// The bytes of launch_exclusive_scan's spine over n entries; `more` further entries where a site has always asked for
// them (most ask for one).
size_t scan_spine_bytes(uint32_t n, uint32_t more = 0) {
    return (size_t)(qmcp::scan_spine_entries(n) + more) * sizeof(uint32_t) + 16;
}

// The rank of every bit of a mask, one step: the words' popcounts, scanned in place (exclusive, the total behind the
// last word).  queue_mask_ranks only queues the two launches, for buffers sized ahead of a loop or with the rest of a
// call's arena; mask_ranks sizes `ranks` ((words + 2) words) and `spine` first.  Neither opens a span.
void queue_mask_ranks(hipStream_t st, const uint64_t* mask, uint32_t words, const DevBuf& ranks, const DevBuf& spine) {
    qmcp::launch_word_popcounts(st, mask, words, ranks.u32());
    qmcp::launch_exclusive_scan(st, ranks.u32(), words, ranks.u32(), spine.u32(), true);
}

int mask_ranks(qmcp_hip_ctx* c, hipStream_t st, const uint64_t* mask, uint32_t words, DevBuf& ranks, DevBuf& spine) {
    TRY(ensure(c, ranks, ((size_t)words + 2) * sizeof(uint32_t)));
    TRY(ensure(c, spine, scan_spine_bytes(words + 1, 1)));
    queue_mask_ranks(st, mask, words, ranks, spine);
    return QMCP_OK;
}

int scan_counts(qmcp_hip_ctx* c, DevBuf& counts, DevBuf& out, uint32_t ltot) {
    TRY(ensure(c, out, ((size_t)ltot + 1) * sizeof(uint32_t)));
    TRY(ensure(c, c->spine, scan_spine_bytes(ltot)));
    {
        KernelSpan sp(c, "scan_positions(3 kernels)");
        qmcp::launch_exclusive_scan(c->stream, counts.u32(), ltot, out.u32(), c->spine.u32(), true);
    }
    HIP_TRY(hipGetLastError());
    return QMCP_OK;
}

// the ranked path is taken when no position range holds more than 1/kRankBalance of the reads:
// a range's ranking is one wave's serial walk (~0.65 ns per read) against ~0.03 ns per read for
// the radix sort it replaces
constexpr uint64_t kRankBalance = 24;
// ... and when the call is large enough for a per-range workgroup to have work (QMCP_HIP_RANK_MIN
// overrides, for experiments)
static uint32_t rank_min_reads(const qmcp_hip_ctx* c) { return c->opt.rank_min_reads ? c->opt.rank_min_reads : (1u << 17); }

float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0.f;
    return ms;
}
