/*
 * qmcp_hip.h -- C ABI of the MI355X-native quasi-MCP coverage-downsampling solver.
 *
 * This is the drop-in boundary for the one hot path this repository accelerates:
 * the `-a quasi-mcp-*` solver behind the reference's plugin surface
 *
 *     qmcp::Solver::solve(uint32_t max_coverage, bam_api::BamApi&)
 *         -> std::unique_ptr<std::vector<bam_api::ReadIndex>>
 *     (reference: libs/qmcp-solver/include/qmcp-solver/solver.hpp:13-20,
 *      registered by name in src/solver_manager.hpp:18-27).
 *
 * The reference has no FFI of its own (it is one C++ binary).  A maintainer drops
 * this library in by adding one `qmcp::Solver` subclass that narrows
 * `SOAPairedReads::start_inds/end_inds` (libs/bam-api/include/bam-api/soa_paired_reads.hpp:19-24)
 * to uint32 and calls `qmcp_hip_solve_host`; that adapter ships in
 * genome-downsampler_amd/host/ and is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types cross this boundary
 *   - read i is the inclusive interval [starts[i], ends[i]] on its contig
 *     (end_ind is inclusive in the reference: libs/bam-api/src/read.cpp:13)
 *   - reads are grouped by contig: contig c owns reads
 *     [contig_read_offsets[c], contig_read_offsets[c+1]); n_contigs == 1 reproduces the
 *     reference exactly (it is single-contig: libs/bam-api/src/bam_api.cpp:422).  Reads in any
 *     order with a contig id each take qmcp_hip_solve_by_contig_host / _device (at the end)
 *   - the result is a keep bitmask: bit (i & 63) of word (i >> 6) is set iff read i is kept;
 *     expanding it in ascending order gives the reference's `Solution` vector
 *     (quasi_mcp_cpu_max_flow_solver.cpp:89-100)
 *   - every function returns QMCP_OK (0) or a negative QMCP_E* code; the message for the
 *     calling thread's last failure is available from qmcp_hip_last_error().  Nothing here
 *     terminates the process (the reference's CUDA path calls std::terminate():
 *     libs/qmcp-solver/include/qmcp-solver/cuda_helpers.cuh:13-22 -- the C++ adapter
 *     re-creates that behaviour on top of the status code).
 *   - there is no CPU fallback: without a usable HIP device every entry point fails.
 */
#ifndef QMCP_HIP_H
#define QMCP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QMCP_HIP_ABI_VERSION 5

enum {
    QMCP_OK = 0,
    QMCP_EINVAL = -1,      /* bad argument (null pointer, n_contigs == 0, offsets not monotone ...) */
    QMCP_EREAD = -2,       /* a read has start > end or end >= contig length                       */
    QMCP_ERANGE = -3,      /* problem exceeds the 32-bit coordinate / count limits of this build   */
    QMCP_ENODEVICE = -4,   /* no HIP device / device index out of range                            */
    QMCP_EHIP = -5,        /* a HIP runtime call failed (message has the hipError string)          */
    QMCP_ENOMEM = -6       /* device or host allocation failed                                     */
};

/* Selection paths the solver can take per call (reported in qmcp_hip_stats.path). */
enum {
    QMCP_PATH_NONE = 0,
    QMCP_PATH_UNIFORM = 1, /* all reads of the call have one span: block-parallel sweep            */
    QMCP_PATH_GENERAL = 2, /* mixed spans: event-driven priority sweep                             */
    QMCP_PATH_NEAR_UNIFORM = 3 /* one dominant span and a few shorter reads on deep data: the one-span sweep
                                  over the regular reads, the others selected as verified exceptions       */
};

/* Opaque solver context: owns one HIP stream and a reusable device arena.  Mirrors the
 * lifetime rules of a reference solver instance (constructed once, `solve` called many
 * times: src/tests/coverage_tester.cpp:30-34); creating it is the first and only point
 * where the GPU is touched (reference solvers are constructed eagerly even for --help:
 * src/app.hpp:35, so the C++ adapter creates the context lazily on first solve). */
typedef struct qmcp_hip_ctx qmcp_hip_ctx;

typedef struct qmcp_hip_stats {
    uint64_t n_reads;
    uint64_t n_kept;          /* popcount of the keep mask                                        */
    uint64_t total_length;    /* sum of contig lengths                                            */
    uint32_t n_contigs;
    uint32_t path;            /* QMCP_PATH_*                                                      */
    uint32_t min_span;        /* min / max of (end - start + 1) over the call                     */
    uint32_t max_span;
    uint32_t sort_passes;     /* radix passes of the bucketing stage (1 = one range partition,    */
                              /* the large uniform-span route; >= 2 = LSD radix sort)             */
    uint32_t sweep_stretches; /* chains the sweep ran side by side: the non-empty contigs, or more    */
                              /* where cut points (coverage <= M) split them                       */
    float ms_total;           /* device time of the whole solve (HIP events on the solver stream) */
    float ms_prepare;         /* validate + span reduction + per-position start/end counts        */
    float ms_scan;            /* prefix scans -> bucket offsets / coverage                        */
    float ms_sort;            /* radix bucketing of reads by (start, span)                        */
    float ms_sweep;           /* selection sweep                                                  */
    float ms_mark;            /* keep-mask emission                                               */
    float ms_h2d;             /* host entry point only                                            */
    float ms_d2h;             /* host entry point only                                            */
    uint32_t columns_sent;    /* host entry points only: 1 = every read has one span, only the starts
                                 crossed the link and the device rebuilt the ends; 2 = both columns  */
    uint32_t spec_boundaries; /* stretches that started at a speculative boundary (data a few times
                                 deeper than M: no cut point, but the sweep forgets its start)      */
    uint32_t spec_mismatches; /* of those, how many disagreed with the stretch before them: the parts
                                 of the genome they lie in were swept again with three times the
                                 run-in                                                              */
    uint32_t spec_retry_mismatches; /* ... and how many disagreed in that sweep: those parts were
                                 swept exactly                                                       */
    uint32_t sweep_blocks_changed; /* event-driven sweep (deep data): blocks of one read length's positions that
                                 changed the kept profile -- the chain's serial work is ~170 instructions per
                                 changed block + ~60 per 16 blocks tested; block-scan sweeps: blocks redone in
                                 the general form                                                     */
    uint32_t sweep_blocks;    /* ... of this many blocks swept                                       */
    uint32_t arena_grown_mid_solve; /* device buffers that had to grow after the solve's first launch (a
                                 stall on queued work); 0 from the second call of a shape on         */
    uint32_t near_uniform_exceptions; /* QMCP_PATH_NEAR_UNIFORM (also when the route was tried and given up for
                                 the mixed-span one): reads shorter than the dominant span            */
    uint32_t near_uniform_selected;   /* ... of those, kept                                              */
    uint32_t near_uniform_rounds;     /* ... sweeps it took (1 = no exception was wanted by the sweep)   */
    uint32_t near_uniform_giveup;     /* 0, or why the route handed the call to the mixed-span one: QMCP_NU_GIVEUP_* */
    int32_t pm_grid;                  /* pass-major form of the range-ranked route: the grid its ranges were cut on, -1 the
                                 global axis, +1 aligned to the contigs' starts; 0: the form did not run             */
    uint32_t pm_heaviest_wave_slots;  /* ... and the wave-slots (groups of 64 padded record slots) of its heaviest range:
                                 what the per-range kernels' slowest workgroup walks                                */
} qmcp_hip_stats;

/* qmcp_hip_stats.near_uniform_giveup */
enum {
    QMCP_NU_GIVEUP_NONE = 0,
    QMCP_NU_GIVEUP_NOT_TRIED = 1,      /* switched off, small call, span or M outside the event-driven sweep, too shallow */
    QMCP_NU_GIVEUP_LONGER_READS = 2,   /* the dominant span is not the longest (a deletion lengthens a read)              */
    QMCP_NU_GIVEUP_TOO_MANY = 3,       /* more than a tenth of the reads are exceptions, or the list overflowed           */
    QMCP_NU_GIVEUP_HEAVY_RANGE = 4,    /* one position range holds too many reads for the ranked route                    */
    QMCP_NU_GIVEUP_UNMODELLED = 5,     /* a run of used-up buckets without an anchor, or too many suspects / neighbours   */
    QMCP_NU_GIVEUP_BUDGET = 6,         /* the rounds did not settle within the budget                                     */
    QMCP_NU_GIVEUP_REMEMBERED = 7      /* an earlier call of this shape on this context did not settle                    */
};

int qmcp_hip_abi_version(void);
const char* qmcp_hip_last_error(void);

/* Number of HIP devices visible to the process (0 if none); never initialises a context. */
int qmcp_hip_device_count(void);

int qmcp_hip_create(int device, qmcp_hip_ctx** out_ctx);
void qmcp_hip_destroy(qmcp_hip_ctx* ctx);

/* Per-context options: which of the (all exact) kernels and routes a solve takes where the library would otherwise
 * choose by the data, and the host entries' threads -- the counterpart of the reference solver's setters
 * (libs/qmcp-solver/include/qmcp-solver/quasi_mcp_cuda_max_flow_solver.hpp:30-31: set_block_size, set_kernel_cycles).
 * Every choice gives the same keep mask; the options exist for tests (every route is forced and compared with the
 * oracle), measurements and debugging.  0 means "the library chooses" in every field.
 * qmcp_hip_create initialises a context's options from the defaults and then from the environment variables named below
 * (a debug override, read once, there and nowhere else); qmcp_hip_set_options replaces them. */
typedef struct qmcp_hip_options {
    uint32_t struct_size;         /* sizeof(qmcp_hip_options) of the caller's build (the struct may grow at its end)      */
    int32_t pass_major;           /* range-ranked route: -1 the range-major form, +1 the pass-major form wherever its hard
                                     limits allow (QMCP_HIP_PM=0|1)                                                       */
    int32_t sweep;                /* one-length sweep: QMCP_SWEEP_* (QMCP_HIP_SWEEP=fast|gen|ev)                          */
    int32_t cut_points;           /* split contigs at cut points: -1 never, +1 always (QMCP_HIP_CUTS=0|1)                 */
    int32_t speculation;          /* speculative stretch boundaries: -1 never, +1 at any depth (QMCP_HIP_SPEC=0|1)        */
    uint32_t speculation_run_in;  /* blocks of run-in of the first tier (QMCP_HIP_SPEC_BURN)                              */
    int32_t near_uniform;         /* near-uniform route: -1 off (QMCP_HIP_NEAR=0)                                         */
    uint32_t near_uniform_rounds; /* its budget of rounds (QMCP_HIP_NEAR_ROUNDS)                                          */
    float near_uniform_min_depth; /* sigma depth below which it is not tried (default 1.5: DESIGN.md 4.1; the mean coverage in
                                     units of M where M = 50) (QMCP_HIP_NEAR_MIN_DEPTH)                                  */
    int32_t near_uniform_debug;   /* 1: what every pair of rounds did, to stderr (QMCP_HIP_NEAR_DEBUG); 2 (lab): the rounds
                                     after the first sweep every stretch again, not only those a selection reaches     */
    int32_t force_sort_route;     /* 1: the keep mask from the radix sort even where the ranked route applies
                                     (QMCP_HIP_NO_RANK)                                                                   */
    int32_t keep_expand;          /* 1: the event-driven sweep always expands its output (QMCP_HIP_EXPAND)                */
    int32_t mixed_sweep_in_lds;   /* 1: the LDS-cached mixed-span sweep instead of the register-resident one
                                     (QMCP_HIP_GENERAL_LDS)                                                               */
    uint32_t rank_min_reads;      /* calls below this many reads take the sort-based route (QMCP_HIP_RANK_MIN; 2^17)      */
    uint32_t host_threads;        /* host entries: threads that narrow / check the columns (QMCP_HIP_HOST_THREADS; 8)     */
    uint32_t copy_streams;        /* host entries: copy streams (QMCP_HIP_COPY_STREAMS)                                   */
    int32_t host_both_columns;    /* 1: host entries always send starts AND ends (QMCP_HIP_HOST_BOTH_COLUMNS)             */
    int32_t pm_grid;              /* pass-major form: where its ranges are cut -- -1 on the global axis, +1 at the contigs'
                                     starts wherever that still fits 256 ranges; 0: there, if the heaviest range comes out
                                     lighter (QMCP_HIP_PM_GRID=-1|1)                                                       */
} qmcp_hip_options;
enum { QMCP_SWEEP_AUTO = 0, QMCP_SWEEP_FAST = 1, QMCP_SWEEP_GENERAL = 2, QMCP_SWEEP_EVENTS = 3 };
void qmcp_hip_default_options(qmcp_hip_options* out);            /* all zero but struct_size                          */
int qmcp_hip_set_options(qmcp_hip_ctx* ctx, const qmcp_hip_options* options);
int qmcp_hip_get_options(qmcp_hip_ctx* ctx, qmcp_hip_options* out);

/* Instrumentation (the reference's only timing is the "solve took" wall-clock log line,
 * src/app.cpp:132-139).  With profiling on, kernel launches of a solve are bracketed by HIP events
 * on the stream they run on: enabled == 1 every kernel, enabled == 2 only the selection sweep (the
 * event records cost a few microseconds of device idle time per bracket).
 * qmcp_hip_kernel_times writes one line per kernel, "name<TAB>launches<TAB>total_ms", accumulated
 * since profiling was last switched on, and returns the number of lines (negative on error). */
int qmcp_hip_set_profiling(qmcp_hip_ctx* ctx, int enabled);
int qmcp_hip_kernel_times(qmcp_hip_ctx* ctx, char* buf, size_t cap);

/* Replaces QuasiMcpCpuMaxFlowSolver::solve / QuasiMcpCudaMaxFlowSolver::solve
 * (libs/qmcp-solver/src/quasi_mcp_cpu_max_flow_solver.cpp:11-28,
 *  libs/qmcp-solver/src/quasi_mcp_cuda_max_flow_solver.cu:319-435) for host-resident reads.
 * keep_mask_out has ceil(n_reads / 64) words and is fully overwritten.  stats may be NULL.
 * Limits (QMCP_ERANGE beyond them): 2^30 reads and 2^31 - 2 bases per call; reads of one length per
 * call take the block sweep (any length up to 512 bases, longer ones and any mix of lengths the event
 * sweeps, reads up to 2^24 - 1 bases); 2^28 reads per contig on the block sweep. */
int qmcp_hip_solve_host(qmcp_hip_ctx* ctx,
                        const uint32_t* starts, const uint32_t* ends, uint64_t n_reads,
                        const uint64_t* contig_read_offsets, const uint32_t* contig_lengths,
                        uint32_t n_contigs, uint32_t max_coverage,
                        uint64_t* keep_mask_out, qmcp_hip_stats* stats);

/* The same for callers that hold the reference's own columns: SOAPairedReads::start_inds / end_inds are
 * std::vector<size_t> (libs/bam-api/include/bam-api/soa_paired_reads.hpp:19-24, read.hpp:11-13), i.e.
 * 64-bit.  The narrowing to uint32 (the reference's CUDA solver narrows too:
 * quasi_mcp_cuda_max_flow_solver.hpp:19) runs here, chunk by chunk on several host threads into pinned
 * staging owned by the context, each chunk's host-to-device copy issued as soon as it is narrowed, so
 * the span the reference times as "solve took" (src/app.cpp:132-139) is the PCIe transfer plus little.
 * A coordinate above 2^32 - 1 fails with QMCP_ERANGE.  When every read of the call has one span (checked
 * on all of them while they are narrowed) only the starts cross the link and the device rebuilds the
 * ends; qmcp_hip_solve_host does the same for calls of 2^20 reads or more (host threads check while
 * the starts are copied).  `breakdown` (may be NULL) receives host wall-clock milliseconds of the
 * call's parts. */
typedef struct qmcp_hip_host_breakdown {
    float ms_total;        /* the whole call                                                        */
    float ms_narrow_h2d;   /* narrowing + host-to-device copies (overlapped with each other)        */
    float ms_solve;        /* enqueue to completion of the device solve                             */
    float ms_d2h;          /* keep mask to the host                                                 */
    uint32_t host_threads; /* threads that narrowed                                                 */
    uint32_t chunks;
    uint32_t columns_sent; /* 1: every read has one span, only the starts crossed the link (the device
                              rebuilt the ends); 2: starts and ends                                   */
} qmcp_hip_host_breakdown;
int qmcp_hip_solve_host64(qmcp_hip_ctx* ctx,
                          const uint64_t* start_inds, const uint64_t* end_inds, uint64_t n_reads,
                          const uint64_t* contig_read_offsets, const uint32_t* contig_lengths,
                          uint32_t n_contigs, uint32_t max_coverage,
                          uint64_t* keep_mask_out, qmcp_hip_stats* stats,
                          qmcp_hip_host_breakdown* breakdown);

/* Solution of the last qmcp_hip_solve_host / _host64 / complete_pairs_host call on this context as the
 * reference returns it: the ascending ReadIndex list of obtain_sequence
 * (quasi_mcp_cpu_max_flow_solver.cpp:89-100), expanded from the context's keep mask on the device
 * (per-word popcounts, a scan, one scatter) and copied out -- for a plugin adapter this replaces a host
 * loop over the mask.  `capacity` entries at least stats.n_kept; *n_out receives the count. */
int qmcp_hip_kept_indices_host(qmcp_hip_ctx* ctx, uint64_t n_reads, uint64_t* indices_out, uint64_t capacity,
                               uint64_t* n_out);

/* Same solve with reads and mask already resident in this context's device memory
 * (d_* are device pointers; contig tables stay on the host).  `hip_stream` is a
 * hipStream_t the caller's producer work was enqueued on, or NULL: the solve is ordered
 * after it and the call returns after the solve has completed on the device. */
int qmcp_hip_solve_device(qmcp_hip_ctx* ctx,
                          const uint32_t* d_starts, const uint32_t* d_ends, uint64_t n_reads,
                          const uint64_t* contig_read_offsets, const uint32_t* contig_lengths,
                          uint32_t n_contigs, uint32_t max_coverage,
                          uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats);

/* The same solve in two halves, for callers that keep more than one solve in flight (one per
 * context: two contexts on one device let the selection sweep of one call -- a serial chain on a
 * few compute units -- run beside the bandwidth-bound stages of the next).  _begin orders the solve
 * after `hip_stream`, enqueues all of it and returns without waiting for the device (it does wait
 * for one 16-byte read-back that picks the kernels; the device keeps working on other contexts
 * meanwhile).  That holds for calls whose reads have ONE length (QMCP_PATH_UNIFORM).  A call with other
 * lengths is decided by what the device finds: on QMCP_PATH_NEAR_UNIFORM the FIRST call of a shape (reads, positions,
 * dominant length, M) waits for the device two to three times and once more per pair of rounds (each round's outcome
 * decides whether another is queued) -- _begin then returns when most of the solve has RUN.  The context remembers in
 * how many rounds the shape settled (up to eight), and the next call of it queues that many rounds and the ranking
 * behind them without looking: _begin returns at once again, _end looks at the route's state words and, should
 * the call have needed more rounds than were queued, solves it again the blocking way before it returns (bench.py
 * reports both rates for cfg4 with 1 % of the reads shortened: other_configs.cfg4_1pct_clipped.pipelined_ms 1.75
 * against device_ms 2.27; before round 4's second half 2.24).  On QMCP_PATH_GENERAL _begin waits once more where it
 * samples the lengths.  A context's first call
 * of a shape may also grow its arena after work is queued (stats.arena_grown_mid_solve), which waits for every
 * stream of the context; the second call of the shape does not.  _end waits for the solve and fills `stats`.  One pending solve per context: a second
 * _begin, or any other entry point of the same context, before _end fails with QMCP_EINVAL.
 * The reference has no counterpart: its solve is one blocking call (src/app.cpp:132-139). */
int qmcp_hip_solve_device_begin(qmcp_hip_ctx* ctx,
                                const uint32_t* d_starts, const uint32_t* d_ends, uint64_t n_reads,
                                const uint64_t* contig_read_offsets, const uint32_t* contig_lengths,
                                uint32_t n_contigs, uint32_t max_coverage,
                                uint64_t* d_keep_mask_out, void* hip_stream);
int qmcp_hip_solve_end(qmcp_hip_ctx* ctx, qmcp_hip_stats* stats);

/* Several devices behind one call (the reference has no counterpart: src/solver_manager.hpp:18-27
 * registers single-device solvers).  Contigs are independent problems (the reference is single-contig,
 * libs/bam-api/src/bam_api.cpp:422), so they are dealt to the devices -- by a cost of reads plus the
 * longest contig a device owns (its sweep chains run side by side), longest-processing-time first --
 * and every device solves its share in its own context on its own host thread: no data-path exchange
 * between devices.  The per-device keep masks are merged into global ReadIndex bit positions on the
 * host (contig boundaries need not be multiples of 64).  `devices` may name a device more than once
 * (separate contexts on it).  per_device_stats: n_devices entries or NULL; contig_device_out:
 * n_contigs entries (index into `devices`) or NULL. */
typedef struct qmcp_hip_multi qmcp_hip_multi;
int qmcp_hip_multi_create(const int* devices, int n_devices, qmcp_hip_multi** out);
void qmcp_hip_multi_destroy(qmcp_hip_multi* m);
int qmcp_hip_multi_solve_host(qmcp_hip_multi* m,
                              const uint32_t* starts, const uint32_t* ends, uint64_t n_reads,
                              const uint64_t* contig_read_offsets, const uint32_t* contig_lengths,
                              uint32_t n_contigs, uint32_t max_coverage,
                              uint64_t* keep_mask_out, qmcp_hip_stats* per_device_stats,
                              int* contig_device_out);

/* Stage probe for parity tests of the deterministic half of the reference solver:
 * writes cov[p] for every base of every contig (contigs concatenated, sum(contig_lengths)
 * entries) -- the array BamApi::find_input_cover returns (libs/bam-api/src/bam_api.cpp:275-286)
 * and from which b and d of create_b_function / create_demand_function
 * (quasi_mcp_cpu_max_flow_solver.cpp:58-87) follow as b[p+1] = min(cov[p], M). */
int qmcp_hip_coverage_host(qmcp_hip_ctx* ctx,
                           const uint32_t* starts, const uint32_t* ends, uint64_t n_reads,
                           const uint64_t* contig_read_offsets, const uint32_t* contig_lengths,
                           uint32_t n_contigs, uint32_t* cov_out);

/* Coverage of the kept subset only (BamApi::find_filtered_cover, bam_api.cpp:288-301);
 * keep_mask is a host bitmask as produced by qmcp_hip_solve_host. */
int qmcp_hip_filtered_coverage_host(qmcp_hip_ctx* ctx,
                                    const uint32_t* starts, const uint32_t* ends, uint64_t n_reads,
                                    const uint64_t* contig_read_offsets,
                                    const uint32_t* contig_lengths, uint32_t n_contigs,
                                    const uint64_t* keep_mask, uint32_t* cov_out);

/* Stage probe: the capped coverage b and the demand d of the reference's flow network for one
 * contig, computed on the device -- create_b_function (quasi_mcp_cpu_max_flow_solver.cpp:58-73):
 * b[0] = 0, b[p + 1] = min(cov[p], M); create_demand_function (:75-87): d[0] = -b[1],
 * d[i] = b[i] - b[i + 1] for 1 <= i < n, d[n] = b[n].  Both outputs have ref_genome_length + 1
 * entries (the reference's std::vector<int>). */
int qmcp_hip_demand_host(qmcp_hip_ctx* ctx,
                         const uint32_t* starts, const uint32_t* ends, uint64_t n_reads,
                         uint32_t ref_genome_length, uint32_t max_coverage,
                         int32_t* b_out, int32_t* d_out);

/* BamApi::find_pairs (libs/bam-api/src/bam_api.cpp:239-273) on the bitmask: mates sit at
 * indices (2q, 2q+1) (bam_api.cpp:456-461), so completing pairs is an OR inside each
 * aligned bit pair.  In place on a device mask of ceil(n_reads/64) words. */
int qmcp_hip_complete_pairs_device(qmcp_hip_ctx* ctx, uint64_t* d_keep_mask, uint64_t n_reads,
                                   void* hip_stream);
int qmcp_hip_complete_pairs_host(qmcp_hip_ctx* ctx, uint64_t* keep_mask, uint64_t n_reads);

/* Amplicon FILTER pre-pass (BamApi::should_be_filtered_out with AmpliconBehaviour::FILTER,
 * libs/bam-api/src/bam_api.cpp:311-319; Amplicon::includes amplicon.cpp:5-7;
 * AmpliconSet::member_includes_both amplicon_set.cpp:5-9; min length / min MAPQ
 * bam_api.cpp:321-327).  Pair q = reads (2q, 2q+1).  pair_keep_out gets one bit per pair:
 * set iff the pair survives (both mates inside one amplicon [amp_start, amp_end] inclusive,
 * both seq_lengths >= min_length, both qualities >= min_mapq).  seq_lengths / qualities may
 * be NULL (that filter is then skipped, as with the reference's defaults of 0). */
int qmcp_hip_amplicon_filter_host(qmcp_hip_ctx* ctx,
                                  const uint32_t* starts, const uint32_t* ends,
                                  const uint32_t* seq_lengths, const uint32_t* qualities,
                                  uint64_t n_reads,
                                  const uint32_t* amp_starts, const uint32_t* amp_ends,
                                  uint32_t n_amplicons, uint32_t min_length, uint32_t min_mapq,
                                  uint64_t* pair_keep_out);

/* The device-resident part of App::execute around the solver (src/app.cpp:113-142) for one
 * contig, in one call: FILTER pre-pass as in qmcp_hip_amplicon_filter_host (n_amplicons == 0
 * skips the amplicon predicate, i.e. AmpliconBehaviour::IGNORE; seq_lengths / qualities may be
 * NULL), compaction of the surviving pairs on the device (what BamApi does while ingesting:
 * only accepted pairs are appended, bam_api.cpp:434-461), the solve on the survivors, optional
 * mate completion (BamApi::find_pairs, src/app.cpp:141), and the result expressed over the
 * ORIGINAL read indices.  keep_mask_out: ceil(n_reads/64) words.  pairs_filtered_out (may be
 * NULL) receives the number of pairs the pre-pass dropped (BamApi::get_filtered_out_reads
 * counts their reads).  n_reads must be even (whole pairs). */
int qmcp_hip_filter_solve_host(qmcp_hip_ctx* ctx,
                               const uint32_t* starts, const uint32_t* ends,
                               const uint32_t* seq_lengths, const uint32_t* qualities,
                               uint64_t n_reads,
                               const uint32_t* amp_starts, const uint32_t* amp_ends,
                               uint32_t n_amplicons, uint32_t min_length, uint32_t min_mapq,
                               uint32_t ref_genome_length, uint32_t max_coverage, int complete_pairs,
                               uint64_t* keep_mask_out, uint64_t* pairs_filtered_out,
                               qmcp_hip_stats* stats);

/* Reads of SEVERAL references in any order -- a multi-reference BAM in file (or pairing) order -- with one contig id per
 * read: contig_ids[i] < n_contigs names read i's contig (contig c has contig_lengths[c] positions), QMCP_NO_CONTIG marks
 * an unplaced read, which is left out of every problem and never kept.  Every other convention is the one above: read i
 * is [starts[i], ends[i]] on its contig, and keep_mask_out (ceil(n_reads / 64) words, fully overwritten) is in INPUT order.
 * The mask equals solving each contig, on its own reads in input order, as one call of qmcp_hip_solve_host.
 * How: the ids are checked and the reads grouped by contig on the device once (a stable LSD radix sort of the ids, one
 * pass per 8 bits of n_contigs); the contigs are packed, in id order, into batches within the per-call limits above
 * (2^30 reads, 2^31 - 2 positions), which run back to back on this context; each batch's mask is scattered back to
 * input order.  So a whole genome (GRCh38: 3.1 Gbp) is one call.  Limits: 2^31 reads, 2^24 contigs; one contig over a
 * per-call limit fails with QMCP_ERANGE and a message naming it.  An id that is neither < n_contigs nor QMCP_NO_CONTIG
 * fails with QMCP_EINVAL, a placed read with start > end or end >= its contig's length with QMCP_EREAD.
 * stats (may be NULL) are summed over the batches: n_reads counts the placed reads, n_contigs and total_length every
 * contig, the times every batch; path, min_span / max_span and the route fields are those of the batch with the most
 * reads (min / max over all batches for the spans).  The host entry leaves the input-order mask in the context, for
 * qmcp_hip_kept_indices_host and qmcp_hip_complete_pairs_host. */
#define QMCP_NO_CONTIG 0xFFFFFFFFu
int qmcp_hip_solve_by_contig_host(qmcp_hip_ctx* ctx,
                                  const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                  uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                  uint32_t max_coverage, uint64_t* keep_mask_out, qmcp_hip_stats* stats);
/* The same with the three columns and the mask in device memory (contig_lengths stays on the host); ordered after
 * `hip_stream` (or NULL) as qmcp_hip_solve_device is, and returns after the solve has completed on the device. */
int qmcp_hip_solve_by_contig_device(qmcp_hip_ctx* ctx,
                                    const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                    uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                    uint32_t max_coverage, uint64_t* d_keep_mask_out, void* hip_stream,
                                    qmcp_hip_stats* stats);

/* qmcp_hip_filter_solve_host for pairs on SEVERAL references, amplicons matched to each read's own reference: the
 * FILTER, a stable compaction of the surviving pairs, qmcp_hip_solve_by_contig_host on them, optional mate completion,
 * and the keep mask in INPUT order (keep_mask_out: ceil(n_reads / 64) words, fully overwritten).  n_reads must be even:
 * pair q is reads 2q, 2q + 1.  contig_ids / contig_lengths / n_contigs as in qmcp_hip_solve_by_contig_host.
 * Amplicons: amp_offsets (n_contigs + 1 entries, starting at 0, never decreasing) gives contig c the amplicons
 * [amp_offsets[c], amp_offsets[c + 1]) of amp_starts / amp_ends, inclusive bounds, in any order (duplicates and nested
 * amplicons allowed).  A pair survives iff both mates are placed on the same contig c, one amplicon of c contains both
 * mates (Amplicon::includes), and both pass min_length on seq_lengths and min_mapq on qualities (either may be NULL:
 * that filter is off).  So pairs with mates on different contigs, with an unplaced mate, or on a contig without
 * amplicons are dropped.  amp_offsets == NULL is AmpliconBehaviour::IGNORE: only the length / MAPQ filters act, and a
 * pair with an unplaced or a cross-contig mate survives; an unplaced read is never selected itself, but with
 * complete_pairs it comes back as the mate of a kept read -- as in the per-reference file flow.
 * The result equals qmcp_hip_filter_solve_host run on each contig's surviving same-contig pairs in input order.
 * Every read is validated, those of dropped pairs included: an id that is neither < n_contigs nor QMCP_NO_CONTIG fails
 * with QMCP_EINVAL, a placed read with start > end or end >= its contig's length with QMCP_EREAD; bad amp_offsets and an
 * odd n_reads with QMCP_EINVAL.  Limits: 2^31 reads, 2^24 contigs.  pairs_filtered_out (may be NULL) receives the
 * number of dropped pairs; stats follow qmcp_hip_solve_by_contig_host (summed over its batches, n_reads = the placed
 * surviving reads).  The final mask stays in the context for qmcp_hip_kept_indices_host. */
int qmcp_hip_filter_solve_by_contig_host(qmcp_hip_ctx* ctx,
                                         const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                         const uint32_t* seq_lengths, const uint32_t* qualities, uint64_t n_reads,
                                         const uint32_t* contig_lengths, uint32_t n_contigs,
                                         const uint32_t* amp_offsets, const uint32_t* amp_starts,
                                         const uint32_t* amp_ends, uint32_t min_length, uint32_t min_mapq,
                                         uint32_t max_coverage, int complete_pairs, uint64_t* keep_mask_out,
                                         uint64_t* pairs_filtered_out, qmcp_hip_stats* stats);

/* Quality-aware selection: the solver the reference would register with uses_quality_of_reads() == true (its qmcp-cpu
 * weighs reads by quality; src/app.cpp:120-128 then grades amplicon pairs instead of filtering them).  A CELL is the
 * set of placed reads of one call that share (contig, start, end): reads of a cell are interchangeable for coverage.
 * Let K be the mask qmcp_hip_solve_host (resp. qmcp_hip_solve_by_contig_host) returns for the same call and
 * c = |K n C| for every cell C.  These entries return the mask Q that keeps, in every cell, the c reads that come first
 * in the order (quality descending, read index ascending), and nothing else -- the canonical selection with its last
 * key "smallest index" replaced by "highest quality, then smallest index".  So Q has the same per-position coverage and
 * the same number of reads as K (a valid, minimum-cardinality maximum-flow support, like K), a cell whose reads share
 * one quality is unchanged (all qualities equal: Q == K bit for bit), and every cell's kept quality is the largest
 * possible.  Not claimed: the optimum of the reference's min-cost objective (qmcp-cpu), which may trade reads for
 * other intervals or for more reads.
 * qualities: one uint32 per read (MAPQ, or the graded quality of AmpliconBehaviour::GRADE), NULL fails with
 * QMCP_EINVAL before anything else; a range (max - min over the placed reads) above 65535 fails with QMCP_ERANGE, found
 * before the solve runs: the output mask is then not written.  Every other argument,
 * limit and error is that of the plain entry; stats (may be NULL) are the plain solve's, qstats (may be NULL) the pass's.
 * The pass runs after the solve on the same stream and before anything else; it is blocking (no _begin / _end form).
 * The host entries leave the final mask in the context, for qmcp_hip_kept_indices_host and
 * qmcp_hip_complete_pairs_host.  For the by-contig entry the cell includes the contig and QMCP_NO_CONTIG reads are
 * never kept. */
typedef struct qmcp_hip_quality_stats {
    uint32_t quality_min, quality_max; /* over the placed reads                                                   */
    uint32_t key_bits, sort_passes;    /* 0 passes: all qualities equal (or no read kept, or every read kept): the
                                          mask is the plain one                                                   */
    uint64_t cells_contested;          /* cells with 0 < c < size                                                 */
    uint64_t reads_swapped;            /* reads that left the kept set (as many joined it)                         */
    float ms_quality;                  /* device time of the pass                                                 */
} qmcp_hip_quality_stats;
int qmcp_hip_solve_quality_host(qmcp_hip_ctx* ctx,
                                const uint32_t* starts, const uint32_t* ends, const uint32_t* qualities,
                                uint64_t n_reads, const uint64_t* contig_read_offsets,
                                const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                uint64_t* keep_mask_out, qmcp_hip_stats* stats, qmcp_hip_quality_stats* qstats);
/* The same with the columns and the mask in device memory (contig tables stay on the host); ordered after `hip_stream`
 * (or NULL) as qmcp_hip_solve_device is, and returns after the pass has completed on the device. */
int qmcp_hip_solve_quality_device(qmcp_hip_ctx* ctx,
                                  const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_qualities,
                                  uint64_t n_reads, const uint64_t* contig_read_offsets,
                                  const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                  uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                  qmcp_hip_quality_stats* qstats);
/* qmcp_hip_solve_by_contig_host, then the pass on its input-order mask with the contig in the cell. */
int qmcp_hip_solve_quality_by_contig_host(qmcp_hip_ctx* ctx,
                                          const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                          const uint32_t* qualities, uint64_t n_reads,
                                          const uint32_t* contig_lengths, uint32_t n_contigs,
                                          uint32_t max_coverage, uint64_t* keep_mask_out, qmcp_hip_stats* stats,
                                          qmcp_hip_quality_stats* qstats);

/* On-target downsampling (exomes, hybrid-capture and amplicon panels): coverage is capped at max_coverage INSIDE target
 * regions only, and reads that touch no target are out of the way.  Reads, contig ids, contig_lengths / n_contigs, limits
 * and errors are those of qmcp_hip_solve_by_contig_host; qualities (one uint32 per read) may be NULL.
 * Targets: target_offsets (n_contigs + 1 entries, starting at 0, never decreasing) gives contig c the regions
 * [target_offsets[c], target_offsets[c + 1]) of target_starts / target_ends, inclusive bounds, in any order, overlapping
 * and nested regions allowed.  Every region is widened by `padding` positions on both sides and clipped to its contig
 * (a region that then begins at or beyond the contig's length is dropped); T_c is the union of contig c's regions.
 * A placed read is ON TARGET iff it covers a position of its contig's T_c, OFF TARGET otherwise (every placed read of a
 * contig without regions is).  The kept set F satisfies cov_F(p) >= min(cov(p), max_coverage) at every target position
 * p with the fewest reads possible, and is defined exactly: with rank_c(p) = |{t in T_c : t < p}|, an on-target read
 * [s, e] becomes [rank_c(s), rank_c(e + 1) - 1] on an axis of |T_c| positions, and the mask is what
 * qmcp_hip_solve_by_contig_host returns for these projected reads (input order kept, contig lengths |T_c|), expressed
 * over the input indices.  With qualities it is what qmcp_hip_solve_quality_by_contig_host returns for them: a cell is
 * the set of reads of one contig with the same PROJECTED interval (a quality range of the on-target reads above 65535
 * fails with QMCP_ERANGE).
 * Off-target reads are never kept, unless flags has QMCP_TARGETS_KEEP_OFF_TARGET: then every placed off-target read is
 * kept ("cap the targets, drop nothing else").  Unplaced reads are never kept.  No region at all is a valid call: it
 * keeps nothing, or with the flag every placed read.
 * Errors: target_offsets == NULL, offsets that do not start at 0 or that decrease, a region with start > end, null region
 * arrays with a non-zero count and unknown flag bits fail with QMCP_EINVAL on the host, before anything is copied or
 * launched: the output mask is not written.  A bad contig id (QMCP_EINVAL) or a bad read (QMCP_EREAD) is found on the
 * device among ALL reads, off-target ones included, before anything is compacted; by then the device mask
 * (d_keep_mask_out, or the context's own for the host entry) has been cleared, as qmcp_hip_solve_by_contig_* clears it
 * before it validates -- it stays all zero, and the host entry does not write keep_mask_out.  The same holds for the
 * quality range error.
 * keep_mask_out: ceil(n_reads / 64) words in INPUT order, fully overwritten; the host entry leaves it in the context for
 * qmcp_hip_kept_indices_host and qmcp_hip_complete_pairs_host.  stats (may be NULL) are those of the by-contig solve of
 * the projected reads (all zero when no read is on target); tstats (may be NULL) describe the pre- and post-pass.
 * The device entry takes the columns and the mask in device memory (the contig and target tables stay on the host), is
 * ordered after `hip_stream` (or NULL) as qmcp_hip_solve_device is, and returns after the work has completed. */
typedef struct qmcp_hip_target_stats {
    uint64_t reads_on_target, reads_off_target;  /* placed reads                     */
    uint64_t target_positions;                   /* sum of |T_c|                      */
    uint32_t regions_in, regions_merged;
    float ms_targets;                            /* project + compaction + expansion  */
} qmcp_hip_target_stats;
#define QMCP_TARGETS_KEEP_OFF_TARGET 1u
int qmcp_hip_solve_targets_host(qmcp_hip_ctx* ctx,
                                const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                const uint32_t* qualities /* may be NULL */, uint64_t n_reads,
                                const uint32_t* contig_lengths, uint32_t n_contigs,
                                const uint32_t* target_offsets, const uint32_t* target_starts,
                                const uint32_t* target_ends, uint32_t padding, uint32_t max_coverage, uint32_t flags,
                                uint64_t* keep_mask_out, qmcp_hip_stats* stats, qmcp_hip_target_stats* tstats);
int qmcp_hip_solve_targets_device(qmcp_hip_ctx* ctx,
                                  const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                  const uint32_t* d_qualities /* may be NULL */, uint64_t n_reads,
                                  const uint32_t* contig_lengths, uint32_t n_contigs,
                                  const uint32_t* target_offsets, const uint32_t* target_starts,
                                  const uint32_t* target_ends, uint32_t padding, uint32_t max_coverage, uint32_t flags,
                                  uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                  qmcp_hip_target_stats* tstats);

/* Coverage profile: a cap that varies along the genome -- 1 000 x on a hotspot panel inside a 100 x exome, 0 on decoy
 * stretches, another sample's own depth profile, "what forced reads leave uncovered".  Reads, contig ids (QMCP_NO_CONTIG
 * is never kept), contig_lengths / n_contigs, limits, read validation and "the mask is cleared before the reads are
 * validated" as in qmcp_hip_solve_by_contig_host.
 * Regions: region_offsets (n_contigs + 1 entries, starting at 0, never decreasing; NULL = no region at all) gives contig
 * c the regions [region_offsets[c], region_offsets[c + 1]) of region_starts / region_ends / region_caps, inclusive bounds,
 * in any order.  A region is clipped to its contig; one that begins at or beyond the contig's length is dropped.  After
 * clipping the regions of one contig must be disjoint (adjacent is fine).
 * Cap: cap_c(p) is the cap of the region of contig c that holds p, default_cap elsewhere.  A cap of 0 is legal: nothing is
 * required there, and a read that lies wholly in such positions is never kept.
 * Answer: the kept set F satisfies cov_F(p) >= min(cov(p), cap_c(p)) at every position with the fewest reads possible,
 * and is defined exactly: per contig, on its reads in input order, the canonical selection rule (DESIGN.md sections 2
 * and 4.2: at the leftmost position with a deficit take the unselected covering reads with the furthest end, then the
 * furthest start, then the lowest index) with need(p) = min(cov(p), cap_c(p)).  With every cap equal to M the mask is
 * bit-identical to qmcp_hip_solve_by_contig_host at M.  A call without regions -- and every batch of contigs (the
 * by-contig solve's batches) that holds no region -- IS that call at default_cap, through the unchanged solve; batches
 * with regions take the sort-based mixed-span route whatever their spans, with need built on the device
 * (k_profile_need), exact cut points only (options.cut_points is honoured, nothing is speculated) and the capped forms
 * of the register-resident walk (spans up to 448; options.mixed_sweep_in_lds = 1 and longer spans: the plain walk).
 * flags: none defined, must be 0.
 * Errors: overlapping regions (after clipping), a region with start > end, offsets that do not start at 0 or that
 * decrease, null region arrays with a non-zero count and unknown flag bits fail with QMCP_EINVAL; a cap or default_cap of
 * 2^31 or more with QMCP_ERANGE -- all on the host, before anything is copied or launched: the output mask is not
 * written.  A bad contig id (QMCP_EINVAL) or a bad read (QMCP_EREAD) is found on the device; by then the device mask has
 * been cleared (the host entry's keep_mask_out is not written).
 * stats (may be NULL): the batch-summed qmcp_hip_stats as in the by-contig solve; path == QMCP_PATH_GENERAL for batches
 * on the capped route.  pstats (may be NULL): regions_in as given, regions_used after dropping, positions_in_regions
 * after clipping; capped_positions (cov > cap) and demand (the sum of need) are reduced on the device by the kernel that
 * builds need, so they count the positions of the batches that hold a region (0 for a call without regions);
 * ms_profile is the device time of that kernel and the cut-point scan.
 * The device entry takes the columns and the mask in device memory (the contig and region tables stay on the host) and is
 * ordered after hip_stream; both entries block until the mask is complete (no _begin / _end form). */
typedef struct qmcp_hip_profile_stats {
    uint64_t positions_in_regions;
    uint64_t capped_positions;
    uint64_t demand;
    uint32_t regions_in, regions_used;
    float ms_profile;
} qmcp_hip_profile_stats;
int qmcp_hip_solve_profile_host(qmcp_hip_ctx* ctx,
                                const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids, uint64_t n_reads,
                                const uint32_t* contig_lengths, uint32_t n_contigs,
                                const uint32_t* region_offsets /* may be NULL */, const uint32_t* region_starts,
                                const uint32_t* region_ends, const uint32_t* region_caps, uint32_t default_cap,
                                uint32_t flags, uint64_t* keep_mask_out, qmcp_hip_stats* stats,
                                qmcp_hip_profile_stats* pstats);
int qmcp_hip_solve_profile_device(qmcp_hip_ctx* ctx,
                                  const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                  uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                  const uint32_t* region_offsets /* may be NULL */, const uint32_t* region_starts,
                                  const uint32_t* region_ends, const uint32_t* region_caps, uint32_t default_cap,
                                  uint32_t flags, uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                  qmcp_hip_profile_stats* pstats);

/* Depth report: what `samtools depth` / mosdepth on the input and on the output would tell, computed on the device from
 * the read columns and a keep mask and summarised per contig and per region -- nothing of the size of the genome crosses
 * the link.  Reads, contig_ids (QMCP_NO_CONTIG = unplaced), contig_lengths / n_contigs as in qmcp_hip_solve_by_contig_host,
 * in any order (nothing is grouped or sorted); at most 2^31 - 1 reads.  keep_mask: ceil(n_reads / 64) words in input order,
 * NULL = every placed read is kept; bits of unplaced reads and bits beyond n_reads are ignored.  Regions (optional:
 * target_offsets == NULL means none) in the CSR form of qmcp_hip_solve_targets_host, padded, clipped, sorted and merged in
 * the same way, so overlapping rows are fine.
 * With cov(p) the number of placed reads covering position p of a contig and kept(p) the number of those whose mask bit
 * is set, a ROW over the inclusive interval [start, end] of one contig holds the sums, the extrema, and
 *   capped_positions   positions with cov(p) > max_coverage (where downsampling had anything to remove)
 *   deficit_positions  positions with kept(p) < min(cov(p), max_coverage) -- 0 for every valid answer
 *   deficit_sum        the sum of max(0, min(cov(p), max_coverage) - kept(p))
 * Outputs, all in host memory in both entries, each may be NULL:
 *   contig_rows[n_contigs]  one row per contig, the whole contig; a contig of length 0 has positions == 0 and every other
 *                           field but `contig` 0
 *   region_rows[region_capacity], *n_region_rows_out   one row per MERGED region, contigs in id order, regions in position
 *                           order; a capacity below the merged count (which never exceeds the number of regions passed
 *                           in) fails with QMCP_EINVAL and a message naming the count needed
 *   hist_in[n_bins], hist_kept[n_bins]   the number of positions in scope with depth d, counted in bin
 *                           min(d, n_bins - 1); scope = the target positions when regions are given, every position of
 *                           every contig otherwise; n_bins in 0 .. 4096, 0 = no histograms
 *   stats                   reads_placed, reads_kept (placed and kept), scope_positions, deficit_positions (in scope),
 *                           regions_in / regions_merged, position_batches, ms_report (device time)
 * A call of more than 2^31 - 2 positions is cut at contig borders into position batches, each one pass over the reads
 * (GRCh38: two); one contig above that fails with QMCP_ERANGE.
 * Errors: null columns, a bad table, n_bins > 4096 and a capacity that is too small fail on the host before the context
 * is looked at and before anything is copied or launched; a bad contig id (QMCP_EINVAL) or a bad placed read
 * (QMCP_EREAD) is found on the device among ALL reads, and then no output buffer has been written.  A context with a
 * pending qmcp_hip_solve_device_begin is refused.  Every number is an integer sum, minimum, maximum or count: the result
 * is deterministic.  The context's own keep mask is left as it is. */
typedef struct qmcp_hip_depth_row {
    uint32_t contig, start, end;                  /* the interval, inclusive                               */
    uint32_t min_in, max_in, min_kept, max_kept;  /* over the interval                                     */
    uint32_t reserved;                            /* 0                                                     */
    uint64_t positions;                           /* end - start + 1                                       */
    uint64_t sum_in, sum_kept;                    /* sums of cov(p) and kept(p)                            */
    uint64_t capped_positions, deficit_positions, deficit_sum;
} qmcp_hip_depth_row;
typedef struct qmcp_hip_depth_stats {
    uint64_t reads_placed, reads_kept;
    uint64_t scope_positions, deficit_positions;
    uint32_t regions_in, regions_merged, position_batches;
    float ms_report;                              /* HIP events on the context's stream                    */
} qmcp_hip_depth_stats;
int qmcp_hip_depth_report_host(qmcp_hip_ctx* ctx,
                               const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                               uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                               const uint64_t* keep_mask /* may be NULL */, uint32_t max_coverage,
                               const uint32_t* target_offsets /* may be NULL */, const uint32_t* target_starts,
                               const uint32_t* target_ends, uint32_t padding, uint32_t n_bins,
                               qmcp_hip_depth_row* contig_rows, qmcp_hip_depth_row* region_rows,
                               uint64_t region_capacity, uint64_t* n_region_rows_out, uint64_t* hist_in,
                               uint64_t* hist_kept, qmcp_hip_depth_stats* stats);
/* The same with the three columns and the mask in device memory (the tables stay on the host, the outputs go to host
 * memory); ordered after `hip_stream` (or NULL) as qmcp_hip_solve_by_contig_device is, and returns when the outputs are in
 * host memory. */
int qmcp_hip_depth_report_device(qmcp_hip_ctx* ctx,
                                 const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                 uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                 const uint64_t* d_keep_mask /* may be NULL */, uint32_t max_coverage,
                                 const uint32_t* target_offsets /* may be NULL */, const uint32_t* target_starts,
                                 const uint32_t* target_ends, uint32_t padding, uint32_t n_bins,
                                 qmcp_hip_depth_row* contig_rows, qmcp_hip_depth_row* region_rows,
                                 uint64_t region_capacity, uint64_t* n_region_rows_out, uint64_t* hist_in,
                                 uint64_t* hist_kept, void* hip_stream, qmcp_hip_depth_stats* stats);

/* Depth track: the per-base form of the depth report -- what `bedtools genomecov -bg` / mosdepth's per-base file on the
 * input and on the output would hold, as runs of equal depth.  Reads, contig_ids, contig_lengths / n_contigs, keep_mask,
 * max_coverage, the optional regions with `padding`, the limits and the position batches are those of
 * qmcp_hip_depth_report_host, and cov(p) / kept(p) are defined there.  The SCOPE is every position of every contig or,
 * when regions are given, every position inside a merged region.  `flags` chooses what a run is:
 *   QMCP_TRACK_IN          depth_in = min(cov, depth_cap) takes part in the run tuple (depth_cap == 0: no clamp)
 *   QMCP_TRACK_KEPT        depth_kept = min(kept, depth_cap) takes part
 *   QMCP_TRACK_SHORT_ONLY  only positions with kept < min(cov, max_coverage) are emitted (on the unclamped values)
 *   QMCP_TRACK_SKIP_ZERO   positions whose selected channels are all 0 are not emitted (genomecov -bg's behaviour)
 * At least one of IN and KEPT must be set; anything else, or an unknown bit, is QMCP_EINVAL before the context is looked
 * at.  A channel that is not selected is reported as 0 and is not compared.  The tuple of a position is (depth_in,
 * depth_kept, short) with short = [kept < min(cov, max_coverage)].  A RUN is a maximal interval [start, end] of
 * consecutive emitted positions with one tuple; it lies in one contig and, with regions, in one merged region.  Runs come
 * back in ascending (contig, start) order: the result is unique and deterministic.
 * Outputs, all in host memory in both entries:
 *   runs[run_capacity], *n_runs_out   the records; runs == NULL counts only.  When runs is given and the total exceeds
 *                           run_capacity the call returns QMCP_ERANGE with *n_runs_out set to the total, and runs and
 *                           stats untouched
 *   stats                   n_runs, positions_in_runs (emitted positions), scope_positions, short_positions (ALL short
 *                           positions in scope, whatever the flags say: the report's deficit_positions), reads_placed,
 *                           reads_kept, regions_in / regions_merged, position_batches, ms_track (device time)
 * Invariant: n_runs <= min(positions_in_runs, 2 * reads_placed + n_contigs + regions_merged) -- every change of any
 * channel sits at some read's start or end + 1, every other run begins at the start of a contig or merged region.
 * Errors: the report's, in its order -- null columns, a bad table and a contig above one position batch on the host
 * before the context is looked at; a bad contig id (QMCP_EINVAL) or a bad placed read (QMCP_EREAD) found on the device
 * among ALL reads; the capacity last.  The caller's buffers are written only after all of them. */
#define QMCP_TRACK_IN 1u
#define QMCP_TRACK_KEPT 2u
#define QMCP_TRACK_SHORT_ONLY 4u
#define QMCP_TRACK_SKIP_ZERO 8u
typedef struct qmcp_hip_track_run {
    uint32_t contig, start, end;                  /* the run, inclusive, in the contig's coordinates       */
    uint32_t depth_in, depth_kept;                /* clamped; 0 for a channel that is not selected         */
    uint32_t flags;                               /* bit 0: short                                          */
} qmcp_hip_track_run;
typedef struct qmcp_hip_track_stats {
    uint64_t n_runs, positions_in_runs, scope_positions, short_positions, reads_placed, reads_kept;
    uint32_t regions_in, regions_merged, position_batches;
    float ms_track;                               /* HIP events on the context's stream                    */
} qmcp_hip_track_stats;
int qmcp_hip_depth_track_host(qmcp_hip_ctx* ctx,
                              const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                              uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                              const uint64_t* keep_mask /* may be NULL */, uint32_t max_coverage,
                              const uint32_t* target_offsets /* may be NULL */, const uint32_t* target_starts,
                              const uint32_t* target_ends, uint32_t padding, uint32_t flags, uint32_t depth_cap,
                              qmcp_hip_track_run* runs /* may be NULL */, uint64_t run_capacity,
                              uint64_t* n_runs_out, qmcp_hip_track_stats* stats);
/* The same with the three columns and the mask in device memory, ordered after `hip_stream` as
 * qmcp_hip_depth_report_device is; returns when the outputs are in host memory. */
int qmcp_hip_depth_track_device(qmcp_hip_ctx* ctx,
                                const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                const uint64_t* d_keep_mask /* may be NULL */, uint32_t max_coverage,
                                const uint32_t* target_offsets /* may be NULL */, const uint32_t* target_starts,
                                const uint32_t* target_ends, uint32_t padding, uint32_t flags, uint32_t depth_cap,
                                qmcp_hip_track_run* runs /* may be NULL */, uint64_t run_capacity,
                                uint64_t* n_runs_out, void* hip_stream, qmcp_hip_track_stats* stats);

/* Coverage ladder: the same reads at several falling coverages in one call -- a titration (100x, 50x, 30x, 10x of one
 * sample).  Reads, contig_ids, contig_lengths / n_contigs and limits are those of qmcp_hip_solve_by_contig_host.
 * coverages[0] > coverages[1] > ... > coverages[n_levels - 1] >= 1, 1 <= n_levels <= QMCP_LADDER_MAX_LEVELS.
 * Definition: K_0 is the mask qmcp_hip_solve_by_contig_host returns for the call at coverages[0]; K_j is the mask it
 * returns at coverages[j] for the reads of K_(j-1) ALONE, in input order with their contig ids, expressed over the input
 * indices.  So K_0 >= K_1 >= ... (the levels are nested), and every K_j is valid for the ORIGINAL reads:
 * cov_Kj(p) >= min(cov_K(j-1)(p), coverages[j]) >= min(cov(p), coverages[j]) because coverages[j] < coverages[j - 1].
 * Output: one byte per read, levels[i] = the number of levels that keep read i (0 .. n_levels), K_j = {i : levels[i] > j};
 * unplaced reads get 0.  levels_out: n_reads bytes in INPUT order, fully overwritten.
 * How: the reads are grouped by contig once; inside each batch the first level is the plain solve, and every further
 * level is a stable compaction of the kept reads (with their input indices) and a solve of the compacted columns.
 * Errors: n_levels == 0 or > QMCP_LADDER_MAX_LEVELS, coverages == NULL, a coverage of 0 and a list that does not fall
 * strictly fail with QMCP_EINVAL on the host, before the context is looked at and before anything is copied or launched:
 * levels_out is not written.  A bad contig id (QMCP_EINVAL) or a bad read (QMCP_EREAD) is found on the device as in
 * qmcp_hip_solve_by_contig_host; by then the device bytes (d_levels_out, or the context's own for the host entry) have
 * been cleared -- they stay all zero, and the host entry does not write levels_out.
 * stats (may be NULL) are those of level 0: they equal the plain by-contig call at coverages[0].  lstats (may be NULL):
 * the levels.  The host entry leaves K_0 in the context, for qmcp_hip_kept_indices_host and qmcp_hip_complete_pairs_host.
 * The device entry takes the three columns and the bytes in device memory (contig_lengths and coverages stay on the
 * host), is ordered after `hip_stream` (or NULL) as qmcp_hip_solve_device is, and returns after the work has completed. */
#define QMCP_LADDER_MAX_LEVELS 16
typedef struct qmcp_hip_ladder_stats {
    uint32_t n_levels, reserved;
    uint64_t n_kept[QMCP_LADDER_MAX_LEVELS];   /* |K_j|                                                               */
    float ms_level[QMCP_LADDER_MAX_LEVELS];    /* device time per level, level 0 = the plain solve                    */
    float ms_ladder;                           /* everything the ladder adds around the solves: level bytes, popcounts,
                                                  scans, offsets, compactions                                         */
} qmcp_hip_ladder_stats;
int qmcp_hip_solve_ladder_host(qmcp_hip_ctx* ctx,
                               const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                               uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                               const uint32_t* coverages, uint32_t n_levels, uint8_t* levels_out,
                               qmcp_hip_stats* stats, qmcp_hip_ladder_stats* lstats);
int qmcp_hip_solve_ladder_device(qmcp_hip_ctx* ctx,
                                 const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                 uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                 const uint32_t* coverages, uint32_t n_levels, uint8_t* d_levels_out,
                                 void* hip_stream, qmcp_hip_stats* stats, qmcp_hip_ladder_stats* lstats);

/* Disjoint replicates: one read set split into several INDEPENDENT downsamples in one call -- pseudo-replicates at 30x, a
 * 30x "truth" subset beside a disjoint 10x "test" subset.  Reads, contig_ids, contig_lengths / n_contigs and limits are
 * those of qmcp_hip_solve_by_contig_host.  coverages[0 .. n_replicates - 1], each in 1 .. 2^31 - 1, in any order, equal
 * values allowed; 1 <= n_replicates <= QMCP_REPLICATES_MAX.
 * Definition: R_1 is the mask qmcp_hip_solve_by_contig_host returns at coverages[0]; R_r (r > 1) is the mask it returns
 * at coverages[r - 1] for the placed reads that lie in none of R_1 .. R_(r-1), ALONE, in input order with their contig
 * ids, expressed over the input indices.  Output: one byte per read, labels[i] = r if i is in R_r, 0 otherwise (unplaced
 * reads get 0); n_reads bytes in INPUT order, fully overwritten.
 * The replicates are disjoint, R_r has minimum cardinality on the reads that were left when it was solved, and at every
 * position cov_Rr(p) >= min(cov(p) - sum_{j<r} cov_Rj(p), coverages[r - 1]).  A replicate that finds no read left is
 * empty, and so is every later one; that is no error.
 * QMCP_REPLICATES_WHOLE_PAIRS: reads (2q, 2q + 1) are pair q (an odd n_reads is QMCP_EINVAL).  After replicate r's solve
 * a placed read whose placed mate is in R_r joins R_r (it is still free: pairs move together; an unplaced mate never
 * joins).  The coverage guarantee still holds -- a replicate only grows --, disjointness holds pair-wise, minimum
 * cardinality is no longer claimed.
 * QMCP_REPLICATES_SHORTFALL: per replicate, short_positions counts the positions where the replicate's depth (mates
 * included) is below min(cov(p), coverages[r - 1]), cov the depth of ALL placed reads, short_bases sums the differences,
 * and n_full is the number of leading replicates without a short position.  Computed on the device by the depth
 * report's kernels over the packed mask of labels == r; without the flag the fields are 0.
 * How: the reads are grouped by contig once per call; a call of one batch keeps the batch's gathered columns and
 * compacts the reads that are still free from replicate to replicate between two sets of columns; a call of several
 * batches walks replicate-major over them and gathers each batch's free reads from the grouping.
 * Errors: NULL coverages, n_replicates outside 1 .. QMCP_REPLICATES_MAX, a coverage of 0, unknown flag bits and an odd
 * n_reads under QMCP_REPLICATES_WHOLE_PAIRS are QMCP_EINVAL, a coverage of 2^31 or more is QMCP_ERANGE: on the host,
 * before the context is looked at and before anything is copied or launched; labels_out is not written.  A bad contig
 * id (QMCP_EINVAL) or a bad read (QMCP_EREAD) is found on the device as in qmcp_hip_solve_by_contig_host; by then the
 * device bytes have been cleared -- they stay all zero, and the host entry does not write labels_out.
 * stats (may be NULL) are replicate 1's solve: they equal the plain by-contig call at coverages[0].  rep_stats (may be
 * NULL; n_replicates entries): the batch-summed stats of each replicate's solves.  rstats (may be NULL): the replicates.
 * The host entry leaves R_1 in the context.  The device entry takes the three columns and the bytes in device memory,
 * is ordered after `hip_stream` (or NULL) as qmcp_hip_solve_device is, and returns after the work has completed. */
#define QMCP_REPLICATES_MAX 16
#define QMCP_REPLICATES_WHOLE_PAIRS 1u
#define QMCP_REPLICATES_SHORTFALL 2u
typedef struct qmcp_hip_replicates_stats {
    uint32_t n_replicates, flags;
    uint32_t n_full, reserved;                        /* leading replicates without a short position (SHORTFALL)     */
    uint64_t n_offered[QMCP_REPLICATES_MAX];          /* reads left when the replicate began                         */
    uint64_t n_kept[QMCP_REPLICATES_MAX];             /* |R_r|, mates included                                       */
    uint64_t n_mates[QMCP_REPLICATES_MAX];            /* reads that joined only as mates (WHOLE_PAIRS)               */
    uint64_t short_positions[QMCP_REPLICATES_MAX];    /* SHORTFALL                                                   */
    uint64_t short_bases[QMCP_REPLICATES_MAX];        /* SHORTFALL                                                   */
    float ms_replicate[QMCP_REPLICATES_MAX];          /* device time of the replicate's solves                       */
    float ms_split;                                   /* everything the call adds around the solves                  */
    float reserved1;
} qmcp_hip_replicates_stats;
int qmcp_hip_solve_replicates_host(qmcp_hip_ctx* ctx,
                                   const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                   uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                   const uint32_t* coverages, uint32_t n_replicates, uint32_t flags,
                                   uint8_t* labels_out, qmcp_hip_stats* stats,
                                   qmcp_hip_stats* rep_stats /* n_replicates entries, or NULL */,
                                   qmcp_hip_replicates_stats* rstats);
int qmcp_hip_solve_replicates_device(qmcp_hip_ctx* ctx,
                                     const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                     uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                     const uint32_t* coverages, uint32_t n_replicates, uint32_t flags,
                                     uint8_t* d_labels_out, void* hip_stream, qmcp_hip_stats* stats,
                                     qmcp_hip_stats* rep_stats /* n_replicates entries, or NULL */,
                                     qmcp_hip_replicates_stats* rstats);

/* Stratified downsampling: one coverage cap per stratum -- strand, read group, sample, lane, haplotype, anything the
 * caller can turn into a small integer per read ("bring every sample of a pooled file to 30x"; "half of the coverage
 * from each strand").  Reads, contig_ids, contig_lengths / n_contigs and the per-read rules are those of
 * qmcp_hip_solve_by_contig_host.  strata[i] < n_strata names read i's stratum, QMCP_NO_STRATUM marks a read that belongs
 * to none: it is never kept, exactly like a QMCP_NO_CONTIG read, and is still validated against its contig.
 * max_coverages[s] is stratum s's cap, 1 <= n_strata <= 65536, n_strata * n_contigs <= 2^24.
 * Definition: the mask is the OR over the strata s of the mask qmcp_hip_solve_by_contig_host returns, at
 * M = max_coverages[s], for the placed reads with strata[i] == s ALONE, in input order, expressed over the input indices.
 * A stratum whose cap is 0 keeps nothing (no solve is run for it).  With n_strata == 1 and every placed read in stratum 0
 * the mask and stats.n_kept are bit-identical to qmcp_hip_solve_by_contig_host at that M.
 * Guarantee: for every stratum s, contig c and position p, the kept reads OF STRATUM s cover p at least
 * min(coverage of p by stratum s, max_coverages[s]) times.  Nothing is promised about the total over the strata: a
 * stratum with little data is NOT topped up from another, and the total at p may be anything between the largest
 * floor and the sum of the caps.
 * How: the reads are grouped once, on the device, by the key stratum * n_contigs + contig; every stratum with a cap and
 * reads is cut into solver calls of its own (never across a stratum boundary), each gathered, solved at the stratum's cap
 * and scattered back; a last pass over the grouped records fills the rows.  One (stratum, contig) must fit one solver
 * call (2^30 reads, 2^31 - 2 positions): QMCP_ERANGE with a message naming the pair otherwise.
 * rows_out (host memory in both entries, n_strata rows, may be NULL): per stratum its placed reads, how many of them are
 * kept, and the bases (end - start + 1) of both; mean depth = bases / sum of the contig lengths.  Written on success only.
 * stats (may be NULL) follow the by-contig convention: the solver calls summed, the route of the largest; n_reads is the
 * number of placed reads = the sum of the rows' n_reads, n_kept the sum of the rows' n_kept.
 * Errors: NULL buffers, max_coverages == NULL and n_strata == 0 fail with QMCP_EINVAL, n_strata > 65536 and
 * n_strata * n_contigs > 2^24 with QMCP_ERANGE, all on the host before anything is copied or launched.  A stratum id that
 * is neither < n_strata nor QMCP_NO_STRATUM (QMCP_EINVAL), a bad contig id (QMCP_EINVAL) and a bad read (QMCP_EREAD) are
 * found on the device; by then the device mask (d_keep_mask_out, or the context's own for the host entry) has been
 * cleared -- ceil(n_reads / 64) words and nothing beyond them -- and the host entry does not write keep_mask_out.
 * The device entry takes the four columns and the mask in device memory (contig_lengths, max_coverages and rows_out stay
 * on the host), is ordered after `hip_stream` (or NULL) as qmcp_hip_solve_device is, and returns after the work has
 * completed.  The host entry leaves the mask in the context, for qmcp_hip_kept_indices_host. */
#define QMCP_NO_STRATUM 0xFFFFFFFFu
typedef struct qmcp_hip_stratum_row {   /* 32 bytes */
    uint64_t n_reads;     /* placed reads of the stratum                                                               */
    uint64_t n_kept;      /* ... of which the mask keeps                                                               */
    uint64_t bases_in;    /* sum of (end - start + 1) over n_reads                                                     */
    uint64_t bases_kept;  /* ... over the kept ones                                                                    */
} qmcp_hip_stratum_row;
int qmcp_hip_solve_stratified_host(qmcp_hip_ctx* ctx,
                                   const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                   const uint32_t* strata, uint64_t n_reads,
                                   const uint32_t* contig_lengths, uint32_t n_contigs,
                                   const uint32_t* max_coverages, uint32_t n_strata,
                                   uint64_t* keep_mask_out, qmcp_hip_stratum_row* rows_out, qmcp_hip_stats* stats);
int qmcp_hip_solve_stratified_device(qmcp_hip_ctx* ctx,
                                     const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                     const uint32_t* d_strata, uint64_t n_reads,
                                     const uint32_t* contig_lengths, uint32_t n_contigs,
                                     const uint32_t* max_coverages, uint32_t n_strata,
                                     uint64_t* d_keep_mask_out, qmcp_hip_stratum_row* rows_out, void* hip_stream,
                                     qmcp_hip_stats* stats);

/* Tiered downsampling: the best reads first, worse reads only where the better ones cannot bring the depth to
 * min(coverage, M).  The tier is any small integer per read (a MAPQ band, primary before supplementary, non-duplicates
 * before duplicates, run A before run B, properly paired before orphans), 0 the best.  Reads, contig_ids, contig_lengths
 * / n_contigs, the per-read rules and the limits are those of qmcp_hip_solve_by_contig_host.  tiers[i] < n_tiers names
 * read i's tier, QMCP_NO_TIER marks a read that is never kept; it is still validated against its contig, like a
 * QMCP_NO_STRATUM read.  1 <= n_tiers <= QMCP_TIERS_MAX, n_tiers * n_contigs <= 2^24.
 * Definition: S_(-1) is empty.  For t = 0 .. n_tiers - 1:
 *   R_t        the placed reads of tier t, alone, in input order
 *   credit_t   credit_t(p) = the depth of S_(t-1) at p
 *   need_t     need_t(p) = min(cov_(R_t)(p), max(0, M - credit_t(p)))
 *   K_t        the canonical selection of qmcp_hip_solve_profile_host over R_t under need_t -- per contig: the leftmost
 *              deficit first, then the furthest end, the furthest start, the lowest index
 *   S_t        S_(t-1) | K_t
 * The result is S_(n_tiers - 1), a mask in input order.  No tier is kept whole: every tier, the first included, is
 * downsampled.  There is no pair completion inside the entry.
 * Guarantees:
 *   1. the kept depth is >= min(cov_all(p), M) at every position p.  (By induction depth(S_t) >= min(cov_(tiers <= t),
 *      M): where credit < M, credit + min(cov_t, M - credit) = min(credit + cov_t, M).)
 *   2. tier 0 restricted to itself is qmcp_hip_solve_by_contig_* of R_0 at M bit for bit, taken on that call's own
 *      routes (every fast route stays in use): n_tiers == 1 with every placed read in tier 0 gives the by-contig mask
 *      and stats.n_kept bit for bit.
 *   3. a read of tier t is kept only through need_t: where S_(t-1) already reaches M on the whole support of tier t,
 *      the tier keeps nothing and no sweep is queued for it.
 *   4. the first tier that has reads on a contig is solved there with zero credit: its selection on that contig equals
 *      the by-contig solve of those reads.
 * Not claimed: minimum cardinality of the whole result, or the optimum of the reference's min-cost objective.
 * How: the reads are grouped once, on the device, by the key tier * n_contigs + contig; every tier with reads is cut
 * into solver calls of its own (never across a tier; one (tier, contig) must fit one call: 2^30 reads, 2^31 - 2
 * positions, QMCP_ERANGE naming the pair otherwise).  Tier 0's calls are the plain solve at M.  After a call of any
 * tier its kept reads are compacted into a kept list of (contig, start, end) entries, while a later tier has reads; a
 * call of tier t >= 1 turns the list's entries on its contigs into credit (events on a zeroed axis, scanned), builds
 * need_t on the device and takes the sort-based mixed-span route of the profile entries under it, exact cut points
 * only (options.cut_points is honoured, nothing is speculated).  Known cost: a later tier with real demand on deep data
 * is one serial chain per contig, as for the ceiling and proportional entries.
 * rows_out (host memory in both entries, n_tiers rows, may be NULL; written on success only), one row per tier:
 * the stratified row's four counts; demand (the sum of need_t), asked_positions (need_t > 0) and capped_positions
 * (cov_(R_t) > max(0, M - credit_t)), all three 0 for tier 0, whose plain solves build no need; sweeps (tier 0: its
 * solver calls; later tiers: the calls that queued a sweep -- a call whose demand is 0 queues none); ms_stage (the
 * device time of the tier's solver calls).  max_coverage == 0 keeps nothing: no solver call is made, and every field
 * behind the four counts is 0.
 * tstats (may be NULL): n_tiers, tiers_used (tiers that kept a read), reads_untiered (reads with QMCP_NO_TIER, placed
 * or not), ms_tiers (the call's device time outside the solver calls: grouping, gathers, kept lists, credit, rows).
 * stats (may be NULL) are tier 0's solver calls, as stats are stage 1's in the pair entry: summed, the route of the
 * largest; n_contigs and total_length are the call's.
 * Errors: NULL buffers, tiers == NULL (also without reads) and n_tiers == 0 fail with QMCP_EINVAL, n_tiers >
 * QMCP_TIERS_MAX, n_tiers * n_contigs > 2^24 and max_coverage >= 2^31 with QMCP_ERANGE, all on the host before anything is copied or launched.
 * A tier id that is neither < n_tiers nor QMCP_NO_TIER (QMCP_EINVAL), a bad contig id (QMCP_EINVAL) and a bad read
 * (QMCP_EREAD) are found on the device; by then the device mask (d_keep_mask_out, or the context's own for the host
 * entry) has been cleared -- ceil(n_reads / 64) words and nothing beyond them -- and the host entry does not write
 * keep_mask_out.  The device entry takes the four columns and the mask in device memory (contig_lengths and rows_out
 * stay on the host), is ordered after `hip_stream` (or NULL) as qmcp_hip_solve_device is, and returns after the work
 * has completed.  The host entry leaves the mask in the context, for qmcp_hip_kept_indices_host. */
#define QMCP_NO_TIER 0xFFFFFFFFu
#define QMCP_TIERS_MAX 16
typedef struct qmcp_hip_tier_row {   /* 64 bytes */
    uint64_t n_reads;           /* placed reads of the tier                                                            */
    uint64_t n_kept;            /* ... of which the mask keeps                                                         */
    uint64_t bases_in;          /* sum of (end - start + 1) over n_reads                                               */
    uint64_t bases_kept;        /* ... over the kept ones                                                              */
    uint64_t demand;            /* sum of need_t over the positions (0 for tier 0)                                     */
    uint64_t asked_positions;   /* positions with need_t > 0 (0 for tier 0)                                            */
    uint64_t capped_positions;  /* positions where the tier's coverage exceeds max(0, M - credit_t) (0 for tier 0)    */
    uint32_t sweeps;            /* tier 0: solver calls; later tiers: solver calls that queued a sweep                 */
    float ms_stage;             /* device time of the tier's solver calls                                              */
} qmcp_hip_tier_row;
typedef struct qmcp_hip_tiers_stats {   /* 24 bytes */
    uint32_t n_tiers;
    uint32_t tiers_used;       /* tiers that kept at least one read                                                    */
    uint64_t reads_untiered;   /* reads whose tier is QMCP_NO_TIER                                                     */
    float ms_tiers;            /* the call's device time outside the solver calls                                      */
    uint32_t reserved;         /* 0                                                                                    */
} qmcp_hip_tiers_stats;
int qmcp_hip_solve_tiers_host(qmcp_hip_ctx* ctx,
                              const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                              const uint32_t* tiers, uint64_t n_reads,
                              const uint32_t* contig_lengths, uint32_t n_contigs,
                              uint32_t max_coverage, uint32_t n_tiers,
                              uint64_t* keep_mask_out, qmcp_hip_tier_row* rows_out, qmcp_hip_stats* stats,
                              qmcp_hip_tiers_stats* tstats);
int qmcp_hip_solve_tiers_device(qmcp_hip_ctx* ctx,
                                const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                const uint32_t* d_tiers, uint64_t n_reads,
                                const uint32_t* contig_lengths, uint32_t n_contigs,
                                uint32_t max_coverage, uint32_t n_tiers,
                                uint64_t* d_keep_mask_out, qmcp_hip_tier_row* rows_out, void* hip_stream,
                                qmcp_hip_stats* stats, qmcp_hip_tiers_stats* tstats);

/* Duplicate-aware downsampling: duplicate families are collapsed to one representative each BEFORE the solve, so that a
 * PCR or optical duplicate does not count towards min(coverage, M) like an independent read.  starts, ends, contig_ids,
 * n_reads, contig_lengths / n_contigs, max_coverage, keep_mask_out, stats, limits and errors are those of
 * qmcp_hip_solve_by_contig_host / _device.  In addition:
 *   tags        one uint32 per read, any value (strand, a library id, a UMI hash); NULL: every tag is 0.
 *   qualities   one uint32 per read; NULL: every quality is 0.  A range (max - min over the placed reads) above 65535
 *               fails with QMCP_ERANGE before anything is written, as in the quality entries.
 *   flags       QMCP_DEDUP_PAIRS selects pair mode, QMCP_DEDUP_COMPLETE_PAIRS asks for mate completion.  Either with an
 *               odd n_reads, COMPLETE_PAIRS without PAIRS, and unknown bits fail with QMCP_EINVAL.
 *   dup_mask_out  may be NULL; ceil(n_reads / 64) words, fully overwritten.
 *   hist_out, hist_bins  may be NULL / 0; hist_bins uint64 words in host memory (both entries), at most 4096 bins
 *               (QMCP_ERANGE beyond).
 *   dstats      may be NULL.
 * CELL: the cell of a placed read is (contig, start, end, tag).  All QMCP_NO_CONTIG reads share one extra cell U.
 * READ MODE (default): the unit is a placed read and a family is a cell.  A unit's score is its quality; the
 * representative of a family is the unit of highest score, then of lowest index.  Unplaced reads are in no family.
 * PAIR MODE: unit q is the reads (2q, 2q + 1), eligible iff at least one mate is placed.  Its signature is the UNORDERED
 * pair {cell(2q), cell(2q + 1)} (mates on different contigs are fine), a family is the set of eligible units with equal
 * signature, a unit's score is the sum of the qualities of its placed mates, the representative is the unit of highest
 * score, then of lowest q.  A pair with both mates unplaced is in no family.
 * RESULT: the survivors are the reads of all representatives (in pair mode an unplaced mate of a representative
 * included).  keep_mask_out is the mask qmcp_hip_solve_by_contig_host returns for the survivors in input order, mapped
 * back to input positions; every other bit is clear.  With COMPLETE_PAIRS the OR inside each aligned bit pair is applied
 * afterwards: it can only add the mate of a kept survivor, a survivor itself.  Bit i of dup_mask_out is set iff read i
 * belongs to a unit that is in a family and is not its representative (in pair mode both mates get the bit, an unplaced
 * one too), so keep & dup == 0 always.  hist_out[k - 1] is the number of families of size k for k < hist_bins, the last
 * bin holds the sizes >= hist_bins.  When no two units share a cell / signature, the mask is that of
 * qmcp_hip_solve_by_contig_host bit for bit.
 * VALIDATION: every read is validated as the by-contig entries do -- the reads of duplicates too -- before anything is
 * written: a bad contig id gives QMCP_EINVAL, a bad read QMCP_EREAD, and no output buffer has been touched.
 * HOW: one pass validates and takes the ranges of tag, quality and span; the widths of the key gstart | span - min_span |
 * tag - tag_min | q_max - q come from those ranges (tags == NULL and one span cost nothing); the stable LSD radix sorts
 * {key, index} as 32-bit records, as split 64-bit keys, or -- beyond 64 bits -- field by field, least significant first.
 * A family then is a run of the sorted order with its representative first.  Pair mode sorts the reads by cell first
 * (dense cell ids), then the units by min id | max id | score_max - score.  Survivor and duplicate bits, the histogram
 * and the counters are made on the device; the survivors are compacted in input order, solved, and the mask expanded.
 * stats (may be NULL) are the inner solve's: n_reads counts the placed survivors.
 * The pass is blocking (no _begin / _end form).  The device entry takes the columns and both masks in device memory
 * (contig_lengths, hist_out and the stats stay on the host), columns at any 4-byte alignment, and is ordered after
 * `hip_stream` (or NULL) as qmcp_hip_solve_device is.  The host entry leaves the keep mask in the context. */
#define QMCP_DEDUP_PAIRS 1u
#define QMCP_DEDUP_COMPLETE_PAIRS 2u
typedef struct qmcp_hip_dedup_stats {
    uint64_t units;            /* placed reads (read mode), pairs with a placed mate (pair mode)                      */
    uint64_t families;         /* distinct cells / signatures among the units                                         */
    uint64_t duplicate_units;  /* units - families                                                                    */
    uint64_t largest_family;   /* units of the largest family                                                         */
    uint64_t reads_survived;   /* reads handed to the inner solve                                                     */
    uint32_t key_bits;         /* width of the key the units were sorted by                                           */
    uint32_t sort_passes;      /* 8-bit LSD passes, both sorts of pair mode together                                  */
    float ms_dedup;            /* device time of everything except the inner solve                                    */
} qmcp_hip_dedup_stats;
int qmcp_hip_solve_dedup_host(qmcp_hip_ctx* ctx,
                              const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                              const uint32_t* tags, const uint32_t* qualities, uint64_t n_reads,
                              const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage, uint32_t flags,
                              uint64_t* keep_mask_out, uint64_t* dup_mask_out, uint64_t* hist_out, uint32_t hist_bins,
                              qmcp_hip_stats* stats, qmcp_hip_dedup_stats* dstats);
int qmcp_hip_solve_dedup_device(qmcp_hip_ctx* ctx,
                                const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                const uint32_t* d_tags, const uint32_t* d_qualities, uint64_t n_reads,
                                const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                uint32_t flags, uint64_t* d_keep_mask_out, uint64_t* d_dup_mask_out, uint64_t* hist_out,
                                uint32_t hist_bins, void* hip_stream, qmcp_hip_stats* stats,
                                qmcp_hip_dedup_stats* dstats);

/* Pair-aware downsampling: a staged solve that credits the mates' coverage.  Paired-end data solved read by read and
 * then completed pair by pair keeps almost twice what was asked for: the solve returns a minimum set for min(cov, M) and
 * never learns that a mate comes along with nearly every read it keeps.  Here the solve sees the mates: it solves for a
 * part of the target, completes the pairs, and tops up only what is still missing.
 * Input: reads, contig_ids (QMCP_NO_CONTIG = unplaced), contig_lengths / n_contigs and limits as in
 * qmcp_hip_solve_by_contig_host, with n_reads even and pair q = reads (2q, 2q + 1).  stages: targets T_1 < T_2 < ... <
 * T_k = max_coverage, 1 <= k <= QMCP_PAIR_MAX_STAGES, T_1 >= 1; stages == NULL (n_stages ignored) is the default
 * {ceil(M / 2), M}, which is {1} for M = 1.
 * Stages: S_0 is empty.  For stage j, credit_j(p) is the depth of the placed reads of S_(j-1) at p and cap_j(p) =
 * max(0, T_j - credit_j(p)); K_j is the canonical selection of qmcp_hip_solve_profile_host -- per contig, leftmost deficit
 * first, then furthest end, furthest start, lowest index -- taken over the placed reads NOT in S_(j-1), alone, in input
 * order, with need(p) = min(cov_rest(p), cap_j(p)); S_j = complete_pairs(S_(j-1) | K_j).  The result is S_k, a keep mask
 * in INPUT order that holds whole pairs.
 * An unplaced read is never a candidate and gives no credit: it enters only as the mate of a kept read.  Mates on
 * different contigs are fine.
 * Why S_k is valid: with cov = credit + cov_rest, min(cov_rest, max(0, T - credit)) = max(0, min(cov, T) - credit)
 * (check cov >= T and cov < T), so after stage j the depth of S_j is at least min(cov, T_j) everywhere; completion only
 * adds reads; at j = k this is the plain solve's invariant at max_coverage.
 * Stage 1 has no credit: it IS qmcp_hip_solve_by_contig_* at T_1, with every route that call takes, so k = 1 is bit for
 * bit that call at max_coverage followed by qmcp_hip_complete_pairs_*.  Later stages take the capped mixed-span route of
 * the coverage profile.
 * Not claimed: that S_k is minimum among whole-pair solutions, or that more stages are always better.  The result is
 * defined by the stages, as the ladder's is by its chain.
 * Errors, all on the host before the context is looked at and before anything is copied or launched: an odd n_reads
 * and a bad stage list (a count outside 1 .. QMCP_PAIR_MAX_STAGES, a target of 0, a list that does not rise strictly, a
 * last target that is not max_coverage, max_coverage 0) fail with QMCP_EINVAL and a message naming the entry; a target
 * or max_coverage of 2^31 or more with QMCP_ERANGE.  Bad ids and reads as in qmcp_hip_solve_by_contig_host.
 * stats (may be NULL) are stage 1's; pstats (may be NULL): the stages.  The host entry leaves S_k in the context, for
 * qmcp_hip_kept_indices_host.  The device entry takes the three columns and the mask in device memory (contig_lengths
 * and stages stay on the host), is ordered after `hip_stream` (or NULL) as qmcp_hip_solve_device is, and returns after
 * the work has completed. */
#define QMCP_PAIR_MAX_STAGES 16
typedef struct qmcp_hip_pair_stats {
    uint32_t n_stages, reserved;
    uint64_t n_selected[QMCP_PAIR_MAX_STAGES];        /* |K_j|                                                         */
    uint64_t n_kept[QMCP_PAIR_MAX_STAGES];            /* |S_j|, after completion                                       */
    uint64_t capped_positions[QMCP_PAIR_MAX_STAGES];  /* stages after the first: positions with cov_rest > cap_j ...   */
    uint64_t demand[QMCP_PAIR_MAX_STAGES];            /* ... and the sum of need over the batches that had candidates  */
    uint32_t target[QMCP_PAIR_MAX_STAGES];            /* T_j                                                           */
    uint32_t sweeps[QMCP_PAIR_MAX_STAGES];            /* capped sweeps queued (one per batch that asked for a read;
                                                         0 for stage 1, the plain solve)                               */
    float ms_stage[QMCP_PAIR_MAX_STAGES];             /* device time of the stage's solves                             */
    float ms_pairs;                                   /* everything the feature adds around the solves: mask gather,
                                                         compaction, credit, need, mask expansion, completion, counts  */
    uint32_t reserved2;
} qmcp_hip_pair_stats;
int qmcp_hip_solve_pairs_host(qmcp_hip_ctx* ctx,
                              const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                              uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                              uint32_t max_coverage, const uint32_t* stages /* may be NULL */, uint32_t n_stages,
                              uint64_t* keep_mask_out, qmcp_hip_stats* stats, qmcp_hip_pair_stats* pstats);
int qmcp_hip_solve_pairs_device(qmcp_hip_ctx* ctx,
                                const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                uint32_t max_coverage, const uint32_t* stages /* may be NULL */, uint32_t n_stages,
                                uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                qmcp_hip_pair_stats* pstats);

/* Template-aware downsampling: the pair-aware staged solve with the unit of selection generalised from the reads
 * (2q, 2q + 1) to every segment that carries one template id.  One entry then serves single-end reads (templates of one
 * segment), pairs (two), long reads with supplementary alignments (every piece of a split read) and spliced reads (every
 * aligned block of the read and of its mate, so that an intron gets no depth).
 * Input: every row is a SEGMENT: one interval [start, end] on contig_id, or QMCP_NO_CONTIG; contig_lengths / n_contigs
 * and limits as in qmcp_hip_solve_by_contig_host.  template_ids[i] < n_templates <= 2^32 - 1 names the segment's
 * template.  The segments of a template may lie anywhere in the input and on any contigs, ids need not all be used, and
 * n_reads (the number of segments) may be odd.  stages as in qmcp_hip_solve_pairs_host: T_1 < ... < T_k = max_coverage,
 * k <= QMCP_PAIR_MAX_STAGES, NULL for {ceil(M / 2), M} ({1} for M = 1).
 * Definition: that of qmcp_hip_solve_pairs_host word for word, with complete_pairs replaced by
 *   complete_templates(S) = { i : some j in S has template_ids[j] == template_ids[i] }.
 * Credit comes from placed segments only; an unplaced segment is never a candidate and enters only through its
 * template.  Depth is counted per segment: two overlapping segments of one template count twice, as overlapping mates do
 * in the pairs entry.  The result S_k is a keep mask in INPUT order that holds whole templates and whose depth is at
 * least min(cov, max_coverage) everywhere.
 * Identities: (1) template_ids[i] = i / 2 with n_reads even gives the mask and the per-stage statistics of
 * qmcp_hip_solve_pairs_* for the same stages, bit for bit; (2) ids that are all distinct with the one stage
 * {max_coverage} give the mask of qmcp_hip_solve_by_contig_* bit for bit; (3) one stage gives
 * qmcp_hip_solve_by_contig_* at max_coverage followed by template completion.
 * Not claimed: that S_k is minimum among whole-template solutions.  (Depth counted once per template where its
 * segments overlap: qmcp_hip_solve_fragments_* below.)
 * Errors: the stage-list and max_coverage errors of qmcp_hip_solve_pairs_host, then template_ids == NULL or
 * n_templates == 0 with n_reads > 0 (QMCP_EINVAL), all on the host before the context is looked at and before anything
 * is copied.  An id >= n_templates is found on the device: QMCP_EINVAL with a message; the mask has been cleared by
 * then, as in the by-contig entries, and the host entry does not write keep_mask_out.  Bad contig ids and bad reads as in
 * qmcp_hip_solve_by_contig_host.
 * stats (may be NULL) are stage 1's; tstats (may be NULL): the stages and the templates.  The completion goes through a
 * bitset of n_templates bits and a count per template (n_templates / 8 + 4 * n_templates bytes of device memory).  The
 * host entry leaves S_k in the context, for qmcp_hip_kept_indices_host.  The device entry takes the four columns and the
 * mask in device memory, is ordered after `hip_stream` (or NULL) as qmcp_hip_solve_device is, and returns after the work
 * has completed. */
typedef struct qmcp_hip_template_stats {
    uint32_t n_stages, reserved;
    uint64_t n_selected[QMCP_PAIR_MAX_STAGES];        /* |K_j|, segments                                               */
    uint64_t n_kept[QMCP_PAIR_MAX_STAGES];            /* |S_j|, segments, after completion                             */
    uint64_t capped_positions[QMCP_PAIR_MAX_STAGES];  /* as in qmcp_hip_pair_stats                                     */
    uint64_t demand[QMCP_PAIR_MAX_STAGES];
    uint32_t target[QMCP_PAIR_MAX_STAGES];            /* T_j                                                           */
    uint32_t sweeps[QMCP_PAIR_MAX_STAGES];
    float ms_stage[QMCP_PAIR_MAX_STAGES];             /* device time of the stage's solves                             */
    float ms_templates;                               /* everything the feature adds around the solves: id check, sizes,
                                                         mask gather, compaction, credit, need, expansion, completion  */
    uint32_t max_template_size;                       /* segments of the largest template                              */
    uint64_t n_templates_used;                        /* templates with at least one segment                           */
    uint64_t n_templates_kept;                        /* templates in S_k                                              */
    uint64_t size_hist[8];                            /* templates of 1 .. 7 segments, and of 8 or more, over the
                                                         templates with at least one segment                           */
} qmcp_hip_template_stats;
int qmcp_hip_solve_templates_host(qmcp_hip_ctx* ctx,
                                  const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                  const uint32_t* template_ids, uint64_t n_reads, uint32_t n_templates,
                                  const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                  const uint32_t* stages /* may be NULL */, uint32_t n_stages,
                                  uint64_t* keep_mask_out, qmcp_hip_stats* stats, qmcp_hip_template_stats* tstats);
int qmcp_hip_solve_templates_device(qmcp_hip_ctx* ctx,
                                    const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                    const uint32_t* d_template_ids, uint64_t n_reads, uint32_t n_templates,
                                    const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                    const uint32_t* stages /* may be NULL */, uint32_t n_stages,
                                    uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                    qmcp_hip_template_stats* tstats);

/* Template-aware downsampling under a cap table: qmcp_hip_solve_templates_* with the region table of
 * qmcp_hip_solve_profile_* in the place of the one max_coverage -- whole templates, capped by region (a paired exome
 * under its targets, a split-read library under a hotspot profile).
 * Input: the segments, template_ids / n_templates and contig table of qmcp_hip_solve_templates_host; region_offsets (may be
 * NULL), region_starts / region_ends / region_caps, default_cap and flags of qmcp_hip_solve_profile_host (regions clipped,
 * disjoint per contig after clipping; flags must be 0); max_coverage = M >= 1, the scale of the schedule, and stages /
 * n_stages as in qmcp_hip_solve_templates_host: T_1 < ... < T_k = M, NULL for {ceil(M / 2), M}.  default_cap is independent
 * of M and may be 0.
 * Definition: cap(p) is the profile entry's.  The stage cap is c_j(p) = ceil(cap(p) * T_j / M), computed in 64 bits: it
 * never decreases in j, c_k = cap, and where cap(p) = M it is T_j.  S_0 is empty.  Stage j: credit_j(p) is the depth of
 * the placed segments of S_(j-1); K_j is the canonical selection of the profile entry over the placed segments not in
 * S_(j-1), alone, in input order, with need(p) = min(cov_rest(p), max(0, c_j(p) - credit_j(p)));
 * S_j = complete_templates(S_(j-1) | K_j).  The result is S_k: whole templates whose depth is at least
 * min(cov(p), cap(p)) everywhere (min(cov_rest, max(0, c - credit)) = max(0, min(cov, c) - credit) holds position by
 * position, so the depth of S_j is at least min(cov, c_j); completion only adds segments).  A segment that lies wholly on
 * cap-0 positions is never selected and enters only through its template.
 * Identities: (1) no region used and default_cap == M is qmcp_hip_solve_templates_*: the mask and every field of
 * qmcp_hip_template_stats, bit for bit (the call IS that entry); (2) ids that are all distinct with the one stage {M}
 * give the mask of qmcp_hip_solve_profile_* for the same table; (3) every cap equal to M, regions present, gives the mask
 * of qmcp_hip_solve_templates_* (another route, the same canonical rule); (4) one stage gives qmcp_hip_solve_profile_*
 * followed by template completion.
 * Not claimed: that S_k is minimum among whole-template solutions; that more stages are better.  (Fragment depth under a
 * cap table is two calls: qmcp_hip_clip_templates_* below, then this entry on its columns.)
 * Errors, all on the host before the context is looked at and before anything is copied or launched: those of
 * qmcp_hip_solve_templates_host (stage list, max_coverage == 0 or >= 2^31, template_ids == NULL, n_templates == 0), then
 * those of qmcp_hip_solve_profile_host (table shape QMCP_EINVAL, a cap or default_cap of 2^31 or more QMCP_ERANGE, unknown
 * flag bits QMCP_EINVAL).  An id >= n_templates is found on the device as in qmcp_hip_solve_templates_host, with the mask
 * cleared.
 * stats / tstats (may be NULL) as in qmcp_hip_solve_templates_host, target[j] = T_j.  qstats (may be NULL): the table as
 * in qmcp_hip_profile_stats; the placed segments that cover a position with cap(p) > 0 and the templates that own one;
 * ms_need, the device time of the kernels that build need[] (and of the cut-point scans behind them).  After an error
 * found on the device tstats holds the schedule without counts and qstats the table's counts without the on-cap counts.  Route: stage 1 is
 * the profile entry's batches at c_1 (a batch without regions takes the plain solve at ceil(default_cap * T_1 / M), a
 * batch whose largest c_1 is 0 keeps nothing); later stages are the templates entry's with need[] built by
 * k_tpl_profile_need from the batch's scaled regions and the credit; a batch whose largest c_j is 0 is skipped.  No
 * _begin / _end form. */
typedef struct qmcp_hip_template_profile_stats {
    uint64_t positions_in_regions;
    uint64_t n_segments_on_cap;                       /* placed segments that cover a position with cap(p) > 0         */
    uint64_t n_templates_on_cap;                      /* templates with at least one such segment                      */
    uint32_t regions_in, regions_used;
    float ms_need;
    uint32_t reserved;
} qmcp_hip_template_profile_stats;
int qmcp_hip_solve_templates_profile_host(qmcp_hip_ctx* ctx,
                                          const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                          const uint32_t* template_ids, uint64_t n_reads, uint32_t n_templates,
                                          const uint32_t* contig_lengths, uint32_t n_contigs,
                                          const uint32_t* region_offsets /* may be NULL */, const uint32_t* region_starts,
                                          const uint32_t* region_ends, const uint32_t* region_caps, uint32_t default_cap,
                                          uint32_t flags, uint32_t max_coverage,
                                          const uint32_t* stages /* may be NULL */, uint32_t n_stages,
                                          uint64_t* keep_mask_out, qmcp_hip_stats* stats, qmcp_hip_template_stats* tstats,
                                          qmcp_hip_template_profile_stats* qstats);
int qmcp_hip_solve_templates_profile_device(qmcp_hip_ctx* ctx,
                                            const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                            const uint32_t* d_template_ids, uint64_t n_reads, uint32_t n_templates,
                                            const uint32_t* contig_lengths, uint32_t n_contigs,
                                            const uint32_t* region_offsets /* may be NULL */, const uint32_t* region_starts,
                                            const uint32_t* region_ends, const uint32_t* region_caps, uint32_t default_cap,
                                            uint32_t flags, uint32_t max_coverage,
                                            const uint32_t* stages /* may be NULL */, uint32_t n_stages,
                                            uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                            qmcp_hip_template_stats* tstats, qmcp_hip_template_profile_stats* qstats);

/* Fragment depth: a template counts ONCE where its segments overlap.  The template entries above count depth per
 * segment, so where the two mates of a short-insert pair overlap one molecule is depth 2; here it is depth 1, as in
 * mosdepth, samtools depth -s and GATK.
 * Input: the segments of qmcp_hip_solve_templates_host: [start, end] inclusive on contig_id or QMCP_NO_CONTIG,
 * template_ids[i] < n_templates, contig_lengths / n_contigs and limits as in qmcp_hip_solve_by_contig_host.
 * Definition: clip(rows).  Take the placed segments of each (template id, contig) group in the order (start ascending,
 * input index ascending); reach is the largest end among the group's earlier members, if there are any.  A member with
 * start <= reach < end gets start' = reach + 1; a member with end <= reach becomes unplaced (its contig id becomes
 * QMCP_NO_CONTIG, its start is unchanged); every other row is unchanged.  Ends never change.  The output is two columns
 * in INPUT order: clipped starts and clipped contig ids.  After clip the placed segments of a template are pairwise
 * disjoint and their union per contig is the union before, so depth per segment on the clipped columns is FRAGMENT
 * DEPTH: the number of templates that cover a position.  clip is idempotent.  Gaps between mates are not filled.
 * qmcp_hip_clip_templates_* returns the two columns, for depth_report, depth_track or qmcp_hip_solve_templates_profile_*
 * (fragment depth there, in two calls).  qmcp_hip_solve_fragments_* is qmcp_hip_solve_templates_* on clip(rows), bit for
 * bit: the mask and every per-stage statistic.  An emptied segment is, like an unplaced one, never a candidate and
 * enters only through its template.  The result holds whole templates and its fragment depth is at least
 * min(fragment depth of all rows, max_coverage) everywhere.
 * Identities: (1) rows in which no two segments of one template overlap give qmcp_hip_solve_templates_*: the mask and
 * every field of qmcp_hip_template_stats except the times; (2) ids that are all distinct with the one stage
 * {max_coverage} give the mask of qmcp_hip_solve_by_contig_*.
 * Not claimed: that the result is minimum among whole-template solutions; physical coverage (the gap between mates); a
 * fused entry under a cap table; compositions with the other modes; a _begin / _end form.
 * Errors: those of qmcp_hip_solve_templates_host in its order (the clip entries: template_ids == NULL or n_templates == 0
 * with n_reads > 0), on the host before the context is looked at; then null buffers, the by-contig limits, and for the
 * clip entries an output that overlaps an input column (QMCP_EINVAL).  Then, on the device and BEFORE anything is
 * clipped: a template id >= n_templates (QMCP_EINVAL), a bad contig id (QMCP_EINVAL), a read with start > end or
 * end >= its contig's length (QMCP_EREAD), with the by-contig messages -- a bad row inside an overlapping group is not
 * hidden by being emptied.  After a device error the clip outputs are untouched; the solve's mask has been cleared, as
 * in the templates entry, and the host entry does not write keep_mask_out.
 * fstats (may be NULL).  A call in which no template has two segments is the identity: it costs the validation and a
 * copy and launches no sort or scan kernel.  Otherwise: a stable LSD radix sort of the rows by the bytes in use of
 * (template id, contig id, start), a segmented running maximum of the ends (no atomics, deterministic) and one pass that
 * writes both columns.  Device memory: 24 bytes per row for the sort, 8 for the clipped columns of the solve entries.
 * The solve entries never modify the caller's columns: the clipped copies live in the context.  The device entries take
 * the columns in device memory, are ordered after `hip_stream` (or NULL) as qmcp_hip_solve_device is, and return after
 * the work has completed. */
typedef struct qmcp_hip_fragment_stats {
    uint64_t n_placed;                 /* placed segments going in                                                     */
    uint64_t n_clipped;                /* start moved, still placed                                                    */
    uint64_t n_emptied;                /* inside what earlier members of the group cover: unplaced in the output       */
    uint64_t bases_in;                 /* bases of the placed segments going in                                        */
    uint64_t bases_removed;            /* bases clipped away = per-segment depth - fragment depth, summed              */
    uint64_t n_templates_overlapping;  /* templates with a clipped or emptied segment                                  */
    uint32_t max_group;                /* most placed segments of one template on one contig                           */
    float ms_clip;                     /* device time of the clip: validation, sort, scan, write-back                  */
} qmcp_hip_fragment_stats;
int qmcp_hip_clip_templates_host(qmcp_hip_ctx* ctx,
                                 const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                 const uint32_t* template_ids, uint64_t n_reads, uint32_t n_templates,
                                 const uint32_t* contig_lengths, uint32_t n_contigs,
                                 uint32_t* clipped_starts_out, uint32_t* clipped_contig_ids_out,
                                 qmcp_hip_fragment_stats* fstats);
int qmcp_hip_clip_templates_device(qmcp_hip_ctx* ctx,
                                   const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                   const uint32_t* d_template_ids, uint64_t n_reads, uint32_t n_templates,
                                   const uint32_t* contig_lengths, uint32_t n_contigs,
                                   uint32_t* d_clipped_starts_out, uint32_t* d_clipped_contig_ids_out, void* hip_stream,
                                   qmcp_hip_fragment_stats* fstats);
int qmcp_hip_solve_fragments_host(qmcp_hip_ctx* ctx,
                                  const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                  const uint32_t* template_ids, uint64_t n_reads, uint32_t n_templates,
                                  const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                  const uint32_t* stages /* may be NULL */, uint32_t n_stages,
                                  uint64_t* keep_mask_out, qmcp_hip_stats* stats, qmcp_hip_template_stats* tstats,
                                  qmcp_hip_fragment_stats* fstats);
int qmcp_hip_solve_fragments_device(qmcp_hip_ctx* ctx,
                                    const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                    const uint32_t* d_template_ids, uint64_t n_reads, uint32_t n_templates,
                                    const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                    const uint32_t* stages /* may be NULL */, uint32_t n_stages,
                                    uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                    qmcp_hip_template_stats* tstats, qmcp_hip_fragment_stats* fstats);

/* Ceiling downsampling: the kept depth never EXCEEDS the cap, and as many reads as possible are kept.  Every other entry
 * of this header is a floor (kept depth >= min(cov, cap), fewest reads) and may overshoot the cap; this one is for a hard
 * limit -- a pileup depth limit, a caller that degrades on a 100 000 x hotspot, a fixed memory budget per locus.
 * Input: reads, contig_ids (QMCP_NO_CONTIG = unplaced), contig_lengths / n_contigs, the region table (region_offsets,
 * may be NULL, region_starts / region_ends / region_caps), default_cap, limits and read validation exactly as in
 * qmcp_hip_solve_profile_host; without regions cap(p) = default_cap everywhere.
 * Answer: per contig, with cov the depth of its placed reads, D is the canonical selection (reads in input order; at the
 * leftmost position with a deficit take the unselected covering reads with the furthest end, then the furthest start,
 * then the lowest index: DESIGN.md sections 2 and 4.12) for need(p) = max(0, cov(p) - cap(p)).  D is the set of DROPPED
 * reads: bit i of the mask is set if and only if read i is placed and not in D.  Unplaced reads are never kept.
 * Guaranteed: kept(p) <= cap(p) at every position (kept <= cap is dropped >= cov - cap); |D| is minimum, so the kept set
 * is a maximum-cardinality subset of the placed reads under the ceiling; the result is deterministic; a cap of 0 drops
 * every read over that position; a contig that is nowhere above its cap keeps every placed read.
 * NOT guaranteed: kept(p) >= min(cov(p), cap(p)).  A hard ceiling can force the depth below the cap next to a deeper
 * position; short_positions / short_bases say where and by how much.  Inside a cell (reads of equal start and end) the
 * lowest index is DROPPED first; a quality-aware choice of which read to drop is not part of this entry.
 * flags: QMCP_CEILING_WHOLE_PAIRS -- reads (2q, 2q + 1) are pair q (n_reads must be even: QMCP_EINVAL otherwise); after the
 * solve a read is also dropped when its mate is in D (the mates' bits are ORed inside D before the complement), so the
 * mask holds whole pairs among the placed reads.  This only lowers depth: the ceiling still holds, but the maximum size
 * is no longer claimed.  An unplaced mate stays unkept whatever happens to its partner.
 * Route: the by-contig solve's grouping and batches; every batch with reads takes the sort-based mixed-span route of the
 * profile entries with need built by k_ceiling_need.  Its cut bit marks need(p) == cov(p) (cov == 0 or cap == 0), the
 * only positions behind which a stretch may start: where cov > cap over long runs a contig is one serial chain
 * (limits).  options.cut_points is honoured, nothing is speculated.  A batch that is nowhere above its
 * caps queues no sweep.  k_ceiling_check then holds the kept depth of every batch against the caps on the device.
 * Errors: as qmcp_hip_solve_profile_host -- a bad table, null arrays, unknown flag bits and an odd n_reads under
 * QMCP_CEILING_WHOLE_PAIRS are QMCP_EINVAL, a cap or default_cap of 2^31 or more is QMCP_ERANGE, all on the host before
 * anything is copied or launched (the output mask is not written); a bad contig id or read is found on the device.
 * stats (may be NULL): the batch-summed qmcp_hip_stats of the solves that select D (n_kept there counts D).
 * cstats (may be NULL): see the struct; short_*, excess_positions and max_kept_depth describe the solve's own mask,
 * before mates are dropped.  The device entry is ordered after hip_stream; both entries block (no _begin / _end form). */
#define QMCP_CEILING_WHOLE_PAIRS 1u
typedef struct qmcp_hip_ceiling_stats {
    uint64_t reads_placed;       /* placed reads                                                                      */
    uint64_t reads_dropped;      /* placed reads not kept, mates included                                             */
    uint64_t mates_dropped;      /* of those, the reads dropped only as mates (QMCP_CEILING_WHOLE_PAIRS)              */
    uint64_t over_positions;     /* positions with cov > cap                                                          */
    uint64_t over_bases;         /* the sum of cov - cap there                                                        */
    uint64_t short_positions;    /* positions with kept < min(cov, cap)                                               */
    uint64_t short_bases;        /* the sum of that shortfall                                                         */
    uint64_t excess_positions;   /* positions with kept > cap: 0 by contract, counted on the device all the same      */
    uint32_t max_kept_depth;     /* the largest kept depth                                                            */
    uint32_t regions_in, regions_used;  /* as in qmcp_hip_profile_stats                                               */
    float ms_ceiling;            /* device time of k_ceiling_need (+ cut-point scan), k_ceiling_check, k_ceiling_finish */
} qmcp_hip_ceiling_stats;
int qmcp_hip_solve_ceiling_host(qmcp_hip_ctx* ctx,
                                const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids, uint64_t n_reads,
                                const uint32_t* contig_lengths, uint32_t n_contigs,
                                const uint32_t* region_offsets /* may be NULL */, const uint32_t* region_starts,
                                const uint32_t* region_ends, const uint32_t* region_caps, uint32_t default_cap,
                                uint32_t flags, uint64_t* keep_mask_out, qmcp_hip_stats* stats,
                                qmcp_hip_ceiling_stats* cstats);
int qmcp_hip_solve_ceiling_device(qmcp_hip_ctx* ctx,
                                  const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                  uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                  const uint32_t* region_offsets /* may be NULL */, const uint32_t* region_starts,
                                  const uint32_t* region_ends, const uint32_t* region_caps, uint32_t default_cap,
                                  uint32_t flags, uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                  qmcp_hip_ceiling_stats* cstats);

/* Budget downsampling: the deepest coverage whose by-contig solve fits a number of reads.  Every other entry takes a
 * coverage and returns however many reads that costs; this one takes the reads a caller can afford (what samtools view -s,
 * Picard DownsampleSam and seqtk sample ask for) and searches the coverage on the device: one grouping, one pass over the
 * depth, a few whole solves.
 * Input: reads in any order, contig_ids (QMCP_NO_CONTIG = unplaced), contig_lengths / n_contigs, limits and read
 * validation exactly as in qmcp_hip_solve_by_contig_host; max_coverage (1 .. 2^31 - 1) is the upper end of the search.
 * Definitions: count(M), M >= 1, is the popcount of the mask qmcp_hip_solve_by_contig_host returns at M; under
 * QMCP_BUDGET_WHOLE_PAIRS after completion -- reads (2q, 2q + 1) are pair q (n_reads must be even), a placed read is
 * also kept when its placed mate is, an unplaced mate is never kept.  count(0) = 0.  top = min(max_coverage, largest depth
 * of the placed reads).
 * Answer: a coverage M* in 0 .. top (bstats->coverage) with
 *   (1) count(M*) <= budget_reads, and
 *   (2) M* == top or count(M* + 1) > budget_reads,
 * and in keep_mask_out exactly that solve's mask (after completion under the flag), bit for bit; M* == 0 is the all-zero
 * mask.  The result is deterministic.
 * Without the flag count is monotone -- the canonical selection has minimum cardinality among the covers of
 * need_M = min(cov, M), and need_M <= need_(M + 1) makes every cover for M + 1 a cover for M -- so M* is
 * the one largest feasible coverage.  WITH the flag monotonicity has been observed and is NOT proven: only (1) and (2) are
 * promised.  budget_reads >= the placed reads gives M* == top, and where top is the largest depth (max_coverage at least
 * that) every placed read is kept: saturated = 1.
 * curve_out (may be NULL, then curve_capacity must be 0): curve_out[M] = S(M) = the sum over all positions of
 * min(cov(p), M) for M = 0 .. min(top, QMCP_BUDGET_CURVE_MAX, curve_capacity - 1): the bases any valid answer at M must
 * hold -- read it to pick a budget.  A HOST array in both entries; bstats->curve_entries says how many were written.
 * Errors: null arrays, unknown flag bits, an odd n_reads under QMCP_BUDGET_WHOLE_PAIRS, max_coverage == 0 or a
 * curve_capacity without curve_out are QMCP_EINVAL, max_coverage >= 2^31 is QMCP_ERANGE, all on the host before anything
 * is copied or launched; a bad contig id or read is found on the device with the codes of the by-contig entry.  The
 * output mask is written by a successful call only.
 * stats (may be NULL): the batch-summed qmcp_hip_stats of the probe at M* (zeros for M* == 0).  bstats (may be NULL): see
 * the struct.  The device entry is ordered after hip_stream; both entries block (no _begin / _end form). */
#define QMCP_BUDGET_WHOLE_PAIRS 1u
#define QMCP_BUDGET_CURVE_MAX 8191u
typedef struct qmcp_hip_budget_stats {
    uint64_t budget;         /* the budget given                                                                      */
    uint64_t reads_placed;   /* placed reads                                                                          */
    uint64_t n_kept;         /* count(M*)                                                                             */
    uint64_t kept_above;     /* count(M* + 1) when a probe measured it, else 0                                        */
    uint64_t bound_above;    /* else the lower bound of count(M* + 1) that ruled M* + 1 out; 0 when M* == top         */
    uint64_t total_bases;    /* the sum of the depth over all positions                                               */
    uint32_t coverage;       /* M*                                                                                    */
    uint32_t max_depth;      /* the largest depth of the placed reads                                                 */
    uint32_t top;            /* min(max_coverage, max_depth)                                                          */
    uint32_t probes;         /* whole solves run                                                                      */
    uint32_t curve_entries;  /* entries written to curve_out                                                          */
    uint32_t saturated;      /* 1 when every placed read is kept                                                      */
    float ms_budget;         /* device time of k_budget_tally, k_budget_curve and k_budget_finish                     */
    float ms_solves;         /* device time of the probes' solves                                                     */
} qmcp_hip_budget_stats;
int qmcp_hip_solve_budget_host(qmcp_hip_ctx* ctx,
                               const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids, uint64_t n_reads,
                               const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                               uint64_t budget_reads, uint32_t flags, uint64_t* curve_out /* may be NULL */,
                               uint32_t curve_capacity, uint64_t* keep_mask_out, qmcp_hip_stats* stats,
                               qmcp_hip_budget_stats* bstats);
int qmcp_hip_solve_budget_device(qmcp_hip_ctx* ctx,
                                 const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                 uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                 uint64_t budget_reads, uint32_t flags, uint64_t* curve_out /* host; may be NULL */,
                                 uint32_t curve_capacity, uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                 qmcp_hip_budget_stats* bstats);

/* Mean-depth downsampling: the deepest coverage whose by-contig solve fits a number of BASES -- "make this 80 x genome
 * 30 x", "bring the exome to 100 x mean on target".  The budget entries above answer in reads; a mean depth is a budget in
 * bases, budget_bases = floor(mean * |R|), over a region set R: the whole genome, or the target regions whose mean Picard
 * reports as MEAN_TARGET_COVERAGE.
 * Input: reads, contig_ids, contig_lengths / n_contigs, limits and read validation exactly as in
 * qmcp_hip_solve_by_contig_host; max_coverage (1 .. 2^31 - 1) is the upper end of the search.  region_offsets (n_contigs +
 * 1 entries) / region_starts / region_ends in the form of qmcp_hip_solve_targets_host: inclusive bounds, any order,
 * overlapping and nested regions allowed, clipped to the contig, a region that begins at or beyond the contig's length
 * dropped, no padding.  R_c is the union of contig c's regions.  region_offsets == NULL: R_c is all of contig c.  A table
 * that is present but empty is legal: R is empty.
 * Definitions: keep_M, M >= 1, is the mask qmcp_hip_solve_by_contig_host returns at M; under QMCP_MEAN_DEPTH_WHOLE_PAIRS
 * after the completion of QMCP_BUDGET_WHOLE_PAIRS (reads (2q, 2q + 1) are pair q, n_reads must be even, a placed read is
 * also kept when its placed mate is, an unplaced mate is never kept).  keep_0 is empty.  bases(M) = the sum over the placed
 * reads i in keep_M of |[start_i, end_i] n R_contig(i)|: the kept depth summed over the positions of R.  top =
 * min(max_coverage, largest depth of the placed reads) -- the depth over ALL positions, not only those of R: the mask
 * changes up to there.
 * Answer: a coverage M* in 0 .. top (mstats->coverage) with
 *   (1) bases(M*) <= budget_bases, and
 *   (2) M* == top or bases(M* + 1) > budget_bases,
 * and in keep_mask_out exactly keep_M*, bit for bit; M* == 0 is the all-zero mask.  The result is deterministic.
 * Monotonicity of bases(M) has been observed on every input tried and is NOT proven, with or without regions or the flag:
 * only (1) and (2) are promised.  Where bases is non-decreasing, M* is the one largest feasible coverage.
 * Bound: S_R(M) = the sum over the positions p of R of min(cov(p), M) <= bases(M), because every valid answer at M keeps
 * at least min(cov, M) at every position.  curve_out (may be NULL, then curve_capacity must be 0): curve_out[M] = S_R(M)
 * for M = 0 .. min(top, QMCP_BUDGET_CURVE_MAX, curve_capacity - 1).  A HOST array in both entries.
 * Errors, all decided from the arguments before the context is looked at: those of qmcp_hip_solve_budget_host -- null
 * arrays, unknown flag bits, an odd n_reads under the flag, max_coverage == 0 or a curve_capacity without curve_out are
 * QMCP_EINVAL; max_coverage >= 2^31, too many contigs or reads are QMCP_ERANGE --, then those of the targets entry for the
 * region table -- offsets that do not start at 0 or decrease, a NULL column with a non-zero count, a region with start >
 * end: QMCP_EINVAL.  A bad contig id or read is found on the device with the codes of the by-contig entry.  The output mask
 * is written by a successful call only.
 * stats (may be NULL): the batch-summed qmcp_hip_stats of the probe at M* (zeros for M* == 0).  mstats (may be NULL): see
 * the struct.  The device entry is ordered after hip_stream; both entries block (no _begin / _end form). */
#define QMCP_MEAN_DEPTH_WHOLE_PAIRS 1u
typedef struct qmcp_hip_mean_depth_stats {
    uint64_t budget;         /* budget_bases as given                                                                  */
    uint64_t positions;      /* |R|: the positions of the merged, clipped regions; every position without a table       */
    uint64_t reads_placed;   /* placed reads                                                                           */
    uint64_t n_kept;         /* reads in keep_M*                                                                       */
    uint64_t kept_bases;     /* bases(M*)                                                                              */
    uint64_t bases_above;    /* bases(M* + 1) when a probe measured it, else 0                                         */
    uint64_t bound_above;    /* else S_R(M* + 1), the bound that ruled M* + 1 out; both are 0 when M* == top            */
    uint64_t total_bases;    /* the sum of the depth over the positions of R                                           */
    uint32_t coverage;       /* M*                                                                                     */
    uint32_t max_depth;      /* the largest depth of the placed reads, over all positions                              */
    uint32_t top;            /* min(max_coverage, max_depth)                                                           */
    uint32_t probes;         /* whole solves run                                                                       */
    uint32_t curve_entries;  /* entries written to curve_out                                                           */
    uint32_t saturated;      /* 1 when every placed read is kept                                                       */
    uint32_t regions_in;     /* regions given (0 without a table)                                                      */
    uint32_t regions_used;   /* regions after clipping and merging                                                     */
    float ms_mean_depth;     /* device time of k_md_weights, the tallies, k_budget_curve, k_budget_finish, k_md_count   */
    float ms_solves;         /* device time of the probes' solves                                                      */
} qmcp_hip_mean_depth_stats;
int qmcp_hip_solve_mean_depth_host(qmcp_hip_ctx* ctx,
                                   const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                   uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                   uint32_t max_coverage, uint64_t budget_bases,
                                   const uint32_t* region_offsets /* may be NULL */, const uint32_t* region_starts,
                                   const uint32_t* region_ends, uint32_t flags, uint64_t* curve_out /* may be NULL */,
                                   uint32_t curve_capacity, uint64_t* keep_mask_out, qmcp_hip_stats* stats,
                                   qmcp_hip_mean_depth_stats* mstats);
int qmcp_hip_solve_mean_depth_device(qmcp_hip_ctx* ctx,
                                     const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                     uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                     uint32_t max_coverage, uint64_t budget_bases,
                                     const uint32_t* region_offsets /* host; may be NULL */, const uint32_t* region_starts,
                                     const uint32_t* region_ends, uint32_t flags, uint64_t* curve_out /* host; may be NULL */,
                                     uint32_t curve_capacity, uint64_t* d_keep_mask_out, void* hip_stream,
                                     qmcp_hip_stats* stats, qmcp_hip_mean_depth_stats* mstats);

/* Coverage thresholds: one call tags every read with the smallest coverage that keeps it -- a titration, a rarefaction
 * curve, "tag the BAM once, cut any downsample later with a filter".  Every other entry answers "which reads at coverage
 * M"; this one answers it for every M in coverage_lo .. coverage_hi at once, in one 16-bit integer per read.
 * Input: reads, contig_ids, contig_lengths / n_contigs, limits and read validation exactly as in
 * qmcp_hip_solve_by_contig_host; 1 <= coverage_lo <= coverage_hi <= QMCP_THRESHOLDS_COVERAGE_MAX.
 * Definitions: keep_M is the mask qmcp_hip_solve_by_contig_host returns at M.
 * Thresholds: thresholds_out[i] (n_reads entries) is the smallest M in coverage_lo .. coverage_hi with i in keep_M, and
 * QMCP_THRESHOLD_NEVER for an unplaced read and for a read that no such M keeps.  Reads kept at coverage_lo get
 * coverage_lo.  This definition needs nothing of the shape of the sets keep_M.
 * Stop: M ascends from coverage_lo, one whole solve each, and solving stops after the first M at which every placed read
 * has a threshold, or at coverage_hi: that M is tstats->top.  Later solves could not assign anything.
 * Violations: tstats->nesting_violations counts the (read, M) pairs with coverage_lo <= M <= top in which a read that
 * already has a threshold is not in keep_M.  WHILE IT IS 0, (thresholds_out[i] <= M) IS keep_M, BIT FOR BIT, FOR EVERY M
 * IN coverage_lo .. coverage_hi.  That the kept sets are nested in M -- the count is 0 -- has been observed on every input
 * tried (exhaustively on small contigs, and on random inputs at every coverage) and is NOT proven; a caller that relies
 * on the equivalence checks the count.
 * QMCP_THRESHOLDS_WHOLE_PAIRS: reads (2q, 2q + 1) are pair q and n_reads must be even.  A placed read takes the smaller
 * of its own threshold and its PLACED mate's; an unplaced mate lends nothing and stays QMCP_THRESHOLD_NEVER.  Then
 * (thresholds_out[i] <= M) is the mask of QMCP_BUDGET_WHOLE_PAIRS's completion of keep_M (while the count is 0).
 * Counts: counts_out (may be NULL, then counts_capacity must be 0) [M - coverage_lo] = the reads with final threshold <= M,
 * for M = coverage_lo .. min(coverage_hi, coverage_lo + counts_capacity - 1); tstats->count_entries entries are written.
 * A HOST array in both entries.
 * Errors, all decided from the arguments before the context is looked at: null arrays, unknown flag bits, an odd n_reads
 * under the flag, coverage_lo == 0, coverage_lo > coverage_hi and a counts_capacity without counts_out are QMCP_EINVAL;
 * coverage_hi > QMCP_THRESHOLDS_COVERAGE_MAX, n_contigs > 2^24 and n_reads > 2^31 are QMCP_ERANGE.  A bad contig id or
 * read is found on the device with the codes of the by-contig entry, and thresholds_out is then left untouched.
 * stats (may be NULL): the batch-summed qmcp_hip_stats of the last solve (at top).  tstats (may be NULL): see the struct.
 * The device entry is ordered after hip_stream; both entries block (no _begin / _end form). */
#define QMCP_THRESHOLD_NEVER 0xFFFFu
#define QMCP_THRESHOLDS_COVERAGE_MAX 65534u
#define QMCP_THRESHOLDS_WHOLE_PAIRS 1u
typedef struct qmcp_hip_thresholds_stats {
    uint64_t reads_placed;        /* placed reads                                                                       */
    uint64_t n_kept;              /* reads with final threshold <= coverage_hi                                          */
    uint64_t nesting_violations;  /* see above; 0 on every input seen so far                                            */
    uint32_t coverage_lo;         /* as given                                                                           */
    uint32_t coverage_hi;         /* as given                                                                           */
    uint32_t top;                 /* the last coverage solved                                                           */
    uint32_t solves;              /* whole solves run: top - coverage_lo + 1                                            */
    uint32_t saturated;           /* 1 when every placed read has a threshold                                           */
    uint32_t count_entries;       /* entries written to counts_out                                                      */
    float ms_thresholds;          /* device time of k_thresholds_step, k_thresholds_finish, k_thresholds_counts         */
    float ms_solves;              /* device time of the solves                                                          */
} qmcp_hip_thresholds_stats;
int qmcp_hip_solve_thresholds_host(qmcp_hip_ctx* ctx,
                                   const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                   uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                   uint32_t coverage_lo, uint32_t coverage_hi, uint32_t flags, uint16_t* thresholds_out,
                                   uint64_t* counts_out /* may be NULL */, uint32_t counts_capacity, qmcp_hip_stats* stats,
                                   qmcp_hip_thresholds_stats* tstats);
int qmcp_hip_solve_thresholds_device(qmcp_hip_ctx* ctx,
                                     const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                     uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                     uint32_t coverage_lo, uint32_t coverage_hi, uint32_t flags, uint16_t* d_thresholds_out,
                                     uint64_t* counts_out /* host; may be NULL */, uint32_t counts_capacity,
                                     void* hip_stream, qmcp_hip_stats* stats, qmcp_hip_thresholds_stats* tstats);

/* Proportional downsampling: keep a fraction of the depth everywhere.  Every other solving entry asks for a flat depth,
 * min(cov(p), cap) with a cap from outside the data; this one takes its demand from the data's own depth, so the SHAPE of
 * the coverage survives (copy-number calling, ChIP / ATAC / RNA signal, allele balance, "this run at a quarter of the
 * sequencing") -- exactly at every position, where samtools view -s keeps the shape only in expectation.
 * Input: reads in any order, contig_ids (QMCP_NO_CONTIG = unplaced), contig_lengths / n_contigs, limits and read
 * validation exactly as in qmcp_hip_solve_by_contig_host.  num / den with 0 <= num <= den and 1 <= den <=
 * QMCP_PROPORTION_DEN_MAX is the fraction; floor and max_coverage (< 2^31; 2^31 - 1: no limit) bound the demand.
 * Answer: per contig, with cov the depth of its placed reads, all in exact integer arithmetic,
 *   q(p)    = ceil(cov(p) * num / den)
 *   need(p) = min(cov(p), max_coverage, max(q(p), floor))
 * and the mask is the canonical selection (reads in input order; at the leftmost position with a deficit take the
 * unselected covering reads with the furthest end, then the furthest start, then the lowest index: DESIGN.md sections 2
 * and 4.12) under this need.  Every position keeps at least the fraction of its depth, rounded up; positions at or below
 * floor are kept whole; max_coverage stays a hard upper end of the demand.  Unplaced reads are never kept.
 * Guaranteed: kept(p) >= need(p) everywhere with the fewest reads; the result is deterministic.  NOT guaranteed: an upper
 * bound on kept(p) -- a read kept for one position covers its neighbours too, as in every floor entry.
 * Identities: (1) num == den or floor >= max_coverage gives the mask and the qmcp_hip_stats of qmcp_hip_solve_by_contig_*
 * at max_coverage (the call IS that entry, every fast route of it included); (2) num == 0 gives that entry at
 * min(floor, max_coverage), and nothing at 0; (3) otherwise the mask is that of qmcp_hip_solve_profile_* under the region
 * table that spells need out with default_cap 0.
 * Route of (3): the by-contig solve's grouping and batches; every batch with reads takes the sort-based mixed-span route
 * of the profile entries with need built by k_prop_need.  Its cut bit marks need(p) == cov(p), the only positions behind
 * which a stretch may start: deep data under a fraction is one serial chain per contig (limits).
 * options.cut_points is honoured, nothing is speculated.
 * Errors, all on the host before anything is copied or launched (the output mask is not written): null arrays, den == 0,
 * num > den and unknown flag bits (flags must be 0) are QMCP_EINVAL; den > QMCP_PROPORTION_DEN_MAX and max_coverage >=
 * 2^31 are QMCP_ERANGE.  A bad contig id or read is found on the device with the codes of the by-contig entry.
 * stats (may be NULL): the batch-summed qmcp_hip_stats.  pstats (may be NULL): see the struct.  The device entry is
 * ordered after hip_stream; both entries block (no _begin / _end form). */
#define QMCP_PROPORTION_DEN_MAX (1u << 20)
typedef struct qmcp_hip_proportional_stats {
    uint64_t reads_placed;     /* placed reads                                                                       */
    uint64_t bases_in;         /* the sum of their spans                                                             */
    uint64_t bases_kept;       /* the sum of the kept reads' spans                                                   */
    uint64_t demand;           /* the sum of need(p)                                                                 */
    uint64_t whole_positions;  /* positions with cov > 0 and need == cov                                             */
    uint64_t floor_positions;  /* positions with q < min(floor, cov, max_coverage): the floor (or the depth) decides  */
    uint64_t capped_positions; /* positions with max(q, floor) > max_coverage and cov > max_coverage                 */
    uint32_t max_depth;        /* the largest depth                                                                  */
    uint32_t max_need;         /* the largest need                                                                   */
    uint32_t num, den, floor;  /* as given                                                                           */
    uint32_t plain_route;      /* 1: identity (1) or (2) applied; demand, the position counters and the two maxima
                                  are then 0                                                                         */
    float ms_need;             /* device time of k_prop_need (+ the cut-point scan), summed over the batches         */
    float ms_tally;            /* device time of k_prop_tally                                                        */
} qmcp_hip_proportional_stats;
int qmcp_hip_solve_proportional_host(qmcp_hip_ctx* ctx,
                                     const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                     uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                     uint32_t num, uint32_t den, uint32_t floor, uint32_t max_coverage, uint32_t flags,
                                     uint64_t* keep_mask_out, qmcp_hip_stats* stats,
                                     qmcp_hip_proportional_stats* pstats);
int qmcp_hip_solve_proportional_device(qmcp_hip_ctx* ctx,
                                       const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                       uint64_t n_reads, const uint32_t* contig_lengths, uint32_t n_contigs,
                                       uint32_t num, uint32_t den, uint32_t floor, uint32_t max_coverage, uint32_t flags,
                                       uint64_t* d_keep_mask_out, void* hip_stream, qmcp_hip_stats* stats,
                                       qmcp_hip_proportional_stats* pstats);

/* Start cap: at most K kept reads per alignment start.  The canonical selection fills a deficit from the reads with the
 * furthest end, which on deep one-length data are the reads that start where the deficit opens: the kept reads pile up
 * on a few start positions.  Here every start site may offer the solve at most K reads (GATK's
 * --max-reads-per-alignment-start, MACS' --keep-dup k).  starts, ends, contig_ids, n_reads, contig_lengths / n_contigs,
 * max_coverage, keep_mask_out, stats, limits (n_reads <= 2^31, n_contigs <= 2^24) and errors are those of
 * qmcp_hip_solve_by_contig_host / _device.  In addition:
 *   cap         K >= 1; 0 fails with QMCP_EINVAL.
 *   groups      one uint32 per read, any value (strand, sample); NULL: one group.  Any range of values is fine.
 *   priorities  one uint32 per read, higher is better (MAPQ); NULL: all equal.  A range (max - min over the placed
 *               reads) above 65535 fails with QMCP_ERANGE before anything is written, as dedup's quality range does.
 *   flags       QMCP_START_CAP_SHORTFALL asks for short_positions / short_bases; unknown bits fail with QMCP_EINVAL.
 *   capped_mask_out  may be NULL; ceil(n_reads / 64) words, fully overwritten.
 *   hist_out, hist_bins  may be NULL / 0; hist_bins uint64 words in host memory (both entries), at most 4096 bins
 *               (QMCP_ERANGE beyond).
 *   cstats      may be NULL.
 * CELL: the cell of a placed read is (contig, start, group).  Unplaced reads belong to no cell and are never kept.
 * ORDER inside a cell: priority descending, then span (end - start) descending, then input index ascending.  Longest
 * first is deliberate: it is the read the canonical rule would prefer, and it makes the survivors independent of the
 * input order up to index ties.
 * SURVIVORS: the first min(K, size) reads of every cell in that order.  The other placed reads are CAPPED.
 * RESULT: keep_mask_out is the mask qmcp_hip_solve_by_contig_host returns for the survivors in input order at
 * max_coverage, bit for bit, mapped back to input positions; every other bit is clear.  Bit i of capped_mask_out is set
 * iff read i is capped, so keep & capped == 0 always.  hist_out[k - 1] is the number of cells of size k for k <
 * hist_bins, the last bin holds the sizes >= hist_bins.
 * PROMISES: (1) at most K kept reads per cell.  (2) The kept depth is >= min(cov of the survivors, max_coverage)
 * everywhere, with minimum cardinality for that demand.  (3) If no cell is larger than K the keep mask is
 * qmcp_hip_solve_by_contig_host's bit for bit.  (4) With one span length in the call, groups == NULL and K == 1, the keep
 * mask and the capped mask are qmcp_hip_solve_dedup_host's read mode (tags NULL, the priorities as qualities) keep mask
 * and duplicate mask bit for bit.  (5) The same input gives the same masks, run to run.
 * NOT PROMISED: kept depth >= min(cov, max_coverage) of ALL placed reads; that is what the shortfall reports.  With
 * QMCP_START_CAP_SHORTFALL short_positions counts the positions where the kept depth is below min(cov of all placed
 * reads, max_coverage) and short_bases sums the deficit there; they are counted on the device by the depth report's pass
 * (its limit applies: n_reads < 2^31, QMCP_ERANGE otherwise).
 * VALIDATION: every read is validated as the by-contig entries do -- the capped reads too -- before anything is written:
 * a bad contig id gives QMCP_EINVAL, a bad read QMCP_EREAD, and no output buffer has been touched.
 * HOW: one pass validates and takes the ranges of group, priority and span; the widths of the key gstart | group -
 * group_min | prio_max - prio | span_max - span come from those ranges (a NULL column and one span cost nothing); dedup's
 * stable LSD radix sorts {key, index} as 32-bit records, as split 64-bit keys, or -- beyond 64 bits -- field by field.
 * A cell then is a run of the sorted order with its best read first; rank = position - the cell's first position, a
 * survivor below K, capped from K on.  The survivors are compacted in input order, solved, and the mask expanded; one more
 * pass over the sorted records counts the kept reads per cell from the final mask.
 * stats (may be NULL) are the inner solve's: n_reads counts the survivors.
 * The pass is blocking (no _begin / _end form).  The device entry takes the columns and both masks in device memory
 * (contig_lengths, hist_out and the stats stay on the host), columns at any 4-byte alignment, and is ordered after
 * `hip_stream` (or NULL) as qmcp_hip_solve_device is.  The host entry leaves the keep mask in the context. */
#define QMCP_START_CAP_SHORTFALL 1u
typedef struct qmcp_hip_start_cap_stats {
    uint64_t reads_placed;       /* reads with a contig                                                               */
    uint64_t cells;              /* distinct (contig, start, group) among them                                        */
    uint64_t cells_over_cap;     /* cells with more than K reads                                                      */
    uint64_t reads_capped;       /* reads_placed - reads_survived                                                     */
    uint64_t largest_cell;       /* reads of the largest cell                                                         */
    uint64_t reads_survived;     /* reads handed to the inner solve                                                   */
    uint64_t cells_kept;         /* cells with at least one kept read: the diversity of the kept set                  */
    uint64_t largest_kept_cell;  /* kept reads of the cell with the most (<= K), counted from the final mask          */
    uint64_t short_positions;    /* QMCP_START_CAP_SHORTFALL: positions with kept < min(cov of all placed reads, M)    */
    uint64_t short_bases;        /* QMCP_START_CAP_SHORTFALL: the deficit summed over them; both 0 without the flag   */
    uint32_t key_bits;           /* width of the key the reads were sorted by                                         */
    uint32_t sort_passes;        /* 8-bit LSD passes                                                                  */
    uint32_t cap;                /* K as given                                                                        */
    float ms_cap;                /* device time of everything except the inner solve                                  */
} qmcp_hip_start_cap_stats;
int qmcp_hip_solve_start_cap_host(qmcp_hip_ctx* ctx,
                                  const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                  const uint32_t* groups, const uint32_t* priorities, uint64_t n_reads,
                                  const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage, uint32_t cap,
                                  uint32_t flags, uint64_t* keep_mask_out, uint64_t* capped_mask_out, uint64_t* hist_out,
                                  uint32_t hist_bins, qmcp_hip_stats* stats, qmcp_hip_start_cap_stats* cstats);
int qmcp_hip_solve_start_cap_device(qmcp_hip_ctx* ctx,
                                    const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                    const uint32_t* d_groups, const uint32_t* d_priorities, uint64_t n_reads,
                                    const uint32_t* contig_lengths, uint32_t n_contigs, uint32_t max_coverage,
                                    uint32_t cap, uint32_t flags, uint64_t* d_keep_mask_out, uint64_t* d_capped_mask_out,
                                    uint64_t* hist_out, uint32_t hist_bins, void* hip_stream, qmcp_hip_stats* stats,
                                    qmcp_hip_start_cap_stats* cstats);

/* Amplicon-aware downsampling: primer-clipped depth, optionally one coverage problem per amplicon.  On a tiled amplicon
 * panel the primer bases are synthetic and every pipeline masks them before calling variants, so depth that counts them
 * overstates what is left after trimming.  Here every unit of reads is assigned to ONE amplicon of its contig, its reads
 * are clipped to that amplicon's insert (the amplicon without its primers), and the clipped reads are solved.  starts,
 * ends, contig_ids, seq_lengths, qualities, n_reads, contig_lengths / n_contigs, amp_offsets / amp_starts / amp_ends,
 * min_length, min_mapq, max_coverage, keep_mask_out, stats, limits (n_reads <= 2^31, n_contigs <= 2^24) and errors are
 * those of qmcp_hip_filter_solve_by_contig_host.  In addition:
 *   amp_offsets        must be given (QMCP_EINVAL when NULL): this entry is about amplicons; filtering without them
 *                      stays with qmcp_hip_filter_solve_by_contig_host.
 *   amp_insert_starts, amp_insert_ends  one word per amplicon, inclusive, parallel to amp_starts / amp_ends; both NULL:
 *                      the insert is the amplicon and nothing is clipped.  amp_start <= insert_start <= insert_end <=
 *                      amp_end must hold for every amplicon: otherwise QMCP_EINVAL names the first one that breaks it,
 *                      before anything is copied.
 *   flags              QMCP_AMPLICONS_SINGLE_END, QMCP_AMPLICONS_PER_AMPLICON, QMCP_AMPLICONS_COMPLETE_PAIRS; unknown
 *                      bits fail with QMCP_EINVAL.
 *   amplicon_of_out    may be NULL; one uint32 per unit in host memory (both entries).
 *   amplicon_rows      may be NULL; one qmcp_hip_depth_row per amplicon in host memory (both entries).
 *   astats             may be NULL.
 * UNIT: the pair of reads 2q, 2q + 1 (n_reads even, QMCP_EINVAL otherwise); with QMCP_AMPLICONS_SINGLE_END one read, and
 * n_reads may be odd.
 * FILTERING: a unit passes min_length / min_mapq exactly as in the FILTER (every read of it, when the column is given).
 * ASSIGNMENT: a unit that passed the filters is assigned to an amplicon of its contig that contains all of its reads:
 * every read placed, all on one contig, amp_start <= the smallest start and amp_end >= the largest end (the OUTER bounds,
 * inclusive: Amplicon::includes, as in the FILTER).  If several amplicons contain it: the greatest start, then the
 * smallest end, then the smallest index in the caller's table; the unit also counts in units_in_several.  A unit that no
 * amplicon contains has none (QMCP_NO_AMPLICON) and is dropped.
 * CLIPPING: every read of an assigned unit is intersected with its amplicon's insert.  A read wholly inside a primer is
 * unplaced for the solve: it is never selected itself and comes back only through mate completion.
 * SOLVE, pooled (default): qmcp_hip_solve_by_contig_host on the clipped reads of the assigned units, in genome
 * coordinates, in input order -- step 3 of qmcp_hip_filter_solve_by_contig_host on the clipped columns.
 * SOLVE, QMCP_AMPLICONS_PER_AMPLICON: every amplicon is a coverage problem of its own: its assigned reads, rebased to the
 * insert (start - insert_start), solved in input order on a contig of the insert's length -- the by-contig solve with
 * the amplicon's index as contig id; the mask is the union.  At most 2^24 amplicons then, and whenever amplicon_rows is
 * given (QMCP_ERANGE beyond).  It keeps more reads than the pooled solve, and where inserts overlap the kept depth can
 * reach the sum of the overlapping amplicons' caps.
 * MATES: QMCP_AMPLICONS_COMPLETE_PAIRS completes the mates of the kept reads as the FILTER flow's complete_pairs does;
 * together with QMCP_AMPLICONS_SINGLE_END it is QMCP_EINVAL.
 * OUTPUTS: keep_mask_out in input order.  amplicon_of_out[u]: the amplicon's index in the caller's table, or
 * QMCP_NO_AMPLICON.  amplicon_rows[k], in the caller's table order, covers the insert of amplicon k: contig = k, start /
 * end = the insert in genome coordinates; the `in` fields are the depth of the clipped reads assigned to k, the `kept`
 * fields that of those in the FINAL mask (after completion), the deficits are against min(in, max_coverage).  The rows
 * come from the depth report's device pass over the rebased columns (its limit applies: n_reads < 2^31); nothing per
 * position crosses the link.
 * PROMISES: (1) with both insert arrays NULL, pooled, the keep mask is qmcp_hip_filter_solve_by_contig_host's bit for bit
 * for the same arguments, with and without completion.  (2) With disjoint amplicons (an uncovered base between any two),
 * inserts NULL and every unit inside one amplicon, both modes give the same mask.  (3) Single-end, inserts NULL, one
 * amplicon spanning each whole contig: the mask is qmcp_hip_solve_by_contig_host's.  (4) The same input gives the same
 * outputs, run to run.
 * VALIDATION: every read is validated as the FILTER does -- those of dropped units too -- before any output is written:
 * a bad contig id gives QMCP_EINVAL, a bad read QMCP_EREAD, and no output buffer has been touched.  The same holds for
 * everything the call refuses from its arguments.  It does NOT hold for a failure after validation (an allocation or a
 * HIP error in the solve or in the rows' pass): the device entry's mask may then have been written; labels, rows and
 * stats are still untouched.
 * HOW: the host sorts each contig's amplicons by (start ascending, end descending, index descending) and keeps the
 * running maximum of the ends.  One streaming kernel validates, filters, finds the last amplicon starting at or before
 * the unit's smallest start by binary search and walks backwards to the first container -- one or two steps on a tiled
 * panel, linear in the contig's amplicons on a deeply nested table --, clips, and writes the label, one keep bit per unit
 * and the clipped columns.  Up to 2 560 amplicons are staged in LDS (60 KiB, two workgroups a CU); larger tables are read
 * from global memory.  The surviving units are compacted in input order, solved, and the mask expanded back.
 * stats (may be NULL) are the inner solve's: n_reads counts the reads of the assigned units.
 * The pass is blocking (no _begin / _end form); a context with a pending qmcp_hip_solve_device_begin is refused.  The
 * device entry takes the five columns and the mask in device memory (tables, labels, rows and stats stay on the host)
 * and is ordered after `hip_stream` (or NULL) as qmcp_hip_solve_device is.  With pairs its kernel reads a pair as one
 * 8-byte word: columns that are not 8-byte aligned are REFUSED with QMCP_EINVAL (single-end takes any 4-byte alignment).
 * The host entry leaves the keep mask in the context. */
#define QMCP_AMPLICONS_SINGLE_END 1u
#define QMCP_AMPLICONS_PER_AMPLICON 2u
#define QMCP_AMPLICONS_COMPLETE_PAIRS 4u
#define QMCP_NO_AMPLICON 0xFFFFFFFFu
typedef struct qmcp_hip_amplicons_stats {
    uint64_t units;               /* pairs, or reads with QMCP_AMPLICONS_SINGLE_END                                    */
    uint64_t units_assigned;      /* units with an amplicon: what the solve sees                                       */
    uint64_t units_filtered;      /* units dropped by min_length / min_mapq                                            */
    uint64_t units_no_amplicon;   /* units that passed the filters and lie in no amplicon                              */
    uint64_t units_in_several;    /* assigned units that more than one amplicon contains                               */
    uint64_t reads_shortened;     /* reads of assigned units that lost bases and kept some                             */
    uint64_t reads_clipped_away;  /* reads of assigned units wholly outside the insert                                 */
    uint64_t bases_clipped;       /* bases taken off the reads of assigned units                                       */
    uint64_t amplicons;           /* amplicons in the caller's table                                                   */
    uint64_t amplicons_unused;    /* amplicons no unit was assigned to                                                 */
    float ms_assign;              /* device time of the assign step (k_amplicon_clip and its totals)                   */
    float ms_report;              /* device time of the rows' pass; 0 without amplicon_rows                            */
} qmcp_hip_amplicons_stats;
int qmcp_hip_solve_amplicons_host(qmcp_hip_ctx* ctx,
                                  const uint32_t* starts, const uint32_t* ends, const uint32_t* contig_ids,
                                  const uint32_t* seq_lengths, const uint32_t* qualities, uint64_t n_reads,
                                  const uint32_t* contig_lengths, uint32_t n_contigs, const uint32_t* amp_offsets,
                                  const uint32_t* amp_starts, const uint32_t* amp_ends,
                                  const uint32_t* amp_insert_starts, const uint32_t* amp_insert_ends,
                                  uint32_t min_length, uint32_t min_mapq, uint32_t max_coverage, uint32_t flags,
                                  uint64_t* keep_mask_out, uint32_t* amplicon_of_out, qmcp_hip_depth_row* amplicon_rows,
                                  qmcp_hip_stats* stats, qmcp_hip_amplicons_stats* astats);
int qmcp_hip_solve_amplicons_device(qmcp_hip_ctx* ctx,
                                    const uint32_t* d_starts, const uint32_t* d_ends, const uint32_t* d_contig_ids,
                                    const uint32_t* d_seq_lengths, const uint32_t* d_qualities, uint64_t n_reads,
                                    const uint32_t* contig_lengths, uint32_t n_contigs, const uint32_t* amp_offsets,
                                    const uint32_t* amp_starts, const uint32_t* amp_ends,
                                    const uint32_t* amp_insert_starts, const uint32_t* amp_insert_ends,
                                    uint32_t min_length, uint32_t min_mapq, uint32_t max_coverage, uint32_t flags,
                                    uint64_t* d_keep_mask_out, uint32_t* amplicon_of_out,
                                    qmcp_hip_depth_row* amplicon_rows, void* hip_stream, qmcp_hip_stats* stats,
                                    qmcp_hip_amplicons_stats* astats);

#ifdef __cplusplus
}
#endif
#endif /* QMCP_HIP_H */
