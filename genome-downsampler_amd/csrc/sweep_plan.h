// sweep_plan.h -- which sweep a call takes, decided on the host from the call's shape alone.
//
// Plain C++17 (no HIP): the solver's translation units include it, and so can a host-only test.  Everything a route
// decides before it launches its sweep lives here -- the form of the sweep, whether contigs are cut at cut points,
// whether stretch boundaries are speculated on and with how long a run-in -- as one plan function per route; the call
// sites (api/uniform_sweep.inc.hip, api/near_uniform_route.inc.hip, api/solve_tail.inc.hip) only execute the plan.
// The routes keep rules of their own where they differ (what "sparse" means, the run-in, the shortest genome worth
// stretches); those differences are named here, not aligned.  So do the layout of the stretch tables and the sizes of
// the sweeps' scratch, which the launchers and the arena both read.  The multi-device cost model (api/multi_device.inc.hip,
// mirrored by sharding.py) is here too, next to the predicate it prices.
#ifndef QMCP_SWEEP_PLAN_H
#define QMCP_SWEEP_PLAN_H
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "qmcp_hip.h"

namespace qmcp {

// ------------------------------------------------------------------ depths
// mean coverage / M below which the sweep runs every block in the general form (lab/sweep_lab.hip)
constexpr double kGenDepth = 11.0;  // lab, cycles per block fast / general: 674 / 542 at 9 x M, 595 / 545 at 10.5, 500 / 543 at 12

// Speculative stretch boundaries: below this mean coverage (in units of M), with a run-in (in blocks)
// that grows with the depth.  lab/spec_burn_study.py, cfg5's shape at 1/32 scale, boundaries that
// disagreed at a run-in of 128 / 256 / 512 / 1024 blocks: depth 2.0: 2 of 364 / 0 / 0 / 0; 2.5: 67 of 364 /
// 1 of 240 / 0 / 0; 3.0: 157 / 28 / 0 of 118 / 0; 4.0: 273 / 86 / 6 of 118 / 0 of 56 -- about twice
// the run-in per half unit of depth.  Two tiers: the first with the run-in of this table, and -- only
// if some boundary disagreed -- a second with three times that (or, where the genome is too short for it,
// none: the exact table); the exact sweep runs only if the second tier disagrees somewhere too.  Every
// tier's launches are queued at once and gated by device words, so nothing waits for the host.
// Round 3 (lab/spec_depth_gap.py, one contig of 20 M positions at 100 x coverage, profiles/r03_spec_depth_gap.log):
// between 4.1 and 11 x M -- where round 2 swept whole contigs as one chain each -- the sweep forgets its start too,
// within about a thousand blocks: boundaries that disagreed at a run-in of 256 / 512 / 1024 / 2048 blocks: depth 4.2:
// 55 of 127 / 2 of 63 / 0 of 31 / 0; 5.9: 85 / 11 / 0 / 0; 8.3: 100 / 20 / 0 / 0; 10: 108 / 23 / 1 of 31 / 0 of 15 --
// sweep 30.9 -> 1.3 ms.  So every depth the general-form sweep takes (below kGenDepth) is speculated on; at cfg4's
// depth (18.75, and at 37.5) every boundary still disagrees at 2 048 blocks (lab/spec_deep_probe.py): the event-driven
// chain stays whole there.
constexpr double kSpecDepth = kGenDepth, kSpecMinDepth = 1.3;

// Near-uniform route: mean coverage / M below which the route is not tried: the shallower the data, the more exceptions
// are wanted and the longer the runs of used-up buckets (cfg4's reads with 1 % clipped, lab/near_uniform_depths.py,
// near-uniform / mixed-span ms: 12.5 x M 2.9 / 105; 6.3 x M 6.0 / 401; 4.7 x M 5.5 / 503; 3.75 x M 6.4 / 659; with 40 %
// of the reads: 5 x M 12.4 / 579; 3 x M 15.7 / 710; 2.1 x M: gives up after four sweeps, 648 / 627 -- runs of used-up
// buckets with neither an anchor nor a cut point --; 1.5 x M 41.9 / 600, from cut points).  Below 1.3 x M nearly every
// window of the mixed-span sweep has a real cut point and that sweep is quick.
// Second half of round 4: the gate is the SIGMA depth (spec_sigma_depth: how far above M the coverage sits, as the depth at
// which M = 50 sits as far), and the crossover with the mixed-span walk -- which real cut points make quick where the
// coverage comes near M often -- was measured (lab/near_uniform_long_shallow.py, two contigs of 40 M positions, 1 % clipped,
// near-uniform / mixed-span ms by sigma depth): 1.24 (M = 20 at 1.4 x M) 18.9 / 7.3; 1.30 (30, 1.4) 23.4 / 10.0; 1.35 (20,
// 1.6) 14.1 / 7.9; 1.37 (10, 2.0) 8.9 / 5.6; 1.40 (50, 1.4) 24.1 / 17.3; 1.44 (30, 1.6) 15.9 / 13.7 | 1.56 (20, 2.0) 10.4 /
// 16.1; 1.60 (50, 1.6) 16.7 / 33.9; 1.67 (10, 3.0) 10.0 / 22.3; 1.72 (30, 2.0) 12.5 / 22.7 -- the route is tried from 1.5.
constexpr double kNuMinDepth = 1.5;
// ... and the depth below which its rounds sweep in stretches whatever the contigs' length (plan_near_uniform)
constexpr double kNuStretchDepth = 3.1;

// shortest span the event-driven sweep is used for: its scratch is 256 bytes per block, i.e. grows as
// the span shrinks; at 32 positions it is 8 bytes per position, what the bucket offsets themselves take
constexpr uint32_t ev_min_span() { return 32u; }

// ------------------------------------------------------------------ what the kernels take
// contigs + windows a stretch table holds (k_build_segments' LDS arrays; kernels/sweep_segments.inc.hip)
constexpr int kSegMaxCandidates = 4096;
// cut-point windows a route asks for: the one-span sweeps, and the tables' most (the mixed-span route)
constexpr uint32_t kSweepWindowsOneSpan = 768, kMaxSweepWindows = 3840;

// Cut-point segmentation: window count for a genome of ltot positions (0: not worth it).  Windows
// hold at least 64 blocks, so a stretch is long enough to amortise a pipeline start.
inline uint32_t sweep_segment_windows(uint32_t ltot, uint32_t ell, uint32_t n_contigs,
                                      uint32_t max_windows = kSweepWindowsOneSpan) {
    if (n_contigs >= 256 || ell == 0) return 0;
    const uint64_t w = (uint64_t)ltot / (64ull * ell);
    const uint32_t most = (uint32_t)kSegMaxCandidates - 256;
    const uint32_t cap = max_windows < most ? max_windows : most;
    return (uint32_t)(w < 2 ? 0 : (w > cap ? cap : w));
}
// seven-wave pipelined forms (spans <= 256); false if the span needs the single-wave kernel
inline bool sweep_uniform_mw_supported(uint32_t ell) { return ell >= 1 && (ell + 63) / 64 <= 4; }
// event-driven form (deep data): a block word holds E = ceil(ell / 64) fields of 30 / E bits, the top one a guard;
// the field maximum EvPack<E>::kSat (kernels/sweep_uniform_events.inc.hip)
constexpr uint64_t ev_pack_sat(uint32_t e) { return (1ull << (30 / e - 1)) - 1; }
// M must leave room in a field: no kept count can reach a saturated field's value
inline bool sweep_uniform_ev_supported(uint32_t ell, uint32_t M) {
    if (!sweep_uniform_mw_supported(ell)) return false;
    return (uint64_t)M + 1 <= ev_pack_sat((ell + 63) / 64);
}

// ------------------------------------------------------------------ the sweeps' tables and scratch
// A call's stretch tables (`seg_words`, k_build_segments writes them): the windows' cuts, then three tables -- tier 0, the
// exact one, and tiers 1 and 2 with speculative boundaries --, each a count and per stretch {start, end, contig end}, the
// owned-from position and the exact table's stretch it lies in.  Where a tier's table begins, and the words of all three:
inline size_t sweep_segment_table_offset(uint32_t n_contigs, uint32_t n_windows, uint32_t tier) {
    return (size_t)n_windows + (size_t)tier * (1 + 5 * ((size_t)n_contigs + n_windows));
}
inline size_t sweep_segment_words(uint32_t n_contigs, uint32_t n_windows) {
    return sweep_segment_table_offset(n_contigs, n_windows, 3);
}
// The event-driven form's scratch (kernels/sweep_uniform_events.inc.hip) for n_wg workgroups: pieces of four blocks, 1 KiB
// each packed; the chain's state at every 64th block; the last changed block per block.
inline uint32_t sweep_ev_pieces(uint32_t ltot, uint32_t ell, uint32_t n_wg) { return ltot / (4u * ell) + n_wg + 1; }
inline size_t sweep_ev_pack_bytes(uint32_t ltot, uint32_t ell, uint32_t n_wg) {
    return (size_t)sweep_ev_pieces(ltot, ell, n_wg) * 1024;
}
inline size_t sweep_ev_ckpt_bytes(uint32_t ltot, uint32_t ell, uint32_t n_wg) {
    return ((size_t)sweep_ev_pieces(ltot, ell, n_wg) / 16 + 2 * (size_t)n_wg + 4) * 512 * sizeof(uint32_t);
}
inline size_t sweep_ev_last_bytes(uint32_t ltot, uint32_t ell, uint32_t n_wg) {
    return ((size_t)sweep_ev_pieces(ltot, ell, n_wg) * 4 + 64) * sizeof(uint32_t);
}
// the most workgroups an event-driven sweep gets: a stretch per contig and per cut-point window of the one-span routes
inline uint32_t sweep_ev_workgroups_max(uint32_t n_contigs) { return n_contigs + kSweepWindowsOneSpan; }
// the mixed-span walk's state at a speculative boundary (>= the register sweep's window of live buckets), per stretch
constexpr uint32_t kSpecSnapWords = 512;
inline size_t spec_snap_bytes(uint32_t n_cand) { return (size_t)n_cand * kSpecSnapWords * sizeof(uint32_t); }

// ------------------------------------------------------------------ speculation
inline uint32_t spec_burn_blocks(double depth) {
    return depth < 2.1 ? 320u : depth < 2.6 ? 640u : depth < 3.1 ? 1152u : depth < 4.1 ? 2304u : 1536u;
}
// The table above was measured at M = 50.  What makes a sweep forget its start is how often the coverage comes near M --
// how many standard deviations above M it sits: z = (mean coverage - M) / sqrt(mean coverage) = sqrt(M) (d - 1) / sqrt(d)
// for Poisson starts at depth d x M.  This is the depth at which M = 50 has the same z; the run-in is looked up at the
// larger of the two (a smaller M keeps the table's value: measured over-provisioned, not under).  Second half of round 4,
// lab/spec_run_in_vs_M.py, one contig of 60 M positions, one read length, boundaries that disagreed / sweep ms at the
// table's run-in and at the corrected one: M = 100 at 2 x M: 12 of 255 / 1.98 -> (1 152 blocks) none; M = 100 at 3 x M:
// 16 of 85 / 5.75 -> 4 of 63 / 7.5; **M = 200 at 2 x M: 161 of 255, the second tier failing too: the exact sweep, 94 ms ->
// (2 304 blocks) ~10 ms**.
// spec_sigma_depth is that depth itself -- below the raw depth where M < 50; spec_depth_in_sigma the larger of the two,
// never below the raw depth.
inline double spec_sigma_depth(double depth, uint32_t M) {
    if (!(depth > 1.0)) return depth;
    const double y = std::sqrt((double)M / 50.0) * (depth - 1.0) / std::sqrt(depth);
    const double x = 0.5 * (y + std::sqrt(y * y + 4.0));
    return x * x;
}
inline double spec_depth_in_sigma(double depth, uint32_t M) {
    const double d_eff = spec_sigma_depth(depth, M);
    return d_eff > depth ? d_eff : depth;
}
inline bool spec_wanted(const qmcp_hip_options& opt, double depth, double depth_lo = -1.0 /* what the lower bound looks at:
                        the sigma depth where it is larger -- "nearly every window has a real cut point" below 1.3 x M holds
                        for M = 50, not for M = 400, whose 1.2 x M is as far above M in standard deviations as M = 50 at
                        1.67 x M */) {
    if (depth_lo < 0.0) depth_lo = depth;
    bool on = depth < kSpecDepth && depth_lo > kSpecMinDepth;  // (shallower: nearly every window has a real cut point)
    if (opt.speculation != 0) on = opt.speculation > 0;        // (never / at any depth)
    return on;
}
inline uint32_t spec_first_run_in(const qmcp_hip_options& opt, double depth) {
    return opt.speculation_run_in ? opt.speculation_run_in : spec_burn_blocks(depth);
}
// Cut-point segmentation of the sweeps (QMCP_HIP_CUTS=0|1 overrides): looked for where mean coverage is a small multiple
// of M -- deep data has no cut points, and the look costs two launches.
inline uint32_t sweep_cut_windows(const qmcp_hip_options& opt, uint32_t ltot, uint32_t span, uint32_t n_contigs, bool shallow,
                                  uint32_t max_windows = kSweepWindowsOneSpan) {
    bool on = shallow;
    if (opt.cut_points != 0) on = opt.cut_points > 0;
    return on ? sweep_segment_windows(ltot, span, n_contigs, max_windows) : 0u;
}

// mean coverage in units of M, counted with the span given (a mix of spans: the longest, an upper bound)
inline double sweep_depth(uint32_t n, uint32_t span, uint32_t ltot, uint32_t M) {
    return (double)n * (double)span / ((double)ltot * (double)(M ? M : 1));
}
// Many times M and yet SPARSE (a small M: depth 12 x M with M = 10 is 0.8 reads a position): more than half of the blocks
// hold a position without a read, so the event-driven form is out and the fast form's check fails nearly everywhere
// (~1 130 cycles a block measured); and in standard deviations such data is shallow -- it forgets as M = 50 at 3.7 x M
// does.  The general pipeline in speculative stretches, then, as below 11 x M (second half of round 4, lab/cliff_hunt.py:
// one contig of 82.6 M positions, 66 M reads of one length, M = 10: 259 ms as one chain).  Such a call is judged by its
// sigma depth: true where the depth is kGenDepth or more, the data sparse and the sigma depth below kGenDepth.
inline bool sparse_deep(double depth, bool sparse, uint32_t M) {
    return depth >= kGenDepth && sparse && spec_sigma_depth(depth, M) < kGenDepth;
}
// "Sparse" on the routes that do not count empty positions (near-uniform, mixed span): fewer reads a position than
// ln(span / ln 2), where with Poisson starts more than half of the blocks of `span` positions hold an empty one.
inline bool sparse_by_reads(uint32_t n, uint32_t ltot, uint32_t span) {
    return (double)n / (double)ltot < std::log((double)span / 0.693);
}
// The upper bound of the speculation, in standard deviations too where that is the larger (lab/spec_run_in_large_M.py, one
// contig of 20 M positions: M = 400 at 3 x M and M = 200 at 4 x M, sigma depths 12.6 and 11.5, do not forget within the
// contig at any run-in up to 9 216 blocks: 42 ms with the tiers against 35 as one chain; M = 400 at 2 x M, 5.4: 10.5
// against 34) -- a sigma depth beyond the raw one counts a little more: 10.9 (M = 200 at 4 x M) behaves as 11.5 and 12.6
// do.  Sparse deep data is judged by its sigma depth alone.
inline double spec_upper_depth(double depth, bool sparse_deep_, uint32_t M) {
    if (sparse_deep_) return spec_sigma_depth(depth, M);
    const double sig = spec_depth_in_sigma(depth, M);
    return sig > depth ? sig * (kSpecDepth / 9.0) : depth;
}
// the first tier's run-in of the one-length sweeps: the table's at the depth in sigma; sparse and many times M, three times
// that (lab/sparse_deep_run_ins.py, boundaries that disagreed, first / second tier, and sweep ms at 1 536 and at 4 608
// blocks: M = 10 at 20 x M: 17 of 21 / 0, 7.2 -> 0 of 7, 5.4; M = 10 at 12 x M: 7 of 42 / 0, 7.3 -> 0 of 14, 5.5; M = 20
// at 15 x M: 31 of 31 / 7 -- the exact sweep --, 53 -> 7 of 10 / 0, 21)
inline uint32_t spec_one_length_run_in(const qmcp_hip_options& opt, double depth, bool sparse_deep_, uint32_t M) {
    return spec_first_run_in(opt, spec_depth_in_sigma(depth, M)) * ((sparse_deep_ && !opt.speculation_run_in) ? 3u : 1u);
}

// ------------------------------------------------------------------ the one-span route (launch_uniform_sweep)
// The uniform-span sweep: seven waves per contig where the span allows it (fast form with checked fallback on deep data,
// every block in the general form on shallow data -- both exact, the choice is about speed only), else the single-wave
// kernel; on deep data the event-driven form.  QMCP_HIP_SWEEP=fast|gen|ev overrides.
enum class UniformForm { Events, SpeculativeGeneral, General, Fast, SingleWave };
struct UniformSweepPlan {
    UniformForm form;
    uint32_t windows;      // cut-point windows to look in (0: whole contigs)
    bool speculate;        // windows without a cut get a speculative boundary (form SpeculativeGeneral)
    uint32_t burn_blocks;  // the first tier's run-in, in blocks
    // the tiers (speculative_sweep): a block is `unit` positions, run-ins are rounded to `round_to` positions, candidate
    // boundaries are `run_ins_apart` run-ins apart, and a genome shorter than `min_run_ins` run-ins is not speculated on
    uint32_t unit, round_to;
    static constexpr uint32_t run_ins_apart = 4, min_run_ins = 8;
};
// empty_positions: start positions that hold no read (0xFFFFFFFF: unknown -- the small-call route)
inline UniformSweepPlan plan_uniform_sweep(const qmcp_hip_options& opt, uint32_t n, uint32_t span, uint32_t ltot,
                                           uint32_t n_contigs, uint32_t M, uint32_t empty_positions) {
    UniformSweepPlan p{};
    p.unit = p.round_to = span;
    // the fast form needs the binding jumps to come from the previous block, which holds while coverage is many times M
    const double depth = sweep_depth(n, span, ltot, M);
    // Sparse: counted from the empty positions.  With a fraction z of them about 1 - (1 - z)^span of the blocks have one:
    // more than half of them from z = ln 2 / span on.  (No read can start in the last span - 1 positions of a contig:
    // those are not holes in the data.)
    const double structural = (double)n_contigs * (double)(span - 1);
    const double holes = (double)empty_positions > structural ? (double)empty_positions - structural : 0.0;
    const bool known = empty_positions != 0xFFFFFFFFu;
    const bool gapped = holes * (double)span > 0.693 * (double)ltot;
    bool gen = depth < kGenDepth;
    const bool sigma_gated = !gen && sparse_deep(depth, known && gapped, M);
    if (sigma_gated) gen = true;
    if (opt.sweep == QMCP_SWEEP_GENERAL) gen = true;
    if (opt.sweep == QMCP_SWEEP_FAST) gen = false;
    // shallow or gapped data: split the contigs at cut points so that more than n_contigs chains run
    p.windows = sweep_cut_windows(opt, ltot, span, n_contigs, gen);
    // Data a few times deeper than M: hardly any cut points, but the sweep forgets its start within tens of blocks
    // (kernels/sweep_segments.inc.hip), so windows without a cut get a speculative boundary with a run-in (every few
    // windows, so that stretches stay several run-ins long); the stretches' outputs are compared where they meet, and if
    // any pair disagrees the exact sweep runs after all (its launch is there either way and returns at once when all
    // agreed).
    p.burn_blocks = spec_one_length_run_in(opt, depth, sigma_gated, M);
    const double depth_gate = sigma_gated ? spec_sigma_depth(depth, M) : depth;
    p.speculate = spec_wanted(opt, spec_upper_depth(depth, sigma_gated, M), spec_depth_in_sigma(depth_gate, M)) && gen &&
                  p.windows != 0 && sweep_uniform_mw_supported(span) && p.burn_blocks >= 2 &&
                  (uint64_t)ltot >= (uint64_t)p.min_run_ins * p.burn_blocks * span;
    // deep data: the event-driven form (a block is only TESTED unless its counts fall below the kept profile); spans below
    // ev_min_span() would need more scratch than the arena holds for it ... and only where few blocks have a start
    // position that holds no read: such a block nearly always changes the kept profile, and a changed block costs the
    // event-driven chain ~6 x the block-scan pipeline's chain step (amplicon panels, whose reads start in a few windows:
    // cfg3 took 0.16 ms against 0.05).  (Unknown on the small-call route: block scan, as in round 1.)
    const bool spiky = !known || gapped;
    bool ev = !gen && !spiky && span >= ev_min_span();
    if (opt.sweep == QMCP_SWEEP_EVENTS) ev = span >= ev_min_span();
    if (opt.sweep == QMCP_SWEEP_FAST || opt.sweep == QMCP_SWEEP_GENERAL) ev = false;
    if (ev && sweep_uniform_ev_supported(span, M)) p.form = UniformForm::Events;
    else if (p.speculate) p.form = UniformForm::SpeculativeGeneral;
    else if (!sweep_uniform_mw_supported(span)) p.form = UniformForm::SingleWave;
    else p.form = gen ? UniformForm::General : UniformForm::Fast;
    return p;
}

// ------------------------------------------------------------------ the near-uniform route (near_uniform_tail)
// Which sweep the rounds run.  Deeper than 11 x M: one chain per contig in the event-driven form -- what the one-span
// route runs there too -- restarted from its checkpoints.  Shallower (round 4): the block-scan pipeline in STRETCHES,
// as the one-span route does -- real cut points (coverage of ALL reads <= M: every read over them is kept in every
// round, whatever has been selected) and speculative boundaries checked on the device -- with the need moved by nadj;
// every round sweeps everything (hundreds of short chains side by side: a whole chain per contig was 7 ms a sweep for
// cfg4's 10^6 positions at 1.5 x M, and long shallow contigs did not take the route).
// Between 3.1 and 11 x M contigs of up to 2 M positions keep the chain: the speculative run-ins there are 1 536 - 2 304
// blocks, as long as such a contig, and the chain changes fewer blocks the deeper the data (lab/near_uniform_depths.py,
// cfg4's reads with 1 % clipped, chain / stretches ms: 6.3 x M 6.0 / 13.1; 4.7 x M 5.5 / 13.2; 3.75 x M 6.4 / 11.5;
// with 40 % of the reads: 5 x M 12.4 / 15.3; 3 x M 15.7 / 11.2; 2.1 x M gives up / 14.2; 1.5 x M 41.9 / 8.6).
struct NearUniformPlan {
    bool tried;            // false: the route is not tried (QMCP_NU_GIVEUP_NOT_TRIED), nothing below is set
    bool stretches;        // the block-scan pipeline, in stretches where windows != 0; false: the event-driven chain
    bool speculate;        // speculative boundaries in the stretches
    uint32_t burn_blocks;  // the first tier's run-in, in blocks
    uint32_t windows;      // cut-point windows (stretches only)
    double depth;          // mean coverage in units of M (for the route's debug line)
};
// ell: the longest (dominant) span; longest: the longest contig; may_rank: the call takes the range-ranked route
inline NearUniformPlan plan_near_uniform(const qmcp_hip_options& opt, uint32_t n, uint32_t ell, uint32_t min_span,
                                         uint32_t ltot, uint32_t n_contigs, uint32_t longest, uint32_t M, bool may_rank) {
    NearUniformPlan p{};
    p.depth = sweep_depth(n, ell, ltot, M);
    const double depth = p.depth;
    double min_depth = kNuMinDepth;
    if (opt.near_uniform_min_depth > 0.f) min_depth = opt.near_uniform_min_depth;  // (lab)
    // (the sigma depth where it is larger: M = 400 at 1.2 x M has as few cut points as M = 50 at 1.67 x M -- and the mixed-span
    //  walk it was left to took 233 ms for 11.9 M reads on 3.7 M positions, 200 x the one-length solve: lab/cliff_hunt.py)
    if (!may_rank || spec_sigma_depth(depth, M) < min_depth || min_span == 0) return p;
    // (the event-driven form's own limits: scratch for short spans, M in a packed field)
    const bool ev_ok = ell >= ev_min_span() && sweep_uniform_ev_supported(ell, M);
    // (many times M and yet sparse -- a small M: more than half of the blocks hold a position without a read, the chain
    //  would run its general step on nearly every block -- is shallow in standard deviations: stretches, as on the one-span
    //  route.  66 M reads on one contig of 82.6 M positions at 12 x M with M = 10, 1 % clipped: 3.2 s in chains.)
    const bool sparse = sparse_by_reads(n, ltot, ell);
    const bool sigma_gated = sparse_deep(depth, sparse, M);
    const double depth_gate = sigma_gated ? spec_sigma_depth(depth, M) : depth;
    const bool mw_ok = sweep_uniform_mw_supported(ell);
    // (sparse data -- more than half of the blocks hold a position without a read -- makes the chain run its general step on
    //  nearly every block: 551 k reads on 1 M positions at 4 x M with M = 20, 1 % clipped: 36.7 ms in chains, lab/cliff_hunt.py)
    bool stretches = depth_gate < kGenDepth && mw_ok && (depth_gate < kNuStretchDepth || longest > 2000000u || !ev_ok || sparse);
    // (deep data whose M does not fit a packed field of the event-driven form -- M = 200 at reads of 250 --: the block-scan
    //  pipeline, one chain per contig, every round a whole sweep; contigs of up to 2 M positions -- 99.7 M reads on 24
    //  contigs at 12 x M were 112 ms on the mixed-span walk against 2.7 with one length, lab/cliff_hunt.py)
    if (depth_gate >= kGenDepth && !ev_ok && mw_ok && longest <= 2000000u) stretches = true;
    if (opt.sweep == QMCP_SWEEP_EVENTS) stretches = false;
    if (opt.sweep == QMCP_SWEEP_GENERAL) stretches = mw_ok;
    if (!stretches) {
        if (!ev_ok) return p;
        if (depth_gate < kGenDepth && longest > 2000000u) return p;  // (spans the pipeline does not take: a whole chain per round)
    }
    p.tried = true;
    p.stretches = stretches;
    p.burn_blocks = spec_one_length_run_in(opt, depth, sigma_gated, M);
    if (stretches) {
        p.windows = sweep_cut_windows(opt, ltot, ell, n_contigs, true);
        p.speculate = spec_wanted(opt, spec_upper_depth(depth, sigma_gated, M), spec_depth_in_sigma(depth_gate, M)) &&
                      p.windows != 0 && p.burn_blocks >= 2 && (uint64_t)ltot >= 8ull * p.burn_blocks * ell;
    }
    return p;
}

// ------------------------------------------------------------------ the mixed-span route (solve_tail)
// Shallow or gapped data: stretches between cut points, one wave each (depth judged with the longest span: an upper
// bound); a mixed-span walk is one light workgroup per stretch and slow per position: five times the windows the one-span
// sweeps get, whose seven-wave workgroups fill the chip at three per compute unit.  Speculative stretch boundaries as for
// one span: the state is the selected reads still alive, i.e. the kept counts of the last max_span start positions,
// which k_spec_verify compares (selend = bucket start + kept count); the run-in is counted in windows of max_span
// positions.  Two phases: the plan, and -- where it asks for a sample of the spans -- its refinement by that sample.
struct MixedSweepPlan {
    uint32_t windows;       // cut-point windows (0: one wave per contig)
    bool sample_span_mode;  // read a sample of the spans (launch_span_mode_share), then refine_mixed_with_span_sample
    bool speculate;         // speculative boundaries (the register-resident walk)
    uint32_t burn_blocks;   // the first tier's run-in, in blocks of max_span positions
    // the tiers (speculative_sweep): run-ins rounded to 64 positions, candidates two run-ins apart (a walk is one light
    // workgroup: many short stretches beat few long ones), no speculation on a genome shorter than four run-ins
    static constexpr uint32_t round_to = 64, run_ins_apart = 2, min_run_ins = 4;
    // what the refinement reads
    double depth;
    bool sigma_gated, in_regs, hopeless;
    uint32_t max_span, ltot, M;
};
inline void finish_mixed_plan(const qmcp_hip_options& opt, MixedSweepPlan& p) {
    if (opt.speculation != 0 || opt.speculation_run_in != 0) p.hopeless = false;
    const double depth_gate = p.sigma_gated ? spec_sigma_depth(p.depth, p.M) : p.depth;
    p.speculate = !p.hopeless && spec_wanted(opt, depth_gate, spec_depth_in_sigma(depth_gate, p.M)) && p.in_regs &&
                  p.windows != 0 && p.burn_blocks >= 2 && (uint64_t)p.ltot >= (uint64_t)p.min_run_ins * p.burn_blocks * p.max_span;
}
// in_regs: the register-resident walk (spans up to 448) runs; remembered_hopeless: a solve of this shape speculated in vain
inline MixedSweepPlan plan_mixed_sweep(const qmcp_hip_options& opt, uint32_t n, uint32_t max_span, uint32_t ltot,
                                       uint32_t n_contigs, uint32_t M, bool in_regs, bool remembered_hopeless) {
    MixedSweepPlan p{};
    p.max_span = max_span; p.ltot = ltot; p.M = M; p.in_regs = in_regs;
    p.depth = sweep_depth(n, max_span, ltot, M);
    // (many times M and yet sparse -- a small M -- is shallow in standard deviations, as on the one-span route)
    p.sigma_gated = sparse_deep(p.depth, sparse_by_reads(n, ltot, max_span), M);
    const double depth_gate = p.sigma_gated ? spec_sigma_depth(p.depth, M) : p.depth;
    p.windows = sweep_cut_windows(opt, ltot, max_span, n_contigs, depth_gate < kGenDepth, kMaxSweepWindows);
    // (the first tier starts lower than for one span: a walk is slow per position, so short stretches matter more, and the
    //  second tier is there)
    p.burn_blocks = opt.speculation_run_in ? spec_first_run_in(opt, p.depth) : spec_first_run_in(opt, p.depth) * 3u / 5u;
    p.hopeless = remembered_hopeless;
    // One dominant read length (what is left for this route once the shorter reads have their own: a few LONGER ones)
    // forgets its state as slowly as one-length data, and the walk's boundaries then disagree nearly everywhere
    // (lab/mixed_spec_check.py: 430 against 185 ms at 7.5 x M); a broad mix of lengths forgets fast and gains
    // (lab/mixed_spec_broad.py: 117 against 271 ms at 5 x M).  A sample of the spans tells the two apart before anything
    // is queued.
    p.sample_span_mode = !p.hopeless && spec_wanted(opt, depth_gate, spec_depth_in_sigma(depth_gate, M)) && in_regs &&
                         p.windows != 0 && n >= (1u << 20);
    finish_mixed_plan(opt, p);
    return p;
}
// share: the sample's size, how many of it have its most common span, and that span; longest: the longest contig
inline MixedSweepPlan refine_mixed_with_span_sample(const qmcp_hip_options& opt, MixedSweepPlan p, const uint32_t share[3],
                                                    uint32_t longest) {
    if (share[0] != 0 && (uint64_t)share[1] * 10u >= (uint64_t)share[0] * 9u) {
        // Second half of round 4: that finding was about how DEEP the data is in standard deviations, not about the one
        // length.  The run-in table (spec_burn_blocks) was measured at M = 50; what makes a sweep forget is how often the
        // coverage comes near M, i.e. z = (mean coverage - M) / sqrt(mean coverage) = sqrt(M) (d - 1) / sqrt(d) for Poisson
        // starts -- the lab's reads at 2.1 x M with M = 350 are as deep as M = 50 at 6 x M, and their boundaries disagreed at
        // the run-in of 2.1 x M.  So: the depth at which M = 50 has the same z; below 3.1 of it the walk speculates with that
        // depth's whole run-in (not three fifths: a boundary that disagrees costs its exact stretch again, and on such data
        // exact stretches are long), deeper it does not.  One GPU's real share of configs[4] (117.7 M positions in its
        // longest contig, 2 x M, M = 50) with 1 % clipped reads, this route: 14.5 s as one chain per contig, 52 ms in 1 925
        // stretches, no boundary disagreeing (lab/cfg5_share_mixed_spec.py) -- which is what a whole-genome BAM with reads
        // LONGER than the dominant length (deletions) gets, since those leave the near-uniform route.
        // (the call's depth is counted with the LONGEST span; nine tenths of the reads have this one)
        const double depth_mode = share[2] >= 1 && share[2] < 511 && share[2] < p.max_span
                                      ? p.depth * (double)share[2] / (double)p.max_span : p.depth;
        const double depth_eff = p.sigma_gated ? spec_sigma_depth(depth_mode, p.M)     // (a small M: shallower than its depth)
                                               : spec_depth_in_sigma(depth_mode, p.M);  // (>= its argument)
        p.hopeless = !(depth_eff < 3.1);
        // deeper than that (run-ins of 1 536 blocks and more) only where the longest contig holds a dozen run-ins: a
        // 10^6-position contig would become two stretches, a chromosome becomes hundreds
        if (p.hopeless && depth_eff < kSpecDepth)
            p.hopeless = (uint64_t)longest < 12ull * spec_first_run_in(opt, depth_eff) * p.max_span;
        if (!p.hopeless)
            p.burn_blocks = spec_first_run_in(opt, p.sigma_gated ? p.depth : depth_eff) *
                            ((p.sigma_gated && !opt.speculation_run_in) ? 3u : 1u);
    }
    finish_mixed_plan(opt, p);
    return p;
}

// ------------------------------------------------------------------ several devices (api/multi_device.inc.hip)
// cost model of a device's share (measured; the same numbers as
// genome-downsampler_amd/sharding.py): per read for the bandwidth-bound stages, per position of the
// LONGEST contig for the sweep (a device's chains run side by side)
constexpr double kNsPerRead = 0.008, kNsPerPosition = 1.5, kNsPerPositionStretches = 0.012;

// (sharding.py: share_sweeps_as_stretches / share_cost) a share's sweep is cut into stretches exactly when the
// solver would cut it: the AGGREGATE depth of everything the device owns (plan_uniform_sweep; neither its sparse gate
// nor the sigma upper bound is modelled)
inline bool share_sweeps_as_stretches(double reads, double positions, size_t n_contigs, uint32_t span, uint32_t M) {
    if (span == 0 || M == 0 || positions <= 0 || n_contigs >= 256) return false;
    const double depth = reads * (double)span / (positions * (double)M);
    if (depth <= kSpecMinDepth) return positions >= 128.0 * (double)span;  // nearly every window has a real cut
    return depth < kSpecDepth && positions >= 8.0 * (double)spec_burn_blocks(spec_depth_in_sigma(depth, M)) * (double)span;
}
inline double share_cost(double reads, double positions, double longest, size_t n_contigs, uint32_t span, uint32_t M) {
    if (share_sweeps_as_stretches(reads, positions, n_contigs, span, M))
        return kNsPerRead * reads + kNsPerPositionStretches * positions;
    return kNsPerRead * reads + kNsPerPosition * longest;
}

}  // namespace qmcp
#endif
