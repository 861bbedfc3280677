// qmcp_api.hip -- context, device arena and stage orchestration behind include/qmcp_hip.h.
//
// Stage order of one solve (all on the context's stream):
//   prepare   validate, span min/max, global start keys, reads-per-start counts
//   scan      exclusive scan of the counts -> bucket offsets boff (and eoff on the mixed path)
//   sort      LSD radix bucketing of read indices by (start[, span desc]), stable in index
//   sweep     selection: block-parallel shortest-path sweep (uniform span) or the
//             event-driven priority sweep (mixed spans); one wave per contig
//   mark      keep bitmask from per-bucket selected prefixes
// One host round trip (12 bytes) after `prepare` picks the path and the radix width.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "qmcp_hip.h"
#include "qmcp_kernels.h"
#include "by_contig_plan.h"
#include "ladder_plan.h"
#include "budget_plan.h"
#include "stratified_plan.h"
#include "tiers_plan.h"
#include "dedup_plan.h"
#include "amplicon_table.h"
#include "amplicon_assign.h"
#include "target_table.h"
#include "cap_table.h"
#include "pair_plan.h"
#include "replicates_plan.h"
#include "fragment_plan.h"
#include "solve_words.h"

// One translation unit, kept in parts under api/ (included below, in dependency order: a part uses only parts above it,
// those a by-contig feature builds on are named in brackets):
//   context             the solver context and the types that own its device arena, pinned blocks, events and streams
//                       (deleting the context frees them all), ensure / ensure_pinned, typed buffer access, the event
//                       pool and timing spans, problem checks, small stage helpers (the rank of a mask's bits)
//   radix_passes        the stable LSD radix sort's passes (records form, wide u64 form): the one loop every sorting entry queues
//   uniform_sweep       which one-length sweep a call takes and its launches (pipelines, event-driven form, stretches,
//                       speculative tiers)
//   near_uniform_sizes  the near-uniform route's sizes, round budget and buffers
//   solve_stages        the stages the sort-based routes share (plain solve and capped solve): keys, sort, bucket offsets,
//                       run lengths, rings, mark, the result scalars, phase times
//   solve_head          a solve's head: arena sizing, the range-ranked route's producers, bucket offsets; the pass-major
//                       ranking
//   near_uniform_route  the near-uniform route's half of a solve's tail
//   solve_tail          a solve's tail -- read the head's facts, pick the route, one function per route --, collection,
//                       context creation, enqueue / complete
//   host_entries        probes, column upload, the extern "C" entry points
//   multi_device        several devices behind one call
//   by_contig           reads in any order with a contig id each: the grouping as a value, a batch's view, the batch loop
//                       over a batch solver, the mask scattered back; the by-contig entries.  Knows no feature built on it
//   amplicon_by_contig  pairs of several contigs: FILTER against each contig's amplicons, compaction, the by-contig solve
//   quality             the plain or by-contig solve, then the quality pass on its mask (same count per cell, best reads)
//   targets             coverage capped inside target regions only: reads projected onto each contig's target positions,
//                       the by-contig solve (and quality pass) of the projected on-target reads, the mask expanded back
//   depth_report        depth before and after a keep mask, per contig and per region, with histograms: position batches,
//                       the reads' events, the positions pass, rows and statistics assembled on the host
//   depth_track         the same pipeline ending in a run-length compaction: per-base depth before and after as records
//                       (contig, start, end, depth_in, depth_kept, short), counted first, then written and copied out
//   ladder              (by_contig) several falling coverages in one call: a batch solver whose further levels run after
//                       each batch, on the reads the level above kept; one byte per read counts the levels that keep it
//   stratified          (by_contig) one coverage cap per stratum (strand, read group, sample): reads grouped once by
//                       (stratum, contig), every stratum solved in batches of its own at its cap, one row of counts each
//   dedup               duplicate families (reads or pairs with equal cells) collapsed to their best unit before the
//                       by-contig solve; duplicate mask, family-size histogram and statistics from the device
//   profile             (by_contig) one cap per region (a piecewise-constant cap along every contig): the cap table, the
//                       capped route (the sort-based mixed route under a need[] built on the device) and the batch solver
//                       with need(p) = min(cov(p), cap(p))
//   pairs               (by_contig, profile) pair-aware downsampling: the batch loop at a first target, then stages over
//                       all batches that credit the depth of the pairs already kept and top up among the other reads on
//                       the capped route
//   tiers               (by_contig, profile) tiered downsampling: reads grouped once by (tier, contig), tier 0 solved plainly
//                       at M, every later tier on the capped route under need = min(its coverage, M - the depth of the
//                       earlier tiers' kept reads), which a list of the kept reads carries from batch to batch
//   templates           (pairs) the pair-aware stages with the unit generalised: every segment that carries one template
//                       id (single-end reads, pairs, split reads, spliced blocks), completed through a bitset of ids
//   templates_profile   (templates, profile) the template stages under a cap per region: stage 1 is the profile's batch
//                       solver at the scaled caps, later stages build need[] from the scaled region table and the credit
//   fragments           (templates) fragment depth: the segments of a template clipped where they overlap (validation, the
//                       sort by template, contig and start, a segmented running maximum, the columns written back), as an
//                       entry of its own and in front of the template stages
//   ceiling             (profile) kept depth never above the cap, the most reads kept: a batch solver with the dual need
//                       max(0, cov(p) - cap(p)) selecting the DROPPED reads, a device-side check, and the complement
//   proportional        (profile) a fraction of the depth everywhere: a batch solver with need(p) = min(cov(p), M,
//                       max(ceil(cov(p) * num / den), floor)) built from the batch's own depth, the plain by-contig call at
//                       both ends of the fraction's range, and a tally of the kept bases
//   budget              (by_contig) the deepest coverage whose by-contig solve fits a number of reads: one grouping, the
//                       curve S(M) from a device-side depth histogram, and a few whole solves picked by budget_plan.h
//   mean_depth          (budget) the deepest coverage whose by-contig solve fits a number of bases inside a region set: the
//                       budget's flow with the histogram restricted to the regions and a weighted count per probe
//   thresholds          (by_contig) every read's smallest keeping coverage in a range: one grouping, one whole solve per
//                       coverage folded into the thresholds by thresholds_plan.h's word logic, the counts per coverage
//   start_cap           (dedup, depth_report) every (contig, start, group) cell reduced to its best K reads before the
//                       by-contig solve; capped mask, cell-size histogram, the cells the kept set uses, and the shortfall
//                       against the demand of all placed reads through the depth report's pass
//   replicates          (by_contig, depth_report) one read set split into disjoint downsamples: the batch loop at the
//                       first coverage, every further replicate solved on the reads still free, replicate-major over the
//                       one grouping's batches
//   amplicon_clip       (amplicon_by_contig, dedup, depth_report) every unit assigned to one amplicon of its contig and
//                       clipped to its insert: the assign pass, compaction, the by-contig solve pooled or per amplicon,
//                       mates, the mask expanded back, and one depth row per amplicon through the depth report's pass
#include "api/context.inc.hip"
#include "api/radix_passes.inc.hip"
#include "api/uniform_sweep.inc.hip"
#include "api/near_uniform_sizes.inc.hip"
#include "api/solve_stages.inc.hip"
#include "api/solve_head.inc.hip"
#include "api/near_uniform_route.inc.hip"
#include "api/solve_tail.inc.hip"
#include "api/host_entries.inc.hip"
#include "api/multi_device.inc.hip"
#include "api/by_contig.inc.hip"
#include "api/amplicon_by_contig.inc.hip"
#include "api/quality.inc.hip"
#include "api/targets.inc.hip"
#include "api/depth_report.inc.hip"
#include "api/depth_track.inc.hip"
#include "api/ladder.inc.hip"
#include "api/stratified.inc.hip"
#include "api/dedup.inc.hip"
#include "api/profile.inc.hip"
#include "api/pairs.inc.hip"
#include "api/tiers.inc.hip"
#include "api/templates.inc.hip"
#include "api/templates_profile.inc.hip"
#include "api/fragments.inc.hip"
#include "api/ceiling.inc.hip"
#include "api/proportional.inc.hip"
#include "api/cap_search.inc.hip"
#include "api/budget.inc.hip"
#include "api/mean_depth.inc.hip"
#include "api/thresholds.inc.hip"
#include "api/replicates.inc.hip"
#include "api/start_cap.inc.hip"
#include "api/amplicon_clip.inc.hip"
