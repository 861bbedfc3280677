// qmcp_kernels.hip -- gfx950 (MI355X, CDNA4) kernels of the quasi-MCP solver path.
//
// Everything here is integer scatter / scan / selection: HBM- or latency-bound, no MFMA.
// wave = 64 lanes throughout.  The path these kernels replace is the reference's
//   coverage build        quasi_mcp_cpu_max_flow_solver.cpp:58-73 (O(N*len) per-base loop)
//   max-flow + readout    quasi_mcp_cpu_max_flow_solver.cpp:19-20,89-100
//   (CUDA equivalent      quasi_mcp_cuda_max_flow_solver.cu:12-79,319-435)
// with the canonical selection rule stated in oracle/qmcp_oracle.c.
//
// Coordinates: contigs are concatenated into one global axis; gpos = pos_offset[c] + pos,
// Ltot = sum of contig lengths.  Reads never cross a contig, so per-position prefix counts
// taken over the global axis cancel exactly at contig borders.
//
// One translation unit, kept in parts under kernels/ (included below, in dependency order):
//   wave_primitives          DPP helpers, wave reductions and scans
//   prepare_scan             k_prepare (validate, statistics, partition histogram), exclusive scan, the two columns a
//                            route asks for late (k_gstart, k_fill_ends)
//   radix_sort               LSD radix passes (sort-based routes)
//   bucket_offsets           sort-based routes: bucket offsets from the sorted keys (heads + reverse min-scan)
//   ranked_route             range partition (one or two levels), per-range offsets, ordered ranking
//   pass_major               the same route without the range-major copy: one pass over the reads sorts every pass of
//                            8 192 in place; the per-range kernels walk its slices (included last: uses the launchers' helpers)
//   sweep_uniform            block forms of the uniform-span sweep, single-wave kernel
//   sweep_segments           cut points (coverage <= M): contigs split into independently swept stretches
//   sweep_uniform_pipelines  seven-wave pipelines: fast form with checked fallback, all-general form
//   sweep_uniform_events     event-driven form for deep data: pack (whole chip), chain (one wave per contig,
//                            LDS-DMA ring), expand (whole chip)
//   sweep_mixed              mixed-span event sweeps (register-resident, LDS-cached, plain)
//   mark_and_next_rows       keep-mask emission for the sort-based routes, coverage probes, FILTER,
//                            pair compaction / completion
//   launchers                host-side launch wrappers declared in qmcp_kernels.h (no kernels): the pick of a template
//                            instantiation from run-time values (dispatch_int / _bool / _sorted / _keys), the sweeps
//                            on a SweepAxis
//   near_uniform             one dominant span + a few shorter reads: the one-span sweep over the regular reads, the
//                            exceptions verified against it and selected one event at a time
//   by_contig                reads in any order with a contig id each: sort keys, contig bounds, gather, mask scatter-back
//   ladder                   the coverage ladder between two levels: compaction of the kept reads with their input index,
//                            the next level's contig offsets, the level bytes
//   amplicon_by_contig       the FILTER of pairs against the amplicons of their own contig, compaction with the ids
//   quality_cells            the quality pass: within every (contig, start, end) cell, the plain solve's count of reads
//                            chosen by quality descending, then read index (composite keys, LSD radix, segmented choice)
//   targets                  on-target downsampling: reads projected onto their contig's target positions, compaction
//                            of the on-target reads, the compact mask expanded back to input order
//   depth_report             depth before and after a keep mask per contig and region: the reads' events (two 64-bit
//                            atomics per read), chunk sums, spine, and the pass that turns them into rows and histograms
//   depth_track              the report's events and spine again, run-length compacted: runs of equal depth counted per
//                            chunk, the counts scanned, and the records written at their ranks (no atomics)
//   stratified               one coverage cap per stratum (strand, read group, sample): validation and stratum-major sort
//                            keys, and the per-stratum rows as a segmented reduction over the grouped records
//   dedup                    duplicate families collapsed before the solve: ranges and validation, composite keys, head
//                            flags, cell ids, survivor / duplicate bits, family statistics, compaction of the survivors
//   start_cap                at most K reads per (contig, start, group) cell before the solve: composite keys, every
//                            cell's first position, survivor / capped bits by rank in cell, the kept members per cell
//   amplicon_clip            amplicon-aware downsampling: one streaming pass that validates, filters, assigns every unit
//                            to one amplicon of its contig and clips its reads to the insert; the counters' totals
//   profile                  a cap that varies along the genome: need(p) = min(cov(p), cap(p)) per position with its cut
//                            flag, and the cut-point scan over it
//   pairs                    pair-aware downsampling: the kept set's bits in a batch's grouped order and their complement,
//                            the kept reads' depth as scanned events, need(p) = min(cov_rest(p), T - credit(p))
//   tiers                    tiered downsampling: tier-major sort keys, the kept reads of a solved batch appended to a
//                            list of {contig, start, end}, the list's depth on a later batch's axis as scanned events,
//                            need(p) = min(cov_tier(p), M - credit(p)) with its three counters
//   templates                template-aware downsampling: id check and template sizes, and the completion of a kept set
//                            through a bitset of template ids (mark, spread)
//   templates_profile        the template stages under a cap table: need(p) from the regions' scaled caps and the credit,
//                            and the segments and templates that touch a positive cap
//   fragments                fragment depth: the segments of a template clipped where they overlap -- validation, sort keys
//                            by (template, contig, start), a segmented running maximum of the ends (tiles, spine, apply)
//                            and the clipped columns written back to input order
//   ceiling                  ceiling downsampling: need(p) = max(0, cov(p) - cap(p)) for the dropped set, the check of the
//                            kept depth against the caps, and the complement over the placed reads (mates joined first)
//   proportional             proportional downsampling: need(p) = min(cov(p), M, max(ceil(cov(p) * num / den), floor)) in
//                            exact integers with its cut flag, and the tally of the placed and the kept reads' bases
//   budget                   budget downsampling: the depth histogram of a call, the curve S(M) = sum of min(cov, M) from
//                            it, and a probe's pair completion with its popcount
//   mean_depth               mean-depth downsampling: the budget's histogram over the positions of a region set only, the
//                            reads' weights inside it, and a probe's kept bases
//   thresholds               coverage thresholds: one coverage's mask folded into every read's smallest keeping
//                            coverage, the mates' minimum, and the histogram and running sum of the final thresholds
//   replicates               disjoint replicates: the dense split of a replicate's candidates into labels and the next
//                            replicate's columns (LDS-staged), the next contig offsets, the taken mask and its gather,
//                            the mates' completion, the packed mask of one label
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "qmcp_kernels.h"
#include "target_table.h"  // project_read: shared with the host
#include "pm_div.h"        // the walk's division by the sweep's span: constants on the host, multiply on the device

namespace qmcp {

static constexpr int kWave = 64;
// "no constraint".  Real counts stay < 2^28 per contig (checked by the host).  In the map
// algebra below b, u and v never accumulate (a composite's b is <= its first element's b, its
// u and v are <= its last element's), so the largest intermediate is u + b <= 2 kInf + 2^29
// < 2^32: nothing wraps, no saturation is needed, and anything >= kInf just means "infinite"
// (every finite value is < 2^29 < kInf).
static constexpr uint32_t kInf = 0x40000000u;

#include "kernels/wave_primitives.inc.hip"
#include "kernels/prepare_scan.inc.hip"
#include "kernels/radix_sort.inc.hip"
#include "kernels/ranked_route.inc.hip"
#include "kernels/bucket_offsets.inc.hip"
#include "kernels/sweep_uniform.inc.hip"
#include "kernels/sweep_segments.inc.hip"
#include "kernels/sweep_uniform_pipelines.inc.hip"
#include "kernels/sweep_uniform_events.inc.hip"
#include "kernels/sweep_mixed.inc.hip"
#include "kernels/mark_and_next_rows.inc.hip"
#include "kernels/launchers.inc.hip"
#include "kernels/pm_lane_rank.inc.hip"
#include "kernels/pass_major.inc.hip"
#include "kernels/near_uniform.inc.hip"
#include "kernels/by_contig.inc.hip"
#include "kernels/ladder.inc.hip"
#include "kernels/amplicon_by_contig.inc.hip"
#include "kernels/quality_cells.inc.hip"
#include "kernels/targets.inc.hip"
#include "kernels/depth_report.inc.hip"
#include "kernels/depth_track.inc.hip"
#include "kernels/stratified.inc.hip"
#include "kernels/dedup.inc.hip"
#include "kernels/start_cap.inc.hip"
#include "kernels/amplicon_clip.inc.hip"
#include "kernels/profile.inc.hip"
#include "kernels/pairs.inc.hip"
#include "kernels/tiers.inc.hip"
#include "kernels/templates.inc.hip"
#include "kernels/templates_profile.inc.hip"
#include "kernels/fragments.inc.hip"
#include "kernels/ceiling.inc.hip"
#include "kernels/proportional.inc.hip"
#include "kernels/budget.inc.hip"
#include "kernels/mean_depth.inc.hip"
#include "kernels/thresholds.inc.hip"
#include "kernels/replicates.inc.hip"

}  // namespace qmcp
