// solve_words.h -- the word layouts the plain solve's host code and kernels share through small buffers: which word of
// `ranges`, of the device statistics, of the result scalars and of the pinned landing zones means what.  Plain C++
// (no HIP): api/*.inc.hip, the stage drivers under tests/cpp and g++-built tests include it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace qmcp {
namespace words {

// c->ranges (u32 words), the range-ranked route's tables: the first position of every range and the end behind the last
// in [0, kRangeStartWords); the heaviest range's reads and (pass-major form; stats only) wave-slots; for two partition
// levels super_start, tile_base and pass_base, 257 words each
enum Ranges : uint32_t { kRangeStartWords = 65537, kMaxLoad = 65540, kMaxLoadWaveSlots = 65541, kSegTables = 65544,
                         kSegTableWords = 3 * 257, kRangesWords = kRangeStartWords + 7 + kSegTableWords + 5 };
static_assert(kSegTables == kRangeStartWords + 7 && kSegTables + kSegTableWords + 5 == kRangesWords, "ranges layout");
inline uint32_t* max_load(uint32_t* ranges) { return ranges + kMaxLoad; }
inline uint32_t* seg_tables(uint32_t* ranges) { return ranges + kSegTables; }

// c->stats (u32 words): what the head's producer and the tail's small kernels count
enum Stats : uint32_t {
    kMinSpan = 0,         // starts at ~0
    kMaxSpan = 1,
    kBadRead = 2,         // != 0: a read has start > end or end >= its contig length
    kEmptyPositions = 3,  // positions that start no read (k_range_offsets / k_pm_offsets)
    kExceptions = 4,      // near-uniform filter: reads whose span is not the filter's
    kListOverflowed = 5,  // ... != 0: a pass held more exceptions than it can stage
    // Words 6 .. 8 are used twice, never at once: the near-uniform route owns 6 and 7 while it runs, and the mixed route
    // -- which runs only after the near-uniform route has declined -- puts its sample of the spans over them.
    kOverflowEntries = 6,   // near-uniform: exceptions in the list's overflow region (the kernels' n_over)
    kLongestSpanReads = 7,  // near-uniform: reads of the longest span (k_nu_count_span)
    kSpanSample = 6,        // mixed: 3 words -- sampled, in the fullest bin, its span (k_span_mode_share)
    kHeadCounted = 4,       // words kEmptyPositions .. kOverflowEntries: cleared before a head's stages run again
    kStatsInitWords = 8,    // the head's initial values: ~0, then zeros
    kStatsWords = 12,
};

// c->scalars (64 bytes), the solve's results: the kept total (u64) at 0, the sweep's u32 words at 16, the four u32 words
// of a speculative sweep at 32
constexpr size_t kScalarsBytes = 64, kSweepItersAt = 16, kSpecWordsAt = 32;
enum SweepIters : uint32_t { kBlocksChanged = 0, kBlocks = 1, kStretches = 2 };
inline uint32_t* sweep_iters(void* scalars) { return (uint32_t*)((char*)scalars + kSweepItersAt); }
struct SpecWords {
    uint32_t* mismatches1;  // tier 1: boundaries that disagreed
    uint32_t* n_spec1;      //         speculative boundaries
    uint32_t* mismatches2;  // tier 2
    uint32_t* n_spec2;
};
inline SpecWords spec_words(void* scalars) {
    uint32_t* w = (uint32_t*)((char*)scalars + kSpecWordsAt);
    return SpecWords{w, w + 1, w + 2, w + 3};
}

// c->h_scalars (pinned u64 words): the first kHostScalarsRead are the scalars as read back -- iterations: blocks changed
// low, blocks high; stretches low; tier 1: mismatches low, boundaries high; tier 2: mismatches low --, and behind them the
// head's count of empty positions, fetched with the results (u32, the low half)
enum HostScalars : uint32_t { kHostKept = 0, kHostIters = 2, kHostStretches = 3, kHostSpecTier1 = 4, kHostSpecTier2 = 5,
                              kHostScalarsRead = 7, kHostEmptyPositions = 7, kHostScalarsWords = 16 };
inline uint32_t lo32(unsigned long long w) { return (uint32_t)(w & 0xFFFFFFFFull); }
inline uint32_t hi32(unsigned long long w) { return (uint32_t)(w >> 32); }

// c->h_head (pinned u32 words): the read-back that picks the route (empty positions ~0: unknown, the range-ranked head
// did not run), and behind it the kStatsInitWords initial values of the statistics
enum Head : uint32_t { kHeadMinSpan = 0, kHeadMaxSpan = 1, kHeadBadRead = 2, kHeadMaxLoad = 3, kHeadEmptyPositions = 4,
                       kHeadExceptions = 5, kHeadListOverflowed = 6, kHeadMaxLoadWaveSlots = 7, kHeadStatsInit = 8,
                       kHeadWords = 16 };

// c->h_nu (pinned u32 words): the near-uniform route's state words as the rounds leave them; before the rounds the first
// three are the landing zone of the route's own look-ups
enum NearUniform : uint32_t {
    kNuScratch = 0,       // the count of longest-span reads, then the heaviest range of the filtered head
    kNuSelectedLast = 1,  // exceptions the last round selected (before the rounds: exceptions the filtered head listed)
    kNuFlags = 2,         // != 0: a run the replay does not model, or too many suspects (before: the list overflowed)
    kNuSelected = 3,      // selected in all
    kNuSuspects = 4,
    kNuFlagsRead = 5,
    kNuRoundsThatSelected = 6,
    kNuStateWords = 8,
};

}  // namespace words
}  // namespace qmcp
