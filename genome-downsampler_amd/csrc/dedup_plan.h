// dedup_plan.h -- host-side rules of duplicate-aware downsampling (qmcp_hip_solve_dedup_*): the widths of the sort key's
// fields from the call's own ranges, the form of the sort (32-bit records, split 64-bit keys, or successive stable sorts
// by field when the fields do not fit 64 bits) and its number of 8-bit LSD passes.  Plain C++17, no HIP: shared by
// api/dedup.inc.hip, kernels/dedup.inc.hip (DedupPack) and tests/cpp/dedup_plan_driver.cpp.
//
// Read mode sorts the reads by the key, most significant field first,
//     gstart = pos_offset[contig] + start | span - min_span | tag - tag_min | q_max - q
// (an unplaced read: gstart = the sum of the contig lengths, every other field 0), so that a family (a cell) leaves the
// stable sort as one run with its representative -- highest quality, then lowest index -- first.
// Pair mode sorts the reads by the same key without the quality (stage 1: dense cell ids), then the units by
//     min(id0, id1) | max(id0, id1) | score_max - score
// (stage 2), where an unplaced mate has the id n_placed, one past the largest cell id.
// Fields are listed least significant first everywhere below.
#ifndef QMCP_DEDUP_PLAN_H
#define QMCP_DEDUP_PLAN_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QMCP_DD_HD __host__ __device__
#else
#define QMCP_DD_HD
#endif

namespace qmcp {

static constexpr uint32_t kDedupMaxFields = 4;
enum DedupSortForm : uint32_t {
    DEDUP_SORT_REC32 = 0,   // {u32 key, index} records
    DEDUP_SORT_SPLIT64 = 1, // u64 keys and an index column
    DEDUP_SORT_FIELDS = 2,  // beyond 64 bits: one stable u64 sort per field of non-zero width, least significant first
};

QMCP_DD_HD inline uint32_t dedup_bit_width(uint64_t v) {
    uint32_t b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

// where each field of a round's key goes: key = sum over the fields f with bit f of `on` set of value[f] << shift[f]
struct DedupPack {
    uint32_t shift[kDedupMaxFields];
    uint32_t on;
};

struct DedupRound {
    DedupPack pack;
    uint32_t bits, passes;
};

struct DedupSortPlan {
    uint32_t key_bits;  // sum of the field widths
    uint32_t form;      // DedupSortForm
    uint32_t passes;    // 8-bit LSD passes over all rounds (at least 1: a pass also builds the index column)
    uint32_t n_rounds;  // 1 unless form == DEDUP_SORT_FIELDS
    DedupRound rounds[kDedupMaxFields];
};

inline DedupSortPlan plan_dedup_sort(const uint32_t* field_bits, uint32_t n_fields) {
    DedupSortPlan p{};
    for (uint32_t f = 0; f < n_fields; ++f) p.key_bits += field_bits[f];
    if (p.key_bits <= 64) {
        p.form = p.key_bits <= 32 ? DEDUP_SORT_REC32 : DEDUP_SORT_SPLIT64;
        p.n_rounds = 1;
        DedupRound& r = p.rounds[0];
        uint32_t at = 0;
        for (uint32_t f = 0; f < n_fields; ++f) {
            r.pack.shift[f] = at;
            if (field_bits[f]) r.pack.on |= 1u << f;
            at += field_bits[f];
        }
        r.bits = p.key_bits;
        r.passes = p.key_bits ? (p.key_bits + 7) / 8 : 1;
        p.passes = r.passes;
        return p;
    }
    p.form = DEDUP_SORT_FIELDS;
    for (uint32_t f = 0; f < n_fields; ++f) {
        if (!field_bits[f]) continue;
        DedupRound& r = p.rounds[p.n_rounds++];
        r.pack.on = 1u << f;
        r.bits = field_bits[f];
        r.passes = (field_bits[f] + 7) / 8;
        p.passes += r.passes;
    }
    return p;
}

// read mode: {q_max - q, tag - tag_min, span - min_span, gstart}; the ranges are those of the placed reads (lo > hi: no
// placed read), total_length the sum of the contig lengths (the unplaced reads' gstart).  with_quality == false: stage 1
// of pair mode, whose key carries no quality.
inline void dedup_read_fields(uint64_t total_length, uint32_t min_span, uint32_t max_span, uint32_t tag_lo,
                              uint32_t tag_hi, uint32_t q_lo, uint32_t q_hi, bool with_quality, uint32_t bits[4]) {
    bits[0] = with_quality && q_lo <= q_hi ? dedup_bit_width(q_hi - q_lo) : 0;
    bits[1] = tag_lo <= tag_hi ? dedup_bit_width(tag_hi - tag_lo) : 0;
    bits[2] = min_span <= max_span ? dedup_bit_width(max_span - min_span) : 0;
    bits[3] = dedup_bit_width(total_length);
}

// pair mode, stage 2: {score_max - score, max id, min id}; score <= 2 * (q_hi - q_lo), ids <= n_placed
inline void dedup_pair_fields(uint64_t n_placed, uint32_t q_lo, uint32_t q_hi, uint32_t bits[3]) {
    bits[0] = q_lo <= q_hi ? dedup_bit_width(2ull * (q_hi - q_lo)) : 0;
    bits[1] = dedup_bit_width(n_placed);
    bits[2] = bits[1];
}

}  // namespace qmcp
#endif
