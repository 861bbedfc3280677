// fragment_plan.h -- the host side of fragment depth (qmcp_hip_clip_templates_*, qmcp_hip_solve_fragments_*): which
// digits the sort by (template id, contig id, start) has to look at, and in how many rounds of u64 keys.
//
// Plain C++17 (no HIP): api/fragments.inc.hip includes it, and so can a host-only test.  The sort is the stable LSD
// radix of 8-bit digits (radix_sort_wide), so a field costs one pass per BYTE its largest value needs: bytes of
// n_templates - 1, of n_contigs - 1 (at most 3: a by-contig call has at most 2^24 contigs) and of the longest contig's
// last position.  At most 4 + 3 + 4 = 11 bytes: when they fit 8 the key is template | contig | start in one round,
// otherwise round 0 sorts by contig | start and round 1 by the template id, gathered through round 0's value column
// (the stable passes keep round 0's order inside a template).  A plan never has zero passes: one pass over a byte that
// is zero everywhere moves nothing and leaves the index column every later stage reads.
#ifndef QMCP_FRAGMENT_PLAN_H
#define QMCP_FRAGMENT_PLAN_H
#include <cstdint>

namespace qmcp {

// the bytes a field whose largest value is max_value needs (0 when it is always 0)
inline uint32_t bytes_in_use(uint32_t max_value) {
    uint32_t b = 0;
    while (max_value) {
        ++b;
        max_value >>= 8;
    }
    return b;
}

struct FragmentRound {
    uint32_t passes;          // 8-bit passes of this round (its key bytes, at least 1 in round 0)
    uint32_t start_bytes;     // the key's fields from the low end; a field of 0 bytes is not in this round's key
    uint32_t contig_bytes;
    uint32_t template_bytes;
};

struct FragmentPlan {
    uint32_t n_rounds;        // 1 or 2
    FragmentRound rounds[2];
    uint32_t passes;          // over all rounds
    uint32_t key_bytes;       // start + contig + template bytes in use
};

inline FragmentPlan plan_fragment_sort(uint32_t n_templates, uint32_t n_contigs, uint32_t longest_contig) {
    const uint32_t sb = bytes_in_use(longest_contig ? longest_contig - 1u : 0u);
    const uint32_t cb = bytes_in_use(n_contigs ? n_contigs - 1u : 0u);
    const uint32_t tb = bytes_in_use(n_templates ? n_templates - 1u : 0u);
    FragmentPlan p = {};
    p.key_bytes = sb + cb + tb;
    if (p.key_bytes <= 8u) {
        p.n_rounds = 1;
        p.rounds[0] = {p.key_bytes ? p.key_bytes : 1u, sb, cb, tb};
    } else {
        p.n_rounds = 2;
        p.rounds[0] = {sb + cb, sb, cb, 0u};
        p.rounds[1] = {tb, 0u, 0u, tb};
    }
    p.passes = p.rounds[0].passes + p.rounds[1].passes;
    return p;
}

}  // namespace qmcp
#endif
