// amplicon_assign_check.cpp -- csrc/amplicon_assign.h's host search as a stand-alone program (no HIP, no GPU), for
// tests/test_amplicons_clip_cpu.py.  Standard input: n_contigs, the n_contigs + 1 offsets, one "start end" line per
// amplicon, n_units, one "contig smallest_start largest_end" line per unit.  Standard output: one "index several" line
// per unit -- the assigned amplicon's index in the table as given (4294967295: none) and whether a second amplicon
// contains the unit -- after a first line with the table's sorted positions checked (see below).
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "amplicon_assign.h"

int main() {
    uint32_t n_contigs = 0;
    if (std::scanf("%" SCNu32, &n_contigs) != 1) return 2;
    std::vector<uint32_t> offs(n_contigs + 1);
    for (uint32_t& o : offs)
        if (std::scanf("%" SCNu32, &o) != 1) return 2;
    const uint32_t n_amp = offs[n_contigs];
    std::vector<uint32_t> a0(n_amp), a1(n_amp);
    for (uint32_t k = 0; k < n_amp; ++k)
        if (std::scanf("%" SCNu32 " %" SCNu32, &a0[k], &a1[k]) != 2) return 2;
    qmcp::AssignTable t;
    if (qmcp::build_assign_table(offs.data(), a0.data(), a1.data(), nullptr, nullptr, n_contigs, t) != qmcp::kAssignTableOk)
        return 3;
    // the table's own promises: per contig sorted by (start up, end down, index down), pmax the running maximum, the
    // inserts equal to the amplicons when none are given
    for (uint32_t c = 0; c < n_contigs; ++c)
        for (uint32_t k = offs[c]; k < offs[c + 1]; ++k) {
            const uint32_t i = t.index()[k];
            if (i < offs[c] || i >= offs[c + 1] || t.start()[k] != a0[i] || t.end()[k] != a1[i]) return 4;
            if (t.insert_start()[k] != a0[i] || t.insert_end()[k] != a1[i]) return 4;
            uint32_t run = t.end()[k];
            if (k > offs[c]) {
                run = std::max(run, t.pmax()[k - 1]);
                const uint32_t j = k - 1;
                const bool ordered = t.start()[j] < t.start()[k] ||
                                     (t.start()[j] == t.start()[k] &&
                                      (t.end()[j] > t.end()[k] || (t.end()[j] == t.end()[k] && t.index()[j] > i)));
                if (!ordered) return 4;
            }
            if (t.pmax()[k] != run) return 4;
        }
    std::printf("table ok\n");
    uint64_t n_units = 0;
    if (std::scanf("%" SCNu64, &n_units) != 1) return 2;
    for (uint64_t u = 0; u < n_units; ++u) {
        uint32_t c = 0, s = 0, e = 0;
        if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &c, &s, &e) != 3) return 2;
        bool several = false;
        const uint32_t k = qmcp::assign_amplicon(offs.data(), t, c, s, e, &several);
        std::printf("%" PRIu32 " %d\n", k == QMCP_NO_AMPLICON ? QMCP_NO_AMPLICON : t.index()[k], several ? 1 : 0);
    }
    return 0;
}
