// Amplicon intervals for the FILTER pre-pass.  Mirrors
//   Amplicon / Amplicon::includes            libs/bam-api/include/bam-api/amplicon.hpp:8-16, src/amplicon.cpp:5-7
//   AmpliconSet::member_includes_both        libs/bam-api/src/amplicon_set.cpp:5-9
//   BamApi::set_amplicon_filter              libs/bam-api/src/bam_api.cpp:53-95
//   BamApi::process_bed_file / process_tsv_file   bam_api.cpp:101-186
// The device predicate is qmcp_hip_amplicon_filter_host (include/qmcp_hip.h); this header is
// the host-side construction of the interval list it consumes.
#ifndef QMCP_AMD_BAM_API_AMPLICON_SET_HPP
#define QMCP_AMD_BAM_API_AMPLICON_SET_HPP

#include <cstdint>
#include <filesystem>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "bam-api/read.hpp"

namespace bam_api {

enum class AmpliconBehaviour { IGNORE, FILTER, GRADE };  // bam_api_config.hpp:10-17

struct Amplicon {
    Index start;
    Index end;  // compared inclusively, although BED ends are exclusive: kept as the reference does
    Amplicon(Index s, Index e) : start(s), end(e) {}
    bool includes(const Read& read) const { return start <= read.start_ind && read.end_ind <= end; }
};

struct AmpliconSet {
    std::vector<Amplicon> amplicons;
    bool member_includes_both(const Read& r1, const Read& r2) const {
        for (const Amplicon& a : amplicons)
            if (a.includes(r1) && a.includes(r2)) return true;
        return false;
    }
};

using PrimerMap = std::map<std::string, std::pair<Index, Index>>;

// BED: chrom \t start \t end \t name; the first line carrying a name wins; lines whose
// coordinates do not parse or with an empty field are skipped.  Returns false if the file
// cannot be opened (the reference exits the process there).
bool read_primer_bed(const std::filesystem::path& path, PrimerMap& out);
// TSV: left \t right primer names.
bool read_primer_pairs_tsv(const std::filesystem::path& path,
                           std::vector<std::pair<std::string, std::string>>& out);

// set_amplicon_filter: with a TSV every listed pair gives [left.start, right.end] after
// ordering the two primers by start (the reorder is applied to the map entries themselves,
// as in the reference, so it is visible to later pairs that reuse a primer; unknown names
// behave as (0, 0) primers); without a TSV consecutive primers in name order are paired.
AmpliconSet build_amplicon_set(PrimerMap primers,
                               const std::vector<std::pair<std::string, std::string>>* pairs);
bool amplicon_set_from_files(const std::filesystem::path& bed, const std::filesystem::path& tsv,
                             AmpliconSet& out);

// ---- amplicons matched to references by name (BamApiConfig::amplicons_by_reference)
// A primer with the reference it lies on: the BED's chrom column, which read_primer_bed drops.
struct ChromPrimer {
    std::string chrom;
    Index start = 0, end = 0;
};
using ChromPrimerMap = std::map<std::string, ChromPrimer>;

// read_primer_bed keeping the chrom (the same parsing: the first line carrying a name wins, lines whose coordinates do
// not parse or with an empty field are skipped).  chroms receives every chrom the accepted lines name, in order of
// first appearance (later lines of a name included).  false if the file cannot be opened.
bool read_primer_bed_by_chrom(const std::filesystem::path& path, ChromPrimerMap& out, std::vector<std::string>& chroms);

// The amplicons of every reference in CSR form: reference c owns [offsets[c], offsets[c + 1]) of starts / ends
// (inclusive bounds; the layout qmcp_hip_filter_solve_by_contig_host takes).  QMCP_NO_CONTIG (0xFFFFFFFF) is no
// reference: an unplaced read lies in no amplicon.
struct ReferenceAmpliconSet {
    std::vector<std::uint32_t> offsets{0};
    std::vector<Index> starts, ends;
    // What the primer-clipped entries (qmcp_hip_solve_amplicons_host) need besides: the insert of every amplicon --
    // from BED primers [ls, le) and [rs, re) the amplicon stays [ls, re] (the reference's inclusive quirk) and the
    // insert is [le, rs - 1], inclusive -- and the name of its left primer.  A pair whose primers touch or overlap has
    // no insert (insert_start > insert_end there): empty_insert names the first such pair, and whoever asks for the
    // inserts must refuse the set; the FILTER and GRADE never look at them.
    std::vector<Index> insert_starts, insert_ends;
    std::vector<std::string> left_names;
    std::string empty_insert;
    std::size_t n_references() const { return offsets.size() - 1; }
    // r1 on reference c1, r2 on c2: both on one reference, inside one of its amplicons
    bool member_includes_both(std::uint32_t c1, const Read& r1, std::uint32_t c2, const Read& r2) const {
        if (c1 != c2 || c1 >= n_references()) return false;
        for (std::uint32_t k = offsets[c1]; k < offsets[c1 + 1]; ++k) {
            const Amplicon a(starts[k], ends[k]);
            if (a.includes(r1) && a.includes(r2)) return true;
        }
        return false;
    }
};

// build_amplicon_set per reference.  Every chrom must be one of ref_names, exactly (no aliases).  With a TSV every pair
// gives [left.start, right.end] after ordering the two primers by start (the reorder written back to the map, as in
// build_amplicon_set), on the reference both primers lie on; a name missing from the BED is a (0, 0) primer on the
// reference of the other one.  Without a TSV consecutive primers in name order WITHIN each chrom are paired (an odd
// trailing primer of a chrom has no partner).  false + *err naming the culprit for an unknown chrom, a TSV pair across
// two chroms, or a TSV pair neither of whose names is in the BED.
bool build_reference_amplicon_set(ChromPrimerMap primers, const std::vector<std::string>& chroms,
                                  const std::vector<std::pair<std::string, std::string>>* pairs,
                                  const std::vector<std::string>& ref_names, ReferenceAmpliconSet& out,
                                  std::string* err);
// the files (tsv may be empty) -> the set; false + *err (also when a file cannot be opened)
bool reference_amplicon_set_from_files(const std::filesystem::path& bed, const std::filesystem::path& tsv,
                                       const std::vector<std::string>& ref_names, ReferenceAmpliconSet& out,
                                       std::string* err);

}  // namespace bam_api
#endif
