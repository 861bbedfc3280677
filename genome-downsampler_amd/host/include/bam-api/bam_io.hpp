// BAM ingest / emit without HTSlib: BGZF is a sequence of gzip members
// (zlib is enough) and the BAM records the path needs are fixed-layout.  Mirrors
//   Read::Read(BAMReadId, bam1_t*)      libs/bam-api/src/read.cpp:5-14   (end = pos + reference length of the CIGAR - 1)
//   BamApi::read_bam                    libs/bam-api/src/bam_api.cpp:359-507 (qname map pairing, pair appended when its
//                                       second mate is met, filters per pair, filtered_out_reads_)
//   BamApi::write_bam                   bam_api.cpp:534-656 (second pass over the input, records whose running id is in
//                                       the sorted id list are copied; header copied)
// Parity note: the reference holds no BAM fixture and HTSlib is not in this image, so this module is checked
// by round trips on BAMs its own writer produced (tests/test_bam_io.py): parity unpinned.
#ifndef QMCP_AMD_BAM_API_BAM_IO_HPP
#define QMCP_AMD_BAM_API_BAM_IO_HPP

#include <cstdint>
#include <filesystem>
#include <string>
#include <vector>

#include "bam-api/amplicon_set.hpp"
#include "bam-api/paired_reads.hpp"

namespace bam_api {

struct BamFilters {
    std::uint32_t min_seq_length = 0;  // on l_seq of both mates   (bam_api.cpp:321-323)
    std::uint32_t min_mapq = 0;        // on MAPQ of both mates    (bam_api.cpp:325-327)
    AmpliconBehaviour amplicon_behaviour = AmpliconBehaviour::IGNORE;
    const AmpliconSet* amplicons = nullptr;
    bool per_reference = false;        // fill out.contig_ids / contig_lengths (BamApiConfig::per_reference)
    // BamApiConfig::amplicons_by_reference (needs per_reference): FILTER and GRADE ask this set, with each mate's
    // reference, instead of `amplicons`
    const ReferenceAmpliconSet* reference_amplicons = nullptr;
    // other than NONE (needs per_reference): fill out.strata / stratum_names
    Stratify stratify = Stratify::NONE;
};

struct BamIngestStats {
    std::uint64_t records = 0;        // alignments in the file (BAMReadId runs over these)
    std::uint64_t imported = 0;       // reads appended to the container (whole pairs)
    std::uint32_t min_imported_mapq = UINT32_MAX, max_imported_mapq = 0;  // GRADE only (bam_api.cpp:351-357)
};

// Appends accepted pairs to `out` (mate with FREAD1 first), sets out.ref_genome_length to the first
// reference's length, lists every record id that was not imported in `filtered_out` (ascending).  With
// filters.per_reference also every reference's length (out.contig_lengths) and each appended read's refID
// (out.contig_ids; QMCP_NO_CONTIG for refID == -1) -- pairing and filters are the same either way.
// With filters.stratify also each appended read's stratum (out.strata) and the strata's names (out.stratum_names); no
// record is dropped for its stratum.
// false + *err on a malformed or unreadable file (the reference exits the process there).
bool read_bam(const std::filesystem::path& path, const BamFilters& filters, PairedReads& out,
              std::vector<BAMReadId>& filtered_out, BamIngestStats* stats, std::string* err);

// Template-aware ingest (BamApiConfig::template_aware): every accepted record gives one segment per aligned block, and a
// template is the set of accepted records that share a QNAME -- a single-end read, a pair, a split read with its
// supplementary alignments, a spliced read and its mate.
struct TemplateIngest {
    std::uint32_t min_seq_length = 0;  // a template is dropped when any of its accepted MAPPED records has a shorter l_seq
    std::uint32_t min_mapq = 0;        // ... or a lower MAPQ (the pair rule of read_bam, extended)
    bool split_spliced = true;         // a record is cut at every N operation of its CIGAR; false: one segment per record
    bool include_secondary = false;    // records with flag 0x100 are taken; false: skipped and listed in filtered_out
};
struct TemplateSegments {
    // one entry per segment, in file order, a record's blocks left to right: the inclusive interval, the refID
    // (QMCP_NO_CONTIG for an unmapped record: flag 0x4 or refID -1, one segment with start = end = 0), the template id,
    // the record's MAPQ and l_seq, and the record's id (BAMReadId, the running number of the alignment in the file)
    std::vector<std::uint32_t> starts, ends, contig_ids, template_ids, qualities, seq_lengths;
    std::vector<BAMReadId> segment_records;
    std::uint32_t n_templates = 0;     // ids are dense, in order of first appearance
    std::vector<std::uint32_t> contig_lengths;
    std::uint64_t records = 0;         // alignments in the file
};
// D stays inside its block (as rlen counts it in read_bam); a block is what lies between two N operations and consumes
// reference.  A record whose in-place CIGAR is <l_seq>S<rlen>N and that carries a CG:B,I field takes its CIGAR from the
// field (the long-CIGAR convention, SAM specification 4.2.2).  Every accepted record gives at least one segment: a mapped
// record whose CIGAR consumes no reference gives [pos, pos].  Supplementary records (0x800) are taken.  filtered_out:
// the records that are not in the segments (skipped secondaries, and the records of dropped templates), ascending.
// false + *err on a malformed or unreadable file.
bool read_bam_templates(const std::filesystem::path& path, const TemplateIngest& cfg, TemplateSegments& out,
                        std::vector<BAMReadId>& filtered_out, std::string* err);

// The header's references alone: names and lengths in header order.  false + *err on a malformed or unreadable file.
bool read_bam_references(const std::filesystem::path& path, std::vector<std::string>& names,
                         std::vector<std::uint32_t>& lengths, std::string* err);

// Copies the header and the records whose running id is in `bam_ids` (sorted in place, as the reference does)
// to a new file: BAM if the output's extension is ".bam", SAM text otherwise (bam_api.cpp:564).  BGZF blocks are
// deflated on several threads (QMCP_BAM_THREADS; the reference: hts_set_thread_pool(outfile), bam_api.cpp:569-586).
// Returns the number of records written, or UINT32_MAX + *err on failure.
std::uint32_t write_bam(const std::filesystem::path& input, const std::filesystem::path& output,
                        std::vector<BAMReadId>& bam_ids, std::string* err);

// A record for the synthetic-BAM writer used by the tests (the reference's tests build reads in memory
// and never write one): single reference, CIGAR given as (length, op) with op in "MIDNSHP=X".
// write_bam with one aux field appended to every written record: <tag> S <uint16>, five bytes, block_size grown by five;
// in SAM text <tag>:i:<value>.  tagged holds (record id, value) pairs (sorted here).  Refused BEFORE the output is
// opened: a tag that is not [A-Za-z][A-Za-z0-9], and an input record among the written ones that carries the tag
// already.  UINT32_MAX with *err set on a refusal or failure.
std::uint32_t write_bam_tagged(const std::filesystem::path& input, const std::filesystem::path& output,
                               std::vector<std::pair<BAMReadId, std::uint16_t>>& tagged, const std::string& tag,
                               std::string* err);

struct BamRecordSpec {
    std::string qname;
    std::uint16_t flag = 0;
    std::int32_t pos = 0;
    std::uint8_t mapq = 0;
    std::vector<std::pair<std::uint32_t, char>> cigar;
    std::uint32_t l_seq = 0;
};
bool write_synthetic_bam(const std::filesystem::path& path, const std::string& ref_name,
                         std::uint32_t ref_length, const std::vector<BamRecordSpec>& records,
                         std::string* err);

}  // namespace bam_api
#endif
