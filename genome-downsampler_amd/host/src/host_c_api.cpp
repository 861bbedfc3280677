// C entry points of libqmcp_host.so for ctypes callers (tests, bench.py): the reads-gen
// restatement and the C++ solver adapter driven exactly as the reference drives a solver
// (SolverManager::get(name).solve(M, BamApi)).
#include <chrono>
#include <new>
#include <cstdint>
#include <cstring>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>

#include "bam-api/amplicon_set.hpp"
#include "bam-api/bam_api.hpp"
#include "bam-api/bam_io.hpp"
#include "qmcp-solver/quasi_mcp_hip_quality_solver.hpp"
#include "reads_gen.hpp"
#include "solver_manager.hpp"

namespace {

// Weight functions of the reference's CoverageTester (src/tests/coverage_tester.cpp:157-175).
double low_both_sides(double x) { return x - x * x; }
double with_hole(double x) {
    if (x > 0.3684 && x < 0.6316) return 1000.0 * (x * x - x + 0.25) * (x * x - x + 0.25) + 0.2;
    return 0.5;
}
double zero_both_sides(double x) { return -10.0 * (x - 0.5) * (x - 0.5) + 1.0; }

SolverManager& manager() {
    static SolverManager m;
    return m;
}

// The default manager's solvers, and "quasi-mcp-hip-quality" beside them: an opt-in solver (an embedding application
// registers it with SolverManager::add), so qmcp_host_solver_names keeps listing the default manager only.
constexpr const char* kQualitySolverName = "quasi-mcp-hip-quality";
qmcp::Solver* resolve(const char* name) {
    if (manager().contains(name)) return &manager().get(name);
    if (std::strcmp(name, kQualitySolverName) == 0) {
        static qmcp::QuasiMcpHipQualitySolver quality;
        return &quality;
    }
    return nullptr;
}

// amplicon_mode -1: the solver decides, as App::execute does (src/app.cpp:120-128) -- GRADE for a solver that uses the
// reads' qualities, FILTER for every other
bam_api::AmpliconBehaviour amplicon_behaviour(int amplicon_mode, qmcp::Solver& solver) {
    if (amplicon_mode < 0) amplicon_mode = solver.uses_quality_of_reads() ? 2 : 1;
    return amplicon_mode == 1 ? bam_api::AmpliconBehaviour::FILTER
         : amplicon_mode == 2 ? bam_api::AmpliconBehaviour::GRADE : bam_api::AmpliconBehaviour::IGNORE;
}

}  // namespace

extern "C" {

// kind: 0 uniform, 1 x-x^2, 2 hole, 3 zero-on-both-sides.  Writes 2*pairs reads.
int qmcp_host_reads_gen(std::uint32_t seed, int kind, std::uint64_t pairs,
                        std::uint32_t genome_length, std::uint32_t read_length,
                        std::uint32_t* starts, std::uint32_t* ends, std::uint32_t* qualities) {
    if (genome_length < 2ull * read_length || read_length == 0) return -1;
    std::mt19937 gen(seed);
    switch (kind) {
        case 0:
            reads_gen::rand_reads_uniform_soa(gen, pairs, genome_length, read_length, starts, ends,
                                              qualities);
            return 0;
        case 1:
            reads_gen::rand_reads_soa(gen, pairs, genome_length, read_length, low_both_sides,
                                      starts, ends, qualities);
            return 0;
        case 2:
            reads_gen::rand_reads_soa(gen, pairs, genome_length, read_length, with_hole, starts,
                                      ends, qualities);
            return 0;
        case 3:
            reads_gen::rand_reads_soa(gen, pairs, genome_length, read_length, zero_both_sides,
                                      starts, ends, qualities);
            return 0;
        default:
            return -1;
    }
}

// AoS path of the generator (what the reference's tests call), copied out column-wise;
// lets a test check that the lean SoA variant and the AoS variant agree.
int qmcp_host_reads_gen_aos(std::uint32_t seed, int kind, std::uint64_t pairs,
                            std::uint32_t genome_length, std::uint32_t read_length,
                            std::uint32_t* starts, std::uint32_t* ends, std::uint32_t* qualities) {
    std::mt19937 gen(seed);
    bam_api::AOSPairedReads r;
    if (kind == 0) r = reads_gen::rand_reads_uniform(gen, pairs, genome_length, read_length);
    else if (kind == 1) r = reads_gen::rand_reads(gen, pairs, genome_length, read_length, low_both_sides);
    else if (kind == 2) r = reads_gen::rand_reads(gen, pairs, genome_length, read_length, with_hole);
    else if (kind == 3) r = reads_gen::rand_reads(gen, pairs, genome_length, read_length, zero_both_sides);
    else return -1;
    for (std::size_t i = 0; i < r.reads.size(); ++i) {
        starts[i] = static_cast<std::uint32_t>(r.reads[i].start_ind);
        ends[i] = static_cast<std::uint32_t>(r.reads[i].end_ind);
        if (qualities) qualities[i] = r.reads[i].quality;
        if (r.reads[i].bam_id != i || r.reads[i].is_first_read != (i % 2 == 0)) return -2;
    }
    return 0;
}

// BED (+ optional TSV, may be NULL or "") -> amplicon intervals, as BamApi::set_amplicon_filter
// builds them.  Returns the number of amplicons, -1 if a file cannot be opened, -2 if cap is
// too small.
int qmcp_host_amplicons_from_files(const char* bed_path, const char* tsv_path,
                                   std::uint32_t* starts, std::uint32_t* ends, std::size_t cap) {
    bam_api::AmpliconSet set;
    if (!bam_api::amplicon_set_from_files(bed_path, tsv_path ? tsv_path : "", set)) return -1;
    if (set.amplicons.size() > cap) return -2;
    for (std::size_t i = 0; i < set.amplicons.size(); ++i) {
        starts[i] = static_cast<std::uint32_t>(set.amplicons[i].start);
        ends[i] = static_cast<std::uint32_t>(set.amplicons[i].end);
    }
    return static_cast<int>(set.amplicons.size());
}

// In-memory BamApi helpers as the reference's tests use them (src/tests/coverage_tester.cpp:
// find_input_cover / find_filtered_cover; src/app.cpp:141: find_pairs).  `layout` 0 builds the
// BamApi from an AoS container, 1 from an SoA one (both constructors exist in the reference).
// cover_in / cover_out have ref_genome_length entries; paired_out capacity n; returns the
// number of paired ids.
std::int64_t qmcp_host_bamapi_probe(const std::uint32_t* starts, const std::uint32_t* ends,
                                    std::uint64_t n, std::uint32_t ref_genome_length, int layout,
                                    const std::uint64_t* ids, std::uint64_t n_ids,
                                    std::uint32_t* cover_in, std::uint32_t* cover_out,
                                    std::uint64_t* paired_out) {
    bam_api::AOSPairedReads aos;
    aos.ref_genome_length = ref_genome_length;
    for (std::uint64_t i = 0; i < n; ++i)
        aos.push_back(bam_api::Read(i, starts[i], ends[i], 0, ends[i] - starts[i] + 1, i % 2 == 0));
    bam_api::SOAPairedReads soa;
    soa.from(aos);
    bam_api::BamApi api = layout == 0 ? bam_api::BamApi(aos) : bam_api::BamApi(soa);
    // exercise the lazy layout conversion both ways
    if (api.get_paired_reads_aos().reads.size() != n || api.get_paired_reads_soa().ids.size() != n)
        return -1;
    const std::vector<bam_api::ReadIndex> idv(ids, ids + n_ids);
    const auto in = api.find_input_cover();
    const auto out = api.find_filtered_cover(idv);
    for (std::size_t p = 0; p < in.size(); ++p) { cover_in[p] = in[p]; cover_out[p] = out[p]; }
    const auto paired = api.find_pairs(idv);
    for (std::size_t i = 0; i < paired.size(); ++i) paired_out[i] = paired[i];
    return static_cast<std::int64_t>(paired.size());
}

// Names registered in the SolverManager, '\n'-separated, into buf.
int qmcp_host_solver_names(char* buf, std::size_t cap) {
    std::string all;
    for (const std::string& n : manager().get_names()) { all += n; all += '\n'; }
    if (all.size() + 1 > cap) return -1;
    std::memcpy(buf, all.c_str(), all.size() + 1);
    return static_cast<int>(manager().get_names().size());
}

// 1 if the solver of that name (the default manager's, or "quasi-mcp-hip-quality") uses the reads' qualities -- the
// app then grades amplicon pairs instead of filtering them --, 0 if not, -1 for an unknown name.  Builds nothing on the
// device: solvers touch it on their first solve only.
int qmcp_host_solver_uses_quality(const char* solver_name) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    return found->uses_quality_of_reads() ? 1 : 0;
}

// qmcp_host_solve with each read's quality (qmcp_host_solve builds reads of quality 0): kept_out (capacity n) gets the
// ascending ReadIndex, with_pairs != 0 applies BamApi::find_pairs.  adapter_pairs != 0: the solver itself completes
// pairs on the device for this call (QuasiMcpHipSolver::set_complete_pairs; -2 for a solver without that setter).
// Negative on an unknown solver.
std::int64_t qmcp_host_solve_with_qualities(const char* solver_name, const std::uint32_t* starts,
                                            const std::uint32_t* ends, const std::uint32_t* qualities, std::uint64_t n,
                                            std::uint32_t ref_genome_length, std::uint32_t max_coverage,
                                            int with_pairs, int adapter_pairs, std::uint64_t* kept_out) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::AOSPairedReads aos;
    aos.ref_genome_length = ref_genome_length;
    aos.reserve(n);
    for (std::uint64_t i = 0; i < n; ++i)
        aos.push_back(bam_api::Read(i, starts[i], ends[i], qualities[i], ends[i] - starts[i] + 1, i % 2 == 0));
    bam_api::BamApi api(aos);
    auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
    if (adapter_pairs && hip == nullptr) return -2;
    if (adapter_pairs) hip->set_complete_pairs(true);
    auto solution = found->solve(max_coverage, api);
    if (adapter_pairs) hip->set_complete_pairs(false);
    std::vector<bam_api::ReadIndex> ids = with_pairs ? api.find_pairs(*solution) : *solution;
    for (std::size_t i = 0; i < ids.size(); ++i) kept_out[i] = ids[i];
    return static_cast<std::int64_t>(ids.size());
}

// Runs SolverManager::get(name).solve(M, BamApi(aos)) the way src/app.cpp:134-135 and
// src/tests/coverage_tester.cpp:109-118 do; returns the number of kept reads, fills
// kept_out (capacity n) with ascending ReadIndex; with_pairs != 0 additionally applies
// BamApi::find_pairs (src/app.cpp:141).  Negative on unknown solver.
std::int64_t qmcp_host_solve(const char* solver_name, const std::uint32_t* starts,
                             const std::uint32_t* ends, std::uint64_t n,
                             std::uint32_t ref_genome_length, std::uint32_t max_coverage,
                             int with_pairs, std::uint64_t* kept_out) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::AOSPairedReads aos;
    aos.ref_genome_length = ref_genome_length;
    aos.reserve(n);
    for (std::uint64_t i = 0; i < n; ++i)
        aos.push_back(bam_api::Read(i, starts[i], ends[i], 0, ends[i] - starts[i] + 1, i % 2 == 0));
    bam_api::BamApi api(aos);
    qmcp::Solver& solver = *found;
    auto solution = solver.solve(max_coverage, api);
    std::vector<bam_api::ReadIndex> ids = with_pairs ? api.find_pairs(*solution) : *solution;
    for (std::size_t i = 0; i < ids.size(); ++i) kept_out[i] = ids[i];
    return static_cast<std::int64_t>(ids.size());
}

// ---- BAM ingest / emit (bam-api/bam_io.hpp) for ctypes callers
// Writes a synthetic single-reference BAM: record i = {qname "q<names[i]>", flags[i], pos[i], mapq[i], CIGAR
// "<clip_front[i]>S<match[i]>M<del[i]>D<match2[i]>M" with zero-length parts left out, l_seq = sum of S and M}.
int qmcp_host_write_synthetic_bam(const char* path, std::uint32_t ref_length, std::uint64_t n,
                                  const std::uint32_t* names, const std::uint16_t* flags,
                                  const std::uint32_t* pos, const std::uint8_t* mapq,
                                  const std::uint32_t* clip_front, const std::uint32_t* match,
                                  const std::uint32_t* del, const std::uint32_t* match2) {
    std::vector<bam_api::BamRecordSpec> recs(n);
    for (std::uint64_t i = 0; i < n; ++i) {
        bam_api::BamRecordSpec& r = recs[i];
        r.qname = "q" + std::to_string(names[i]);
        r.flag = flags[i];
        r.pos = (std::int32_t)pos[i];
        r.mapq = mapq[i];
        if (clip_front[i]) r.cigar.push_back({clip_front[i], 'S'});
        if (match[i]) r.cigar.push_back({match[i], 'M'});
        if (del[i]) r.cigar.push_back({del[i], 'D'});
        if (match2[i]) r.cigar.push_back({match2[i], 'M'});
        r.l_seq = clip_front[i] + match[i] + match2[i];
    }
    std::string err;
    return bam_api::write_synthetic_bam(path, "ref1", ref_length, recs, &err) ? 0 : -1;
}

// BamApi(path, config) -> get_paired_reads_soa(): columns out (capacity cap reads); returns the number of
// imported reads, *n_filtered_out = size of get_filtered_out_reads() (ids into filtered_out, capacity cap_f),
// *ref_len = ref_genome_length.  amplicon_mode: 0 IGNORE, 1 FILTER, 2 GRADE (bed/tsv may be NULL or "").
std::int64_t qmcp_host_read_bam(const char* path, const char* bed, const char* tsv, int amplicon_mode,
                                std::uint32_t min_len, std::uint32_t min_mapq, std::uint64_t cap,
                                std::uint64_t* bam_ids, std::uint32_t* starts, std::uint32_t* ends,
                                std::uint32_t* qualities, std::uint32_t* seq_lengths, std::uint8_t* is_first,
                                std::uint64_t cap_f, std::uint64_t* filtered_out, std::uint64_t* n_filtered_out,
                                std::uint32_t* ref_len) {
    bam_api::BamApiConfig cfg;
    if (bed && bed[0]) cfg.bed_filepath = bed;
    if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
    cfg.min_seq_length = min_len;
    cfg.min_mapq = min_mapq;
    cfg.amplicon_behaviour = amplicon_mode == 1 ? bam_api::AmpliconBehaviour::FILTER
                           : amplicon_mode == 2 ? bam_api::AmpliconBehaviour::GRADE : bam_api::AmpliconBehaviour::IGNORE;
    try {
        bam_api::BamApi api(path, cfg);
        const bam_api::SOAPairedReads& r = api.get_paired_reads_soa();
        const std::uint64_t n = r.ids.size();
        if (n > cap || api.get_filtered_out_reads().size() > cap_f) return -2;
        for (std::uint64_t i = 0; i < n; ++i) {
            bam_ids[i] = r.ids[i]; starts[i] = (std::uint32_t)r.start_inds[i]; ends[i] = (std::uint32_t)r.end_inds[i];
            qualities[i] = r.qualities[i]; seq_lengths[i] = r.seq_lengths[i]; is_first[i] = r.is_first_reads[i] ? 1 : 0;
        }
        *n_filtered_out = api.get_filtered_out_reads().size();
        for (std::size_t i = 0; i < api.get_filtered_out_reads().size(); ++i) filtered_out[i] = api.get_filtered_out_reads()[i];
        *ref_len = (std::uint32_t)r.ref_genome_length;
        return (std::int64_t)n;
    } catch (const std::bad_alloc&) {
        return -3;  // (nothing is thrown through the C boundary)
    }
}

// qmcp_host_read_bam with BamApiConfig::per_reference: the same columns, plus each read's contig id (contig_ids, cap
// entries; QMCP_NO_CONTIG for an unmapped read) and every reference's length (ref_lengths, ref_cap entries; *n_refs
// receives the count).  -2 when a capacity is too small, -3 out of memory, -4 with amplicon files (message in err).
std::int64_t qmcp_host_read_bam_per_reference(const char* path, const char* bed, const char* tsv,
                                              std::uint32_t min_len, std::uint32_t min_mapq, std::uint64_t cap,
                                              std::uint64_t* bam_ids, std::uint32_t* starts, std::uint32_t* ends,
                                              std::uint32_t* qualities, std::uint32_t* seq_lengths,
                                              std::uint8_t* is_first, std::uint32_t* contig_ids, std::uint64_t cap_f,
                                              std::uint64_t* filtered_out, std::uint64_t* n_filtered_out,
                                              std::uint64_t ref_cap, std::uint32_t* ref_lengths, std::uint64_t* n_refs,
                                              char* err, std::size_t err_cap) {
    bam_api::BamApiConfig cfg;
    if (bed && bed[0]) cfg.bed_filepath = bed;
    if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
    cfg.min_seq_length = min_len;
    cfg.min_mapq = min_mapq;
    cfg.per_reference = true;
    try {
        bam_api::BamApi api(path, cfg);
        const bam_api::SOAPairedReads& r = api.get_paired_reads_soa();
        const std::uint64_t n = r.ids.size();
        if (n > cap || api.get_filtered_out_reads().size() > cap_f || r.contig_lengths.size() > ref_cap) return -2;
        for (std::uint64_t i = 0; i < n; ++i) {
            bam_ids[i] = r.ids[i]; starts[i] = (std::uint32_t)r.start_inds[i]; ends[i] = (std::uint32_t)r.end_inds[i];
            qualities[i] = r.qualities[i]; seq_lengths[i] = r.seq_lengths[i]; is_first[i] = r.is_first_reads[i] ? 1 : 0;
            contig_ids[i] = r.contig_ids[i];
        }
        *n_filtered_out = api.get_filtered_out_reads().size();
        for (std::size_t i = 0; i < api.get_filtered_out_reads().size(); ++i) filtered_out[i] = api.get_filtered_out_reads()[i];
        *n_refs = r.contig_lengths.size();
        for (std::size_t k = 0; k < r.contig_lengths.size(); ++k) ref_lengths[k] = r.contig_lengths[k];
        return (std::int64_t)n;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        if (err && err_cap) {
            std::strncpy(err, e.what(), err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return -4;
    }
}

// ---- amplicons matched to references by name (BamApiConfig::amplicons_by_reference)
namespace {
void copy_err(const std::string& msg, char* err, std::size_t cap) {
    if (err && cap) {
        std::strncpy(err, msg.c_str(), cap - 1);
        err[cap - 1] = 0;
    }
}
}  // namespace

// BED (+ optional TSV, may be NULL or "") against the references ref_names[0..n_refs) -> the amplicons of every
// reference in CSR form (build_reference_amplicon_set): offsets_out (n_refs + 1 entries), starts_out / ends_out (cap
// entries).  Returns the number of amplicons, -2 if cap is too small, -4 with the message in err (a file that cannot
// be opened, an unknown chrom, a TSV pair across references).
std::int64_t qmcp_host_amplicons_by_reference(const char* bed_path, const char* tsv_path, const char* const* ref_names,
                                              std::uint64_t n_refs, std::uint32_t* offsets_out, std::uint32_t* starts_out,
                                              std::uint32_t* ends_out, std::uint64_t cap, char* err, std::size_t err_cap) {
    try {
        std::vector<std::string> names;
        for (std::uint64_t r = 0; r < n_refs; ++r) names.emplace_back(ref_names[r]);
        bam_api::ReferenceAmpliconSet set;
        std::string msg;
        if (!bam_api::reference_amplicon_set_from_files(bed_path, tsv_path ? tsv_path : "", names, set, &msg)) {
            copy_err(msg, err, err_cap);
            return -4;
        }
        if (set.starts.size() > cap) return -2;
        for (std::size_t k = 0; k < set.offsets.size(); ++k) offsets_out[k] = set.offsets[k];
        for (std::size_t i = 0; i < set.starts.size(); ++i) {
            starts_out[i] = static_cast<std::uint32_t>(set.starts[i]);
            ends_out[i] = static_cast<std::uint32_t>(set.ends[i]);
        }
        return static_cast<std::int64_t>(set.starts.size());
    } catch (const std::bad_alloc&) {
        return -3;
    }
}

// The header's reference names, '\n'-separated, into buf (capacity cap) and their lengths (lengths_cap entries).
// Returns the number of references, -2 if a capacity is too small, -1 with the reader's message in buf.
std::int64_t qmcp_host_reference_names(const char* path, char* buf, std::size_t cap, std::uint32_t* lengths,
                                       std::uint64_t lengths_cap) {
    std::vector<std::string> names;
    std::vector<std::uint32_t> lens;
    std::string msg;
    if (!bam_api::read_bam_references(path, names, lens, &msg)) {
        copy_err(msg, buf, cap);
        return -1;
    }
    std::string all;
    for (const std::string& n : names) { all += n; all += '\n'; }
    if (all.size() + 1 > cap || lens.size() > lengths_cap) return -2;
    std::memcpy(buf, all.c_str(), all.size() + 1);
    for (std::size_t k = 0; k < lens.size(); ++k) lengths[k] = lens[k];
    return static_cast<std::int64_t>(names.size());
}

// qmcp_host_read_bam_per_reference with amplicon_mode (0 IGNORE, 1 FILTER, 2 GRADE) and the two flags of BamApiConfig
// (per_reference, amplicons_by_reference).  contig_ids is filled only with per_reference.  -2 when a capacity is too
// small, -3 out of memory, -4 when BamApi refuses the configuration or the amplicon files (message in err).
std::int64_t qmcp_host_read_bam_by_reference(const char* path, const char* bed, const char* tsv, int amplicon_mode,
                                             int per_reference, int amplicons_by_reference, std::uint32_t min_len,
                                             std::uint32_t min_mapq, std::uint64_t cap, std::uint64_t* bam_ids,
                                             std::uint32_t* starts, std::uint32_t* ends, std::uint32_t* qualities,
                                             std::uint32_t* seq_lengths, std::uint8_t* is_first,
                                             std::uint32_t* contig_ids, std::uint64_t cap_f,
                                             std::uint64_t* filtered_out, std::uint64_t* n_filtered_out,
                                             std::uint64_t ref_cap, std::uint32_t* ref_lengths, std::uint64_t* n_refs,
                                             char* err, std::size_t err_cap) {
    bam_api::BamApiConfig cfg;
    if (bed && bed[0]) cfg.bed_filepath = bed;
    if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
    cfg.min_seq_length = min_len;
    cfg.min_mapq = min_mapq;
    cfg.amplicon_behaviour = amplicon_mode == 1 ? bam_api::AmpliconBehaviour::FILTER
                           : amplicon_mode == 2 ? bam_api::AmpliconBehaviour::GRADE : bam_api::AmpliconBehaviour::IGNORE;
    cfg.per_reference = per_reference != 0;
    cfg.amplicons_by_reference = amplicons_by_reference != 0;
    try {
        bam_api::BamApi api(path, cfg);
        const bam_api::SOAPairedReads& r = api.get_paired_reads_soa();
        const std::uint64_t n = r.ids.size();
        if (n > cap || api.get_filtered_out_reads().size() > cap_f || r.contig_lengths.size() > ref_cap) return -2;
        for (std::uint64_t i = 0; i < n; ++i) {
            bam_ids[i] = r.ids[i]; starts[i] = (std::uint32_t)r.start_inds[i]; ends[i] = (std::uint32_t)r.end_inds[i];
            qualities[i] = r.qualities[i]; seq_lengths[i] = r.seq_lengths[i]; is_first[i] = r.is_first_reads[i] ? 1 : 0;
            contig_ids[i] = r.contig_ids.size() == n ? r.contig_ids[i] : 0u;
        }
        *n_filtered_out = api.get_filtered_out_reads().size();
        for (std::size_t i = 0; i < api.get_filtered_out_reads().size(); ++i) filtered_out[i] = api.get_filtered_out_reads()[i];
        *n_refs = r.contig_lengths.size();
        for (std::size_t k = 0; k < r.contig_lengths.size(); ++k) ref_lengths[k] = r.contig_lengths[k];
        return (std::int64_t)n;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// read_bam's own verdict on a file, without BamApi's exit-on-error (the reference exits the process on an
// unreadable input; a caller that wants to look first -- and the tests of corrupt files -- use this): 0 and the
// number of imported reads in *n_reads, or -1 and the reader's message in err (capacity cap).  Allocation
// failures on absurd sizes are reported the same way, never thrown through the C boundary.
int qmcp_host_check_bam(const char* path, std::uint64_t* n_reads, char* err, std::size_t cap) {
    std::string msg;
    int rc = -1;
    try {
        bam_api::SOAPairedReads reads;
        std::vector<bam_api::BAMReadId> filtered;
        bam_api::BamFilters f;
        if (bam_api::read_bam(path, f, reads, filtered, nullptr, &msg)) {
            if (n_reads) *n_reads = reads.ids.size();
            rc = 0;
        }
    } catch (const std::bad_alloc&) {
        msg = "out of memory while reading the BAM file";
    } catch (const std::exception& e) {
        msg = e.what();
    }
    if (err && cap) {
        std::strncpy(err, msg.c_str(), cap - 1);
        err[cap - 1] = 0;
    }
    return rc;
}

// BamApi::write_bam alone (bam_api.cpp:534-656): the header and the records whose running id is in `ids` (n of them;
// sorted here, as the reference sorts them) copied to `out_path` -- BAM if it ends in ".bam", SAM text otherwise.
// Returns the number of records written, -1 on failure (message in err, capacity cap).
std::int64_t qmcp_host_copy_records(const char* in_path, const char* out_path, const std::uint64_t* ids, std::uint64_t n,
                                    char* err, std::size_t cap) {
    std::string msg;
    std::int64_t rc = -1;
    try {
        std::vector<bam_api::BAMReadId> v(ids, ids + n);
        const std::uint32_t written = bam_api::write_bam(in_path, out_path, v, &msg);
        if (written != UINT32_MAX) rc = (std::int64_t)written;
    } catch (const std::exception& e) {
        msg = e.what();
    }
    if (err && cap) {
        std::strncpy(err, msg.c_str(), cap - 1);
        err[cap - 1] = 0;
    }
    return rc;
}

// The file-to-file flow of App::execute (src/app.cpp:113-151) for one solver: BamApi(path) -> solve ->
// find_pairs -> write_paired_reads(out) (+ write_bam_api_filtered_out_reads(filtered) if given).
// Returns the number of records written to `out_path`, negative on an unknown solver.
std::int64_t qmcp_host_downsample_bam(const char* solver_name, const char* in_path, const char* out_path,
                                      const char* filtered_path, std::uint32_t max_coverage,
                                      std::uint32_t min_len, std::uint32_t min_mapq) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::BamApiConfig cfg;
    cfg.min_seq_length = min_len;
    cfg.min_mapq = min_mapq;
    try {
        bam_api::BamApi api(in_path, cfg);
        auto solution = found->solve(max_coverage, api);
        std::vector<bam_api::ReadIndex> paired = api.find_pairs(*solution);
        const std::uint32_t written = api.write_paired_reads(out_path, paired);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        return written;
    } catch (const std::bad_alloc&) {
        return -3;
    }
}

// qmcp_host_downsample_bam with BamApiConfig::per_reference: every reference of the file is its own coverage problem
// (the solver takes qmcp_hip_solve_by_contig_host), pairing and writing as before -- a kept read still brings its mate,
// on whichever reference that lies.  Returns the number of records written, -1 on an unknown solver.
std::int64_t qmcp_host_downsample_bam_per_reference(const char* solver_name, const char* in_path, const char* out_path,
                                                    const char* filtered_path, std::uint32_t max_coverage,
                                                    std::uint32_t min_len, std::uint32_t min_mapq) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::BamApiConfig cfg;
    cfg.min_seq_length = min_len;
    cfg.min_mapq = min_mapq;
    cfg.per_reference = true;
    try {
        bam_api::BamApi api(in_path, cfg);
        auto solution = found->solve(max_coverage, api);
        std::vector<bam_api::ReadIndex> paired = api.find_pairs(*solution);
        const std::uint32_t written = api.write_paired_reads(out_path, paired);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        return written;
    } catch (const std::bad_alloc&) {
        return -3;
    }
}

// qmcp_host_downsample_bam_per_reference with amplicons: BamApiConfig {bed, tsv, amplicon_mode (0 IGNORE, 1 FILTER,
// 2 GRADE), per_reference, amplicons_by_reference}.  FILTER acts during ingest, as in the single-reference flow; the
// survivors are solved one reference at a time and paired as before.  Returns the number of records written, -1 on an
// unknown solver, -3 out of memory, -4 when BamApi refuses the configuration or the amplicon files (message in err).
std::int64_t qmcp_host_downsample_bam_by_reference(const char* solver_name, const char* in_path, const char* out_path,
                                                   const char* filtered_path, std::uint32_t max_coverage,
                                                   std::uint32_t min_len, std::uint32_t min_mapq, const char* bed,
                                                   const char* tsv, int amplicon_mode, int per_reference,
                                                   int amplicons_by_reference, char* err, std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::BamApiConfig cfg;
    if (bed && bed[0]) cfg.bed_filepath = bed;
    if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
    cfg.min_seq_length = min_len;
    cfg.min_mapq = min_mapq;
    cfg.amplicon_behaviour = amplicon_behaviour(amplicon_mode, *found);
    cfg.per_reference = per_reference != 0;
    cfg.amplicons_by_reference = amplicons_by_reference != 0;
    try {
        bam_api::BamApi api(in_path, cfg);
        auto solution = found->solve(max_coverage, api);
        std::vector<bam_api::ReadIndex> paired = api.find_pairs(*solution);
        const std::uint32_t written = api.write_paired_reads(out_path, paired);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        return written;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// qmcp_host_downsample_bam_by_reference with target regions: BamApiConfig {targets_filepath, target_padding,
// keep_off_target} on top of the amplicon fields (bed / tsv may be NULL).  FILTER / GRADE act at ingest as before; the
// targets act in the solve (qmcp_hip_solve_targets_host).  Returns as qmcp_host_downsample_bam_by_reference; -4 also
// when the target BED is refused (targets without per_reference, an unknown chrom, a malformed line).
std::int64_t qmcp_host_downsample_bam_targets(const char* solver_name, const char* in_path, const char* out_path,
                                              const char* filtered_path, std::uint32_t max_coverage,
                                              std::uint32_t min_len, std::uint32_t min_mapq, const char* bed,
                                              const char* tsv, int amplicon_mode, int per_reference,
                                              int amplicons_by_reference, const char* targets,
                                              std::uint32_t target_padding, int keep_off_target, char* err,
                                              std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::BamApiConfig cfg;
    if (bed && bed[0]) cfg.bed_filepath = bed;
    if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
    cfg.min_seq_length = min_len;
    cfg.min_mapq = min_mapq;
    cfg.amplicon_behaviour = amplicon_behaviour(amplicon_mode, *found);
    cfg.per_reference = per_reference != 0;
    cfg.amplicons_by_reference = amplicons_by_reference != 0;
    if (targets && targets[0]) cfg.targets_filepath = targets;
    cfg.target_padding = target_padding;
    cfg.keep_off_target = keep_off_target != 0;
    try {
        bam_api::BamApi api(in_path, cfg);
        auto solution = found->solve(max_coverage, api);
        std::vector<bam_api::ReadIndex> paired = api.find_pairs(*solution);
        const std::uint32_t written = api.write_paired_reads(out_path, paired);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        return written;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// qmcp_host_downsample_bam_targets with a depth report: BamApiConfig {depth_report_filepath, depth_report_bins} on top
// (targets may be NULL: the report is then per reference only).  After the output has been written, the hip solver
// reports the reads the solve saw against the final kept set (after find_pairs) with M = max_coverage and the call's
// targets and padding, and the TSV goes to report_path.  Returns as qmcp_host_downsample_bam_targets; -4 also for a
// report without per_reference or with a solver that has none, -5 when the report cannot be written.
std::int64_t qmcp_host_downsample_bam_report(const char* solver_name, const char* in_path, const char* out_path,
                                             const char* filtered_path, std::uint32_t max_coverage,
                                             std::uint32_t min_len, std::uint32_t min_mapq, const char* bed,
                                             const char* tsv, int amplicon_mode, int per_reference,
                                             int amplicons_by_reference, const char* targets,
                                             std::uint32_t target_padding, int keep_off_target, const char* report_path,
                                             std::uint32_t report_bins, char* err, std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::BamApiConfig cfg;
    if (bed && bed[0]) cfg.bed_filepath = bed;
    if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
    cfg.min_seq_length = min_len;
    cfg.min_mapq = min_mapq;
    cfg.amplicon_behaviour = amplicon_behaviour(amplicon_mode, *found);
    cfg.per_reference = per_reference != 0;
    cfg.amplicons_by_reference = amplicons_by_reference != 0;
    if (targets && targets[0]) cfg.targets_filepath = targets;
    cfg.target_padding = target_padding;
    cfg.keep_off_target = keep_off_target != 0;
    if (report_path && report_path[0]) cfg.depth_report_filepath = report_path;
    cfg.depth_report_bins = report_bins;
    try {
        bam_api::BamApi api(in_path, cfg);
        auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
        if (hip == nullptr && !api.depth_report_filepath().empty())
            throw std::invalid_argument("this solver has no depth report");
        auto solution = found->solve(max_coverage, api);
        std::vector<bam_api::ReadIndex> paired = api.find_pairs(*solution);
        const std::uint32_t written = api.write_paired_reads(out_path, paired);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        if (!api.depth_report_filepath().empty()) {
            std::vector<std::string> names;
            std::vector<std::uint32_t> lengths;
            std::string msg;
            if (!bam_api::read_bam_references(in_path, names, lengths, &msg)) {
                copy_err(msg, err, err_cap);
                return -5;
            }
            qmcp::DepthReport report;
            hip->depth_report(max_coverage, api, paired, api.depth_report_bins(), report);
            if (!qmcp::write_depth_report_tsv(api.depth_report_filepath(), report, names)) {
                copy_err("could not write " + api.depth_report_filepath().string(), err, err_cap);
                return -5;
            }
        }
        return written;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// qmcp_host_downsample_bam_report with a depth track: BamApiConfig {depth_track_filepath, depth_track_channel,
// depth_track_cap} on top (report_path may be NULL: no report).  After the output -- and the report -- has been written,
// the hip solver's depth track of the reads the solve saw against the final kept set (after find_pairs), inside the
// call's targets and padding when given, goes to track_path as bedGraph: channel "kept", "in" or "both", both depths
// compared, zero positions kept.  Returns as qmcp_host_downsample_bam_report; -4 also for a track without per_reference,
// another channel, or a solver that has none, -5 when the track cannot be written.
std::int64_t qmcp_host_downsample_bam_track(const char* solver_name, const char* in_path, const char* out_path,
                                            const char* filtered_path, std::uint32_t max_coverage, std::uint32_t min_len,
                                            std::uint32_t min_mapq, const char* bed, const char* tsv, int amplicon_mode,
                                            int per_reference, int amplicons_by_reference, const char* targets,
                                            std::uint32_t target_padding, int keep_off_target, const char* report_path,
                                            std::uint32_t report_bins, const char* track_path, const char* track_channel,
                                            std::uint32_t track_cap, char* err, std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::BamApiConfig cfg;
    if (bed && bed[0]) cfg.bed_filepath = bed;
    if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
    cfg.min_seq_length = min_len;
    cfg.min_mapq = min_mapq;
    cfg.amplicon_behaviour = amplicon_behaviour(amplicon_mode, *found);
    cfg.per_reference = per_reference != 0;
    cfg.amplicons_by_reference = amplicons_by_reference != 0;
    if (targets && targets[0]) cfg.targets_filepath = targets;
    cfg.target_padding = target_padding;
    cfg.keep_off_target = keep_off_target != 0;
    if (report_path && report_path[0]) cfg.depth_report_filepath = report_path;
    cfg.depth_report_bins = report_bins;
    if (track_path && track_path[0]) cfg.depth_track_filepath = track_path;
    if (track_channel && track_channel[0]) cfg.depth_track_channel = track_channel;
    cfg.depth_track_cap = track_cap;
    try {
        bam_api::BamApi api(in_path, cfg);
        auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
        if (hip == nullptr && !api.depth_report_filepath().empty())
            throw std::invalid_argument("this solver has no depth report");
        if (hip == nullptr && !api.depth_track_filepath().empty())
            throw std::invalid_argument("this solver has no depth track");
        auto solution = found->solve(max_coverage, api);
        std::vector<bam_api::ReadIndex> paired = api.find_pairs(*solution);
        const std::uint32_t written = api.write_paired_reads(out_path, paired);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        if (!api.depth_report_filepath().empty() || !api.depth_track_filepath().empty()) {
            std::vector<std::string> names;
            std::vector<std::uint32_t> lengths;
            std::string msg;
            if (!bam_api::read_bam_references(in_path, names, lengths, &msg)) {
                copy_err(msg, err, err_cap);
                return -5;
            }
            if (!api.depth_report_filepath().empty()) {
                qmcp::DepthReport report;
                hip->depth_report(max_coverage, api, paired, api.depth_report_bins(), report);
                if (!qmcp::write_depth_report_tsv(api.depth_report_filepath(), report, names)) {
                    copy_err("could not write " + api.depth_report_filepath().string(), err, err_cap);
                    return -5;
                }
            }
            if (!api.depth_track_filepath().empty()) {
                qmcp::DepthTrack track;
                hip->depth_track(max_coverage, api, paired, QMCP_TRACK_IN | QMCP_TRACK_KEPT, api.depth_track_cap(), track);
                if (!qmcp::write_depth_track_bedgraph(api.depth_track_filepath(), track, names, api.depth_track_channel())) {
                    copy_err("could not write " + api.depth_track_filepath().string(), err, err_cap);
                    return -5;
                }
            }
        }
        return written;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// qmcp_host_downsample_bam_by_reference with a coverage ladder: BamApiConfig {coverage_ladder} on top of the amplicon
// fields (bed / tsv may be NULL; FILTER acts at ingest as before).  One ingest and one qmcp_hip_solve_ladder_host call;
// the level at max_coverage goes to out_path, level `levels[j]` through find_pairs to out_template with its "{M}"
// replaced by the coverage.  written_out (1 + n_levels entries) receives each file's record count, out_path's first.
// Returns the number of files written; -1 on an unknown solver, -3 out of memory, -4 with a message in err when the
// configuration is refused: no per_reference, a template without "{M}", levels not strictly below max_coverage and
// strictly decreasing, a solver that grades by quality or has no ladder.
std::int64_t qmcp_host_downsample_bam_ladder(const char* solver_name, const char* in_path, const char* out_path,
                                             const char* filtered_path, std::uint32_t max_coverage,
                                             std::uint32_t min_len, std::uint32_t min_mapq, const char* bed,
                                             const char* tsv, int amplicon_mode, int per_reference,
                                             int amplicons_by_reference, const std::uint32_t* levels,
                                             std::uint32_t n_levels, const char* out_template,
                                             std::int64_t* written_out, char* err, std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::BamApiConfig cfg;
    if (bed && bed[0]) cfg.bed_filepath = bed;
    if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
    cfg.min_seq_length = min_len;
    cfg.min_mapq = min_mapq;
    cfg.amplicon_behaviour = amplicon_behaviour(amplicon_mode, *found);
    cfg.per_reference = per_reference != 0;
    cfg.amplicons_by_reference = amplicons_by_reference != 0;
    if (levels != nullptr) cfg.coverage_ladder.assign(levels, levels + n_levels);
    try {
        const std::string tmpl = out_template ? out_template : "";
        const std::size_t at = tmpl.find("{M}");
        if (cfg.coverage_ladder.empty()) throw std::invalid_argument("a coverage ladder needs at least one level");
        if (at == std::string::npos) throw std::invalid_argument("the ladder's output template has no {M}");
        if (found->uses_quality_of_reads())
            throw std::invalid_argument("a coverage ladder does not take a solver that grades by quality");
        auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
        if (hip == nullptr) throw std::invalid_argument("this solver has no coverage ladder");
        bam_api::BamApi api(in_path, cfg);
        auto solutions = hip->solve_ladder(max_coverage, api, api.coverage_ladder());
        for (std::size_t j = 0; j < solutions.size(); ++j) {
            std::string path = out_path;
            if (j > 0) {
                path = tmpl;
                path.replace(at, 3, std::to_string(api.coverage_ladder()[j - 1]));
            }
            std::vector<bam_api::ReadIndex> paired = api.find_pairs(*solutions[j]);
            const std::uint32_t written = api.write_paired_reads(path, paired);
            if (written_out) written_out[j] = written;
        }
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        return (std::int64_t)solutions.size();
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

namespace {
// "strand" / "read_group" -> BamApiConfig::stratify_by; anything else is refused
bam_api::Stratify stratify_from_name(const char* name) {
    const std::string s = name ? name : "";
    if (s == "strand") return bam_api::Stratify::STRAND;
    if (s == "read_group") return bam_api::Stratify::READ_GROUP;
    throw std::invalid_argument("stratify must be \"strand\" or \"read_group\", not \"" + s + "\"");
}
}  // namespace

// qmcp_host_read_bam_per_reference with BamApiConfig::stratify_by ("strand" / "read_group"): the same columns, plus each
// read's stratum (strata, cap entries) and the strata's names, one per line, in names_out (names_cap bytes; *n_strata
// receives the count).  -2 when a capacity is too small, -3 out of memory, -4 with the message in err.
std::int64_t qmcp_host_read_bam_stratified(const char* path, const char* stratify, std::uint32_t min_len,
                                           std::uint32_t min_mapq, std::uint64_t cap, std::uint64_t* bam_ids,
                                           std::uint32_t* starts, std::uint32_t* ends, std::uint32_t* qualities,
                                           std::uint32_t* seq_lengths, std::uint8_t* is_first, std::uint32_t* contig_ids,
                                           std::uint32_t* strata, std::uint64_t cap_f, std::uint64_t* filtered_out,
                                           std::uint64_t* n_filtered_out, std::uint64_t ref_cap,
                                           std::uint32_t* ref_lengths, std::uint64_t* n_refs, char* names_out,
                                           std::size_t names_cap, std::uint64_t* n_strata, int per_reference, char* err,
                                           std::size_t err_cap) {
    try {
        bam_api::BamApiConfig cfg;
        cfg.min_seq_length = min_len;
        cfg.min_mapq = min_mapq;
        cfg.per_reference = per_reference != 0;
        cfg.stratify_by = stratify_from_name(stratify);
        bam_api::BamApi api(path, cfg);
        const bam_api::SOAPairedReads& r = api.get_paired_reads_soa();
        const std::uint64_t n = r.ids.size();
        std::string names;
        for (const std::string& s : r.stratum_names) names += s + "\n";
        if (n > cap || api.get_filtered_out_reads().size() > cap_f || r.contig_lengths.size() > ref_cap ||
            names.size() + 1 > names_cap)
            return -2;
        for (std::uint64_t i = 0; i < n; ++i) {
            bam_ids[i] = r.ids[i]; starts[i] = (std::uint32_t)r.start_inds[i]; ends[i] = (std::uint32_t)r.end_inds[i];
            qualities[i] = r.qualities[i]; seq_lengths[i] = r.seq_lengths[i]; is_first[i] = r.is_first_reads[i] ? 1 : 0;
            contig_ids[i] = r.contig_ids[i];
            strata[i] = r.strata[i];
        }
        *n_filtered_out = api.get_filtered_out_reads().size();
        for (std::size_t i = 0; i < api.get_filtered_out_reads().size(); ++i) filtered_out[i] = api.get_filtered_out_reads()[i];
        *n_refs = r.contig_lengths.size();
        for (std::size_t k = 0; k < r.contig_lengths.size(); ++k) ref_lengths[k] = r.contig_lengths[k];
        std::memcpy(names_out, names.c_str(), names.size() + 1);
        *n_strata = r.stratum_names.size();
        return (std::int64_t)n;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// The file-to-file flow with BamApiConfig::stratify_by ("strand" / "read_group"): one ingest, one
// qmcp_hip_solve_stratified_host call (QuasiMcpHipSolver::solve picks it when the reads carry strata), find_pairs,
// write_paired_reads.  targets / report / ladder_levels are handed to BamApiConfig as given so that it refuses the
// combinations it refuses.  strata_report (may be NULL): a TSV written after the output, one line per stratum -- name,
// cap, reads, kept, mean depth before and after (bases / the sum of the reference lengths) -- of the solve's own kept
// set (before mate completion).  Returns the number of records written; -1 on an unknown solver, -3 out of memory, -4
// with a message in err when the configuration is refused, -5 when the report cannot be written.
std::int64_t qmcp_host_downsample_bam_stratified(const char* solver_name, const char* in_path, const char* out_path,
                                                 const char* filtered_path, std::uint32_t max_coverage,
                                                 std::uint32_t min_len, std::uint32_t min_mapq, int per_reference,
                                                 const char* stratify, const char* targets, const char* report,
                                                 const std::uint32_t* ladder_levels, std::uint32_t n_ladder_levels,
                                                 const char* strata_report, char* err, std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    try {
        bam_api::BamApiConfig cfg;
        cfg.min_seq_length = min_len;
        cfg.min_mapq = min_mapq;
        cfg.per_reference = per_reference != 0;
        cfg.stratify_by = stratify_from_name(stratify);
        if (targets && targets[0]) cfg.targets_filepath = targets;
        if (report && report[0]) cfg.depth_report_filepath = report;
        if (ladder_levels != nullptr) cfg.coverage_ladder.assign(ladder_levels, ladder_levels + n_ladder_levels);
        bam_api::BamApi api(in_path, cfg);
        if (found->uses_quality_of_reads())
            throw std::invalid_argument("stratified downsampling does not take a solver that grades by quality");
        auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
        if (hip == nullptr) throw std::invalid_argument("this solver has no stratified downsampling");
        std::unique_ptr<qmcp::Solution> solution = hip->solve(max_coverage, api);
        std::vector<bam_api::ReadIndex> paired = api.find_pairs(*solution);
        const std::uint32_t written = api.write_paired_reads(out_path, paired);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        if (strata_report && strata_report[0]) {
            const bam_api::SOAPairedReads& r = api.get_paired_reads_soa();
            double positions = 0;
            for (std::uint32_t l : r.contig_lengths) positions += l;
            std::FILE* f = std::fopen(strata_report, "w");
            if (f == nullptr) return -5;
            std::fprintf(f, "#stratum\tcap\treads\tkept\tmean_depth_in\tmean_depth_kept\n");
            for (std::size_t s = 0; s < r.stratum_names.size(); ++s) {
                const qmcp_hip_stratum_row& row = hip->last_stratum_rows()[s];
                std::fprintf(f, "%s\t%u\t%llu\t%llu\t%.6f\t%.6f\n", r.stratum_names[s].c_str(),
                             hip->last_stratum_caps()[s], (unsigned long long)row.n_reads, (unsigned long long)row.n_kept,
                             positions > 0 ? (double)row.bases_in / positions : 0.0,
                             positions > 0 ? (double)row.bases_kept / positions : 0.0);
            }
            if (std::fclose(f) != 0) return -5;
        }
        return (std::int64_t)written;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// The file-to-file flow with BamApiConfig::dedup: one ingest (strand bit and MAPQ per read), one
// qmcp_hip_solve_dedup_host call in pair mode with mate completion (QuasiMcpHipSolver::solve_dedup), find_pairs,
// write_paired_reads -- duplicate pairs are simply not written; filtered_path keeps its meaning of ingest filters only.
// targets / report / ladder_levels / stratify / bed / tsv / amplicons_by_reference are handed to BamApiConfig as given so
// that it refuses the combinations it refuses.  dedup_report (may be NULL): a TSV written after the output -- the
// statistics, then one size<TAB>families line per bin of the family-size histogram at 64 bins.  Returns the number of
// records written; -1 on an unknown solver, -3 out of memory, -4 with a message in err when the configuration is
// refused, -5 when the report cannot be written.
std::int64_t qmcp_host_downsample_bam_dedup(const char* solver_name, const char* in_path, const char* out_path,
                                            const char* filtered_path, std::uint32_t max_coverage, std::uint32_t min_len,
                                            std::uint32_t min_mapq, int per_reference, const char* targets,
                                            const char* report, const std::uint32_t* ladder_levels,
                                            std::uint32_t n_ladder_levels, const char* stratify, const char* bed,
                                            const char* tsv, int amplicons_by_reference, const char* dedup_report,
                                            char* err, std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    try {
        bam_api::BamApiConfig cfg;
        cfg.min_seq_length = min_len;
        cfg.min_mapq = min_mapq;
        cfg.per_reference = per_reference != 0;
        cfg.dedup = true;
        if (targets && targets[0]) cfg.targets_filepath = targets;
        if (report && report[0]) cfg.depth_report_filepath = report;
        if (ladder_levels != nullptr) cfg.coverage_ladder.assign(ladder_levels, ladder_levels + n_ladder_levels);
        if (stratify && stratify[0]) cfg.stratify_by = stratify_from_name(stratify);
        if (bed && bed[0]) cfg.bed_filepath = bed;
        if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
        cfg.amplicons_by_reference = amplicons_by_reference != 0;
        if (cfg.dedup && cfg.per_reference && cfg.amplicons_by_reference)
            throw std::invalid_argument("duplicate-aware downsampling does not take amplicon files");
        bam_api::BamApi api(in_path, cfg);
        if (found->uses_quality_of_reads())
            throw std::invalid_argument("duplicate-aware downsampling does not take a solver that grades by quality");
        auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
        if (hip == nullptr) throw std::invalid_argument("this solver has no duplicate-aware downsampling");
        constexpr std::uint32_t kBins = 64;
        std::unique_ptr<qmcp::Solution> solution = hip->solve_dedup(max_coverage, api, kBins);
        std::vector<bam_api::ReadIndex> paired = api.find_pairs(*solution);
        const std::uint32_t written = api.write_paired_reads(out_path, paired);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        if (dedup_report && dedup_report[0]) {
            const qmcp_hip_dedup_stats& ds = hip->last_dedup_stats();
            std::FILE* f = std::fopen(dedup_report, "w");
            if (f == nullptr) return -5;
            std::fprintf(f, "#stat\tvalue\n");
            std::fprintf(f, "units\t%llu\nfamilies\t%llu\nduplicate_units\t%llu\nlargest_family\t%llu\nreads_survived\t%llu\n",
                         (unsigned long long)ds.units, (unsigned long long)ds.families,
                         (unsigned long long)ds.duplicate_units, (unsigned long long)ds.largest_family,
                         (unsigned long long)ds.reads_survived);
            std::fprintf(f, "#size\tfamilies\n");
            for (std::uint32_t b = 0; b < kBins; ++b)
                std::fprintf(f, "%u\t%llu\n", b + 1, (unsigned long long)hip->last_dedup_hist()[b]);
            if (std::fclose(f) != 0) return -5;
        }
        return (std::int64_t)written;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// The file-to-file flow with a coverage profile: one per-reference ingest, one qmcp_hip_solve_profile_host call
// (QuasiMcpHipSolver::solve_profile) with the regions in CSR form per reference of the file (n_refs + 1 offsets; the
// caller has matched chroms to references and flattened overlaps) and max_coverage as the default cap, find_pairs,
// write_paired_reads.  Refused, each with its own message (-4): no per_reference, targets, a depth report, a ladder,
// stratify, dedup, amplicon files, a solver that grades by quality, offsets for another number of references.  Returns
// the number of records written; -1 on an unknown solver, -3 out of memory.
std::int64_t qmcp_host_downsample_bam_profile(const char* solver_name, const char* in_path, const char* out_path,
                                              const char* filtered_path, std::uint32_t max_coverage, std::uint32_t min_len,
                                              std::uint32_t min_mapq, int per_reference, const std::uint32_t* region_offsets,
                                              const std::uint32_t* region_starts, const std::uint32_t* region_ends,
                                              const std::uint32_t* region_caps, std::uint64_t n_refs, const char* targets,
                                              const char* report, std::uint32_t n_ladder_levels, const char* stratify,
                                              int dedup, const char* bed, const char* tsv, int amplicons_by_reference,
                                              char* err, std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    try {
        if (!per_reference) throw std::invalid_argument("a coverage profile needs per_reference");
        if (targets && targets[0]) throw std::invalid_argument("a coverage profile does not go together with targets");
        if (report && report[0]) throw std::invalid_argument("a coverage profile does not go together with a depth report");
        if (n_ladder_levels) throw std::invalid_argument("a coverage profile does not go together with a coverage ladder");
        if (stratify && stratify[0]) throw std::invalid_argument("a coverage profile does not go together with stratify_by");
        if (dedup) throw std::invalid_argument("a coverage profile does not go together with dedup");
        if ((bed && bed[0]) || (tsv && tsv[0]) || amplicons_by_reference)
            throw std::invalid_argument("a coverage profile does not take amplicon files");
        if (found->uses_quality_of_reads())
            throw std::invalid_argument("a coverage profile does not take a solver that grades by quality");
        auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
        if (hip == nullptr) throw std::invalid_argument("this solver has no coverage profile");
        if (region_offsets == nullptr) throw std::invalid_argument("a coverage profile needs its region offsets");
        bam_api::BamApiConfig cfg;
        cfg.min_seq_length = min_len;
        cfg.min_mapq = min_mapq;
        cfg.per_reference = true;
        bam_api::BamApi api(in_path, cfg);
        const std::uint32_t n_reg = region_offsets[n_refs];
        if (n_reg && (!region_starts || !region_ends || !region_caps))
            throw std::invalid_argument("a coverage profile with regions needs their starts, ends and caps");
        const std::vector<std::uint32_t> offs(region_offsets, region_offsets + n_refs + 1);
        const std::vector<std::uint32_t> rs(region_starts, region_starts + n_reg), re(region_ends, region_ends + n_reg),
            caps(region_caps, region_caps + n_reg);
        std::unique_ptr<qmcp::Solution> solution = hip->solve_profile(max_coverage, api, offs, rs, re, caps);
        std::vector<bam_api::ReadIndex> paired = api.find_pairs(*solution);
        const std::uint32_t written = api.write_paired_reads(out_path, paired);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        return (std::int64_t)written;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// The file-to-file flow with BamApiConfig::pair_aware: one per-reference ingest, one qmcp_hip_solve_pairs_host call
// (QuasiMcpHipSolver::solve_pairs) under `stages` (NULL or n_stages == 0: the default schedule), write_paired_reads from
// its mask -- whole pairs already, so NO find_pairs.  targets / report / track / ladder_levels / stratify / dedup / bed /
// tsv / amplicons_by_reference are handed to BamApiConfig as given so that it refuses the combinations it refuses; a
// coverage profile (profile != 0) and a solver that grades by quality are refused here.  Returns the number of records
// written; -1 on an unknown solver, -3 out of memory, -4 with a message in err when the configuration is refused.
std::int64_t qmcp_host_downsample_bam_pairs(const char* solver_name, const char* in_path, const char* out_path,
                                            const char* filtered_path, std::uint32_t max_coverage, std::uint32_t min_len,
                                            std::uint32_t min_mapq, int per_reference, const std::uint32_t* stages,
                                            std::uint32_t n_stages, const char* targets, const char* report,
                                            const char* track, const std::uint32_t* ladder_levels,
                                            std::uint32_t n_ladder_levels, const char* stratify, int dedup, int profile,
                                            const char* bed, const char* tsv, int amplicons_by_reference, char* err,
                                            std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    try {
        bam_api::BamApiConfig cfg;
        cfg.min_seq_length = min_len;
        cfg.min_mapq = min_mapq;
        cfg.per_reference = per_reference != 0;
        cfg.pair_aware = true;
        if (stages != nullptr && n_stages) cfg.pair_stages.assign(stages, stages + n_stages);
        if (targets && targets[0]) cfg.targets_filepath = targets;
        if (report && report[0]) cfg.depth_report_filepath = report;
        if (track && track[0]) cfg.depth_track_filepath = track;
        if (ladder_levels != nullptr) cfg.coverage_ladder.assign(ladder_levels, ladder_levels + n_ladder_levels);
        if (stratify && stratify[0]) cfg.stratify_by = stratify_from_name(stratify);
        cfg.dedup = dedup != 0;
        if (bed && bed[0]) cfg.bed_filepath = bed;
        if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
        cfg.amplicons_by_reference = amplicons_by_reference != 0;
        if (profile) throw std::invalid_argument("pair-aware downsampling does not go together with a coverage profile");
        if (found->uses_quality_of_reads())
            throw std::invalid_argument("pair-aware downsampling does not take a solver that grades by quality");
        auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
        if (hip == nullptr) throw std::invalid_argument("this solver has no pair-aware downsampling");
        bam_api::BamApi api(in_path, cfg);
        std::unique_ptr<qmcp::Solution> solution = hip->solve_pairs(max_coverage, api);
        std::vector<bam_api::ReadIndex> kept(solution->begin(), solution->end());
        const std::uint32_t written = api.write_paired_reads(out_path, kept);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        return (std::int64_t)written;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// The file-to-file flow with BamApiConfig::ceiling: one per-reference ingest, one qmcp_hip_solve_ceiling_host call with
// QMCP_CEILING_WHOLE_PAIRS (QuasiMcpHipSolver::solve_ceiling) -- max_coverage is the ceiling; with a coverage profile
// (region_offsets != NULL: n_refs + 1 offsets, as qmcp_host_downsample_bam_profile takes them) the regions' caps are
// ceilings and max_coverage applies elsewhere -- and write_paired_reads from its mask: whole pairs already, and NO
// find_pairs, which would put depth back.  targets / report / track / ladder_levels / stratify / dedup / pair_aware /
// template_aware / bed / tsv / amplicons_by_reference are handed to BamApiConfig as given so that it refuses the
// combinations it refuses; a solver that grades by quality is refused here.  ceiling_report (may be NULL): a TSV
// stat<TAB>value with the qmcp_hip_ceiling_stats and the records written.  cstats (may be NULL) takes the stats.  Returns
// the number of records written; -1 on an unknown solver, -3 out of memory, -4 with a message in err when the
// configuration is refused, -5 when the report cannot be written.
std::int64_t qmcp_host_downsample_bam_ceiling(const char* solver_name, const char* in_path, const char* out_path,
                                              const char* filtered_path, std::uint32_t max_coverage, std::uint32_t min_len,
                                              std::uint32_t min_mapq, int per_reference, const std::uint32_t* region_offsets,
                                              const std::uint32_t* region_starts, const std::uint32_t* region_ends,
                                              const std::uint32_t* region_caps, std::uint64_t n_refs, const char* targets,
                                              const char* report, const char* track, const std::uint32_t* ladder_levels,
                                              std::uint32_t n_ladder_levels, const char* stratify, int dedup, int pair_aware,
                                              int template_aware, const char* bed, const char* tsv,
                                              int amplicons_by_reference, const char* ceiling_report,
                                              qmcp_hip_ceiling_stats* cstats, char* err, std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    try {
        bam_api::BamApiConfig cfg;
        cfg.min_seq_length = min_len;
        cfg.min_mapq = min_mapq;
        cfg.per_reference = per_reference != 0;
        cfg.ceiling = true;
        cfg.pair_aware = pair_aware != 0;
        cfg.template_aware = template_aware != 0;
        if (targets && targets[0]) cfg.targets_filepath = targets;
        if (report && report[0]) cfg.depth_report_filepath = report;
        if (track && track[0]) cfg.depth_track_filepath = track;
        if (ladder_levels != nullptr) cfg.coverage_ladder.assign(ladder_levels, ladder_levels + n_ladder_levels);
        if (stratify && stratify[0]) cfg.stratify_by = stratify_from_name(stratify);
        cfg.dedup = dedup != 0;
        if (bed && bed[0]) cfg.bed_filepath = bed;
        if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
        cfg.amplicons_by_reference = amplicons_by_reference != 0;
        if (found->uses_quality_of_reads())
            throw std::invalid_argument("ceiling downsampling does not take a solver that grades by quality");
        auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
        if (hip == nullptr) throw std::invalid_argument("this solver has no ceiling downsampling");
        bam_api::BamApi api(in_path, cfg);
        std::vector<std::uint32_t> offs, rs, re, caps;
        if (region_offsets != nullptr) {
            const std::uint32_t n_reg = region_offsets[n_refs];
            if (n_reg && (!region_starts || !region_ends || !region_caps))
                throw std::invalid_argument("a coverage profile with regions needs their starts, ends and caps");
            offs.assign(region_offsets, region_offsets + n_refs + 1);
            if (n_reg) {
                rs.assign(region_starts, region_starts + n_reg);
                re.assign(region_ends, region_ends + n_reg);
                caps.assign(region_caps, region_caps + n_reg);
            }
        }
        std::unique_ptr<qmcp::Solution> solution = hip->solve_ceiling(max_coverage, api, offs, rs, re, caps);
        std::vector<bam_api::ReadIndex> kept(solution->begin(), solution->end());
        const std::uint32_t written = api.write_paired_reads(out_path, kept);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        const qmcp_hip_ceiling_stats& cs = hip->last_ceiling_stats();
        if (cstats != nullptr) *cstats = cs;
        if (ceiling_report && ceiling_report[0]) {
            std::FILE* f = std::fopen(ceiling_report, "w");
            if (f == nullptr) return -5;
            std::fprintf(f, "#stat\tvalue\n");
            std::fprintf(f, "reads_placed\t%llu\nreads_dropped\t%llu\nmates_dropped\t%llu\nover_positions\t%llu\n"
                            "over_bases\t%llu\nshort_positions\t%llu\nshort_bases\t%llu\nexcess_positions\t%llu\n",
                         (unsigned long long)cs.reads_placed, (unsigned long long)cs.reads_dropped,
                         (unsigned long long)cs.mates_dropped, (unsigned long long)cs.over_positions,
                         (unsigned long long)cs.over_bases, (unsigned long long)cs.short_positions,
                         (unsigned long long)cs.short_bases, (unsigned long long)cs.excess_positions);
            std::fprintf(f, "max_kept_depth\t%u\nregions_in\t%u\nregions_used\t%u\nrecords_written\t%u\n", cs.max_kept_depth,
                         cs.regions_in, cs.regions_used, written);
            if (std::fclose(f) != 0) return -5;
        }
        return (std::int64_t)written;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// The file-to-file flow with BamApiConfig::replicates: one per-reference ingest, one qmcp_hip_solve_replicates_host call
// with QMCP_REPLICATES_WHOLE_PAIRS | QMCP_REPLICATES_SHORTFALL (QuasiMcpHipSolver::solve_replicates) -- replicate 1 at
// max_coverage, replicate r + 2 at further[r] -- and one write_paired_reads per replicate from its label: replicate 1 to
// out_path, replicate R to out_template with its "{R}" replaced.  NO find_pairs: it would copy a record into two files,
// so every input record is written at most once over all files.  targets / report / track / ladder_levels / stratify /
// dedup / pair_aware / template_aware / ceiling / bed / tsv / amplicons_by_reference are handed to BamApiConfig as given
// so that it refuses the combinations it refuses; a solver that grades by quality is refused here.  written_out (1 +
// n_further entries) receives each file's record count.  replicates_report (may be NULL): a TSV with one line per
// replicate -- coverage, offered, kept, mates, short_positions, short_bases, records_written -- and an n_full line.
// rstats (may be NULL) takes the stats.  Returns the number of files written; -1 on an unknown solver, -3 out of memory,
// -4 with a message in err when the configuration is refused, -5 when the report cannot be written.
std::int64_t qmcp_host_downsample_bam_replicates(const char* solver_name, const char* in_path, const char* out_path,
                                                 const char* filtered_path, std::uint32_t max_coverage, std::uint32_t min_len,
                                                 std::uint32_t min_mapq, int per_reference, const std::uint32_t* further,
                                                 std::uint32_t n_further, const char* out_template, const char* targets,
                                                 const char* report, const char* track, const std::uint32_t* ladder_levels,
                                                 std::uint32_t n_ladder_levels, const char* stratify, int dedup,
                                                 int pair_aware, int template_aware, int ceiling, const char* bed,
                                                 const char* tsv, int amplicons_by_reference, const char* replicates_report,
                                                 std::int64_t* written_out, qmcp_hip_replicates_stats* rstats, char* err,
                                                 std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    try {
        bam_api::BamApiConfig cfg;
        cfg.min_seq_length = min_len;
        cfg.min_mapq = min_mapq;
        cfg.per_reference = per_reference != 0;
        cfg.replicates = std::vector<std::uint32_t>();
        if (further != nullptr) cfg.replicates->assign(further, further + n_further);
        cfg.pair_aware = pair_aware != 0;
        cfg.template_aware = template_aware != 0;
        cfg.ceiling = ceiling != 0;
        if (targets && targets[0]) cfg.targets_filepath = targets;
        if (report && report[0]) cfg.depth_report_filepath = report;
        if (track && track[0]) cfg.depth_track_filepath = track;
        if (ladder_levels != nullptr) cfg.coverage_ladder.assign(ladder_levels, ladder_levels + n_ladder_levels);
        if (stratify && stratify[0]) cfg.stratify_by = stratify_from_name(stratify);
        cfg.dedup = dedup != 0;
        if (bed && bed[0]) cfg.bed_filepath = bed;
        if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
        cfg.amplicons_by_reference = amplicons_by_reference != 0;
        const std::string tmpl = out_template ? out_template : "";
        const std::size_t at = tmpl.find("{R}");
        if (!cfg.replicates->empty() && at == std::string::npos)
            throw std::invalid_argument("the replicates' output template has no {R}");
        if (found->uses_quality_of_reads())
            throw std::invalid_argument("disjoint replicates do not take a solver that grades by quality");
        auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
        if (hip == nullptr) throw std::invalid_argument("this solver has no disjoint replicates");
        bam_api::BamApi api(in_path, cfg);
        const std::vector<std::uint8_t> labels = hip->solve_replicates(max_coverage, api);
        const std::size_t k = api.replicates()->size() + 1;
        std::vector<std::uint32_t> written(k, 0);
        for (std::size_t r = 1; r <= k; ++r) {
            std::string path = out_path;
            if (r > 1) {
                path = tmpl;
                path.replace(at, 3, std::to_string(r));
            }
            std::vector<bam_api::ReadIndex> kept;
            for (std::size_t i = 0; i < labels.size(); ++i)
                if (labels[i] == r) kept.push_back(i);
            written[r - 1] = api.write_paired_reads(path, kept);
            if (written_out) written_out[r - 1] = written[r - 1];
        }
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        const qmcp_hip_replicates_stats& rs = hip->last_replicates_stats();
        if (rstats != nullptr) *rstats = rs;
        if (replicates_report && replicates_report[0]) {
            std::FILE* f = std::fopen(replicates_report, "w");
            if (f == nullptr) return -5;
            std::fprintf(f, "#replicate\tcoverage\toffered\tkept\tmates\tshort_positions\tshort_bases\trecords_written\n");
            for (std::size_t r = 0; r < k; ++r)
                std::fprintf(f, "%zu\t%u\t%llu\t%llu\t%llu\t%llu\t%llu\t%u\n", r + 1,
                             r == 0 ? max_coverage : (*api.replicates())[r - 1], (unsigned long long)rs.n_offered[r],
                             (unsigned long long)rs.n_kept[r], (unsigned long long)rs.n_mates[r],
                             (unsigned long long)rs.short_positions[r], (unsigned long long)rs.short_bases[r], written[r]);
            std::fprintf(f, "n_full\t%u\n", rs.n_full);
            if (std::fclose(f) != 0) return -5;
        }
        return (std::int64_t)k;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// The file-to-file flow with BamApiConfig::budget_reads / budget_fraction: one per-reference ingest, one
// qmcp_hip_solve_budget_host call with QMCP_BUDGET_WHOLE_PAIRS (QuasiMcpHipSolver::solve_budget) -- max_coverage is the
// upper end of the search -- and write_paired_reads from its mask: whole pairs already, and NO find_pairs, which would
// add reads, so the records written stay within the budget.  has_budget_reads != 0: budget_reads counts; budget_fraction
// >= 0: the fraction of the placed reads that passed the ingest filters; both or neither are handed on for BamApiConfig
// and this function to refuse.  targets / report / track / ladder_levels / stratify / dedup / pair_aware / template_aware /
// ceiling / bed / tsv / amplicons_by_reference are handed to BamApiConfig as given so that it refuses the combinations it
// refuses; a solver that grades by quality is refused here.  budget_report (may be NULL): a TSV stat<TAB>value with the
// qmcp_hip_budget_stats and the records written, then one M<TAB>bases line per entry of the curve.  bstats (may be NULL)
// takes the stats.  Returns the number of records written; -1 on an unknown solver, -3 out of memory, -4 with a message
// in err when the configuration is refused, -5 when the report cannot be written.
std::int64_t qmcp_host_downsample_bam_budget(const char* solver_name, const char* in_path, const char* out_path,
                                             const char* filtered_path, std::uint32_t max_coverage, std::uint32_t min_len,
                                             std::uint32_t min_mapq, int per_reference, int has_budget_reads,
                                             std::uint64_t budget_reads, double budget_fraction, const char* targets,
                                             const char* report, const char* track, const std::uint32_t* ladder_levels,
                                             std::uint32_t n_ladder_levels, const char* stratify, int dedup, int pair_aware,
                                             int template_aware, int ceiling, const char* bed, const char* tsv,
                                             int amplicons_by_reference, const char* budget_report,
                                             qmcp_hip_budget_stats* bstats, char* err, std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    try {
        bam_api::BamApiConfig cfg;
        cfg.min_seq_length = min_len;
        cfg.min_mapq = min_mapq;
        cfg.per_reference = per_reference != 0;
        if (has_budget_reads != 0) cfg.budget_reads = budget_reads;
        if (budget_fraction >= 0.0 || budget_fraction != budget_fraction) cfg.budget_fraction = budget_fraction;
        if (!cfg.budget_reads.has_value() && !cfg.budget_fraction.has_value())
            throw std::invalid_argument("budget downsampling needs budget_reads or budget_fraction");
        cfg.ceiling = ceiling != 0;
        cfg.pair_aware = pair_aware != 0;
        cfg.template_aware = template_aware != 0;
        if (targets && targets[0]) cfg.targets_filepath = targets;
        if (report && report[0]) cfg.depth_report_filepath = report;
        if (track && track[0]) cfg.depth_track_filepath = track;
        if (ladder_levels != nullptr) cfg.coverage_ladder.assign(ladder_levels, ladder_levels + n_ladder_levels);
        if (stratify && stratify[0]) cfg.stratify_by = stratify_from_name(stratify);
        cfg.dedup = dedup != 0;
        if (bed && bed[0]) cfg.bed_filepath = bed;
        if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
        cfg.amplicons_by_reference = amplicons_by_reference != 0;
        if (found->uses_quality_of_reads())
            throw std::invalid_argument("budget downsampling does not take a solver that grades by quality");
        auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
        if (hip == nullptr) throw std::invalid_argument("this solver has no budget downsampling");
        bam_api::BamApi api(in_path, cfg);
        std::unique_ptr<qmcp::Solution> solution = hip->solve_budget(max_coverage, api);
        std::vector<bam_api::ReadIndex> kept(solution->begin(), solution->end());
        const std::uint32_t written = api.write_paired_reads(out_path, kept);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        const qmcp_hip_budget_stats& bs = hip->last_budget_stats();
        if (bstats != nullptr) *bstats = bs;
        if (budget_report && budget_report[0]) {
            std::FILE* f = std::fopen(budget_report, "w");
            if (f == nullptr) return -5;
            std::fprintf(f, "#stat\tvalue\n");
            std::fprintf(f, "budget\t%llu\nreads_placed\t%llu\nn_kept\t%llu\nkept_above\t%llu\nbound_above\t%llu\n"
                            "total_bases\t%llu\n",
                         (unsigned long long)bs.budget, (unsigned long long)bs.reads_placed, (unsigned long long)bs.n_kept,
                         (unsigned long long)bs.kept_above, (unsigned long long)bs.bound_above,
                         (unsigned long long)bs.total_bases);
            std::fprintf(f, "coverage\t%u\nmax_depth\t%u\ntop\t%u\nprobes\t%u\ncurve_entries\t%u\nsaturated\t%u\n"
                            "ms_budget\t%.6g\nms_solves\t%.6g\nrecords_written\t%u\n",
                         bs.coverage, bs.max_depth, bs.top, bs.probes, bs.curve_entries, bs.saturated, (double)bs.ms_budget,
                         (double)bs.ms_solves, written);
            std::fprintf(f, "#M\tbases\n");
            const std::vector<std::uint64_t>& curve = hip->last_budget_curve();
            for (std::size_t m = 0; m < curve.size(); ++m)
                std::fprintf(f, "%zu\t%llu\n", m, (unsigned long long)curve[m]);
            if (std::fclose(f) != 0) return -5;
        }
        return (std::int64_t)written;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// Template-aware ingest alone (BamApiConfig::template_aware; bam_api::read_bam_templates): the segments' columns (cap
// entries each; segment_records: each segment's BAM record id), the skipped and dropped records (filtered_out, cap_f
// entries), every reference's length and the number of templates.  Returns the number of segments; -2 when a capacity is
// too small, -3 out of memory, -1 with the reader's message in err on a malformed or unreadable file.
std::int64_t qmcp_host_read_bam_templates(const char* path, std::uint32_t min_len, std::uint32_t min_mapq,
                                          int split_spliced, int include_secondary, std::uint64_t cap,
                                          std::uint32_t* starts, std::uint32_t* ends, std::uint32_t* contig_ids,
                                          std::uint32_t* template_ids, std::uint32_t* qualities,
                                          std::uint32_t* seq_lengths, std::uint64_t* segment_records, std::uint64_t cap_f,
                                          std::uint64_t* filtered_out, std::uint64_t* n_filtered_out, std::uint64_t ref_cap,
                                          std::uint32_t* ref_lengths, std::uint64_t* n_refs, std::uint64_t* n_templates,
                                          char* err, std::size_t err_cap) {
    try {
        bam_api::TemplateIngest cfg;
        cfg.min_seq_length = min_len;
        cfg.min_mapq = min_mapq;
        cfg.split_spliced = split_spliced != 0;
        cfg.include_secondary = include_secondary != 0;
        bam_api::TemplateSegments seg;
        std::vector<bam_api::BAMReadId> filtered;
        std::string msg;
        if (!bam_api::read_bam_templates(path, cfg, seg, filtered, &msg)) {
            copy_err(msg, err, err_cap);
            return -1;
        }
        const std::uint64_t n = seg.starts.size();
        if (n > cap || filtered.size() > cap_f || seg.contig_lengths.size() > ref_cap) return -2;
        for (std::uint64_t i = 0; i < n; ++i) {
            starts[i] = seg.starts[i]; ends[i] = seg.ends[i]; contig_ids[i] = seg.contig_ids[i];
            template_ids[i] = seg.template_ids[i]; qualities[i] = seg.qualities[i]; seq_lengths[i] = seg.seq_lengths[i];
            segment_records[i] = seg.segment_records[i];
        }
        *n_filtered_out = filtered.size();
        for (std::size_t i = 0; i < filtered.size(); ++i) filtered_out[i] = filtered[i];
        *n_refs = seg.contig_lengths.size();
        for (std::size_t k = 0; k < seg.contig_lengths.size(); ++k) ref_lengths[k] = seg.contig_lengths[k];
        *n_templates = seg.n_templates;
        return (std::int64_t)n;
    } catch (const std::bad_alloc&) {
        return -3;
    }
}

// The file-to-file flow with BamApiConfig::template_aware: one template-aware ingest, one qmcp_hip_solve_templates_host
// call (QuasiMcpHipSolver::solve_templates) under `stages` (NULL or n_stages == 0: the default schedule), the records of
// the kept templates written with BamApi::write_records -- NO find_pairs.  Everything pair_aware refuses, and pair_aware
// itself, is handed to BamApiConfig as given so that it refuses it; a coverage profile and a solver that grades by
// quality are refused here.  tstats (may be NULL) receives the call's qmcp_hip_template_stats.  Returns the number of
// records written; -1 on an unknown solver, -3 out of memory, -4 with a message in err when the configuration is refused.
std::int64_t qmcp_host_downsample_bam_templates(const char* solver_name, const char* in_path, const char* out_path,
                                                const char* filtered_path, std::uint32_t max_coverage,
                                                std::uint32_t min_len, std::uint32_t min_mapq, int per_reference,
                                                int split_spliced, int include_secondary, const std::uint32_t* stages,
                                                std::uint32_t n_stages, int pair_aware, const char* targets,
                                                const char* report, const char* track,
                                                const std::uint32_t* ladder_levels, std::uint32_t n_ladder_levels,
                                                const char* stratify, int dedup, int profile, const char* bed,
                                                const char* tsv, int amplicons_by_reference,
                                                qmcp_hip_template_stats* tstats, char* err, std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    try {
        bam_api::BamApiConfig cfg;
        cfg.min_seq_length = min_len;
        cfg.min_mapq = min_mapq;
        cfg.per_reference = per_reference != 0;
        cfg.template_aware = true;
        cfg.split_spliced = split_spliced != 0;
        cfg.include_secondary = include_secondary != 0;
        if (stages != nullptr && n_stages) cfg.template_stages.assign(stages, stages + n_stages);
        cfg.pair_aware = pair_aware != 0;
        if (targets && targets[0]) cfg.targets_filepath = targets;
        if (report && report[0]) cfg.depth_report_filepath = report;
        if (track && track[0]) cfg.depth_track_filepath = track;
        if (ladder_levels != nullptr) cfg.coverage_ladder.assign(ladder_levels, ladder_levels + n_ladder_levels);
        if (stratify && stratify[0]) cfg.stratify_by = stratify_from_name(stratify);
        cfg.dedup = dedup != 0;
        if (bed && bed[0]) cfg.bed_filepath = bed;
        if (tsv && tsv[0]) cfg.tsv_filepath = tsv;
        cfg.amplicons_by_reference = amplicons_by_reference != 0;
        if (profile) throw std::invalid_argument("template-aware downsampling does not go together with a coverage profile");
        if (found->uses_quality_of_reads())
            throw std::invalid_argument("template-aware downsampling does not take a solver that grades by quality");
        auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
        if (hip == nullptr) throw std::invalid_argument("this solver has no template-aware downsampling");
        bam_api::BamApi api(in_path, cfg);
        std::vector<bam_api::BAMReadId> kept = hip->solve_templates(max_coverage, api);
        if (tstats) *tstats = hip->last_template_stats();
        const std::uint32_t written = api.write_records(out_path, kept);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        return (std::int64_t)written;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// The template-aware flow under a cap per region: one template-aware ingest, one qmcp_hip_solve_templates_profile_host
// call (QuasiMcpHipSolver::solve_templates_profile) with the regions in CSR form per reference of the file (n_refs + 1
// offsets, as qmcp_host_downsample_bam_profile takes them; the caller has matched chroms to references and made the
// regions disjoint), default_cap outside them and max_coverage as the scale of `stages`; the records of the kept
// templates written with BamApi::write_records -- NO find_pairs.  per_reference goes to BamApiConfig as given, so that it
// refuses its absence; a solver that grades by quality and offsets for another number of references are refused here.
// tstats / qstats (may be NULL) receive the call's statistics.  Returns the number of records written; -1 on an unknown
// solver, -3 out of memory, -4 with a message in err when the configuration is refused.
std::int64_t qmcp_host_downsample_bam_templates_profile(const char* solver_name, const char* in_path, const char* out_path,
                                                        const char* filtered_path, std::uint32_t max_coverage,
                                                        std::uint32_t min_len, std::uint32_t min_mapq, int per_reference,
                                                        int split_spliced, int include_secondary,
                                                        const std::uint32_t* stages, std::uint32_t n_stages,
                                                        const std::uint32_t* region_offsets,
                                                        const std::uint32_t* region_starts,
                                                        const std::uint32_t* region_ends, const std::uint32_t* region_caps,
                                                        std::uint64_t n_refs, std::uint32_t default_cap,
                                                        qmcp_hip_template_stats* tstats,
                                                        qmcp_hip_template_profile_stats* qstats, char* err,
                                                        std::size_t err_cap) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    try {
        bam_api::BamApiConfig cfg;
        cfg.min_seq_length = min_len;
        cfg.min_mapq = min_mapq;
        cfg.per_reference = per_reference != 0;
        cfg.template_aware = true;
        cfg.split_spliced = split_spliced != 0;
        cfg.include_secondary = include_secondary != 0;
        if (stages != nullptr && n_stages) cfg.template_stages.assign(stages, stages + n_stages);
        if (found->uses_quality_of_reads())
            throw std::invalid_argument("template-aware downsampling does not take a solver that grades by quality");
        auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(found);
        if (hip == nullptr) throw std::invalid_argument("this solver has no template-aware downsampling");
        if (region_offsets == nullptr) throw std::invalid_argument("a cap table needs its region offsets");
        const std::uint32_t n_reg = region_offsets[n_refs];
        if (n_reg && (!region_starts || !region_ends || !region_caps))
            throw std::invalid_argument("a cap table with regions needs their starts, ends and caps");
        bam_api::BamApi api(in_path, cfg);
        const std::vector<std::uint32_t> offs(region_offsets, region_offsets + n_refs + 1);
        const std::vector<std::uint32_t> rs(region_starts, region_starts + n_reg), re(region_ends, region_ends + n_reg),
            caps(region_caps, region_caps + n_reg);
        std::vector<bam_api::BAMReadId> kept = hip->solve_templates_profile(max_coverage, api, offs, rs, re, caps, default_cap);
        if (tstats) *tstats = hip->last_template_stats();
        if (qstats) *qstats = hip->last_template_profile_stats();
        const std::uint32_t written = api.write_records(out_path, kept);
        if (filtered_path && filtered_path[0]) api.write_bam_api_filtered_out_reads(filtered_path);
        return (std::int64_t)written;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// BamApiConfig's rule for targets, without a solve: 0 when BamApi accepts {per_reference, targets, padding}, -4 with its
// message otherwise (targets without per_reference, an unknown chrom, a malformed line)
std::int64_t qmcp_host_check_targets_config(const char* in_path, const char* targets, int per_reference,
                                            std::uint32_t target_padding, std::uint64_t* n_regions, char* err,
                                            std::size_t err_cap) {
    bam_api::BamApiConfig cfg;
    cfg.per_reference = per_reference != 0;
    if (targets && targets[0]) cfg.targets_filepath = targets;
    cfg.target_padding = target_padding;
    try {
        bam_api::BamApi api(in_path, cfg);
        if (n_regions) *n_regions = api.has_targets() ? api.get_targets().starts.size() : 0;
        return 0;
    } catch (const std::bad_alloc&) {
        return -3;
    } catch (const std::invalid_argument& e) {
        copy_err(e.what(), err, err_cap);
        return -4;
    }
}

// The span the reference times as "solve took" (src/app.cpp:132-139) at the plugin boundary: a BamApi
// that already holds the reads as SOAPairedReads (size_t columns) -> solver.solve(M, api) -> Solution.
// Building the BamApi is outside the span, as parsing the BAM is in the reference.  `times` receives
// {wall of solve(), library total, narrow + H2D, device solve, D2H, mask expansion, threads, chunks,
// columns sent};
// returns the number of kept reads (kept_out may be NULL), negative on an unknown solver.
std::int64_t qmcp_host_plugin_solve_timed(const char* solver_name, const std::uint32_t* starts,
                                          const std::uint32_t* ends, std::uint64_t n,
                                          std::uint32_t ref_genome_length, std::uint32_t max_coverage,
                                          std::uint64_t* kept_out, float* times) {
    qmcp::Solver* found = resolve(solver_name);
    if (found == nullptr) return -1;
    bam_api::SOAPairedReads soa;
    soa.ref_genome_length = ref_genome_length;
    soa.reserve(n);
    for (std::uint64_t i = 0; i < n; ++i)
        soa.push_back(bam_api::Read(i, starts[i], ends[i], 0, ends[i] - starts[i] + 1, i % 2 == 0));
    bam_api::BamApi api(soa);
    qmcp::Solver& solver = *found;
    const auto t0 = std::chrono::steady_clock::now();
    auto solution = solver.solve(max_coverage, api);
    const float wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (times) {
        for (int i = 0; i < 9; ++i) times[i] = 0.f;
        times[0] = wall;
        if (auto* hip = dynamic_cast<qmcp::QuasiMcpHipSolver*>(&solver)) {
            const qmcp_hip_host_breakdown& b = hip->last_breakdown();
            times[1] = b.ms_total; times[2] = b.ms_narrow_h2d; times[3] = b.ms_solve; times[4] = b.ms_d2h;
            times[5] = hip->last_expand_ms(); times[6] = (float)b.host_threads; times[7] = (float)b.chunks;
            times[8] = (float)b.columns_sent;
        }
    }
    if (kept_out) for (std::size_t i = 0; i < solution->size(); ++i) kept_out[i] = (*solution)[i];
    return static_cast<std::int64_t>(solution->size());
}

}  // extern "C"
