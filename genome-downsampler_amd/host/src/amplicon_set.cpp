#include "bam-api/amplicon_set.hpp"

#include <algorithm>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>

namespace bam_api {

bool read_primer_bed(const std::filesystem::path& path, PrimerMap& out) {
    std::ifstream file(path);
    if (!file.is_open()) return false;
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream fields(line);
        std::string chrom, start, end, name;
        std::getline(fields, chrom, '\t');
        std::getline(fields, start, '\t');
        std::getline(fields, end, '\t');
        std::getline(fields, name, '\t');
        Index s = 0, e = 0;
        try {
            s = std::stoull(start);
            e = std::stoull(end);
        } catch (const std::invalid_argument&) {
            continue;
        } catch (const std::out_of_range&) {
            continue;
        }
        if (chrom.empty() || start.empty() || end.empty() || name.empty()) continue;
        out.emplace(name, std::make_pair(s, e));  // emplace: an existing name is kept
    }
    return true;
}

bool read_primer_pairs_tsv(const std::filesystem::path& path,
                           std::vector<std::pair<std::string, std::string>>& out) {
    std::ifstream file(path);
    if (!file.is_open()) return false;
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream fields(line);
        std::string left, right;
        std::getline(fields, left, '\t');
        std::getline(fields, right, '\t');
        if (!left.empty() && !right.empty()) out.emplace_back(left, right);
    }
    return true;
}

AmpliconSet build_amplicon_set(PrimerMap primers,
                               const std::vector<std::pair<std::string, std::string>>* pairs) {
    AmpliconSet set;
    auto add = [&set](std::pair<Index, Index>& left, std::pair<Index, Index>& right) {
        if (left.first > right.first) std::swap(left, right);
        set.amplicons.emplace_back(left.first, right.second);
    };
    if (pairs != nullptr) {
        for (const auto& names : *pairs) add(primers[names.first], primers[names.second]);
    } else {
        // an odd trailing primer has no partner (the reference walks past the end there)
        for (auto it = primers.begin(); it != primers.end();) {
            auto& left = it->second;
            if (++it == primers.end()) break;
            add(left, it->second);
            ++it;
        }
    }
    return set;
}

bool amplicon_set_from_files(const std::filesystem::path& bed, const std::filesystem::path& tsv,
                             AmpliconSet& out) {
    PrimerMap primers;
    if (!read_primer_bed(bed, primers)) return false;
    if (tsv.empty()) {
        out = build_amplicon_set(std::move(primers), nullptr);
        return true;
    }
    std::vector<std::pair<std::string, std::string>> pairs;
    if (!read_primer_pairs_tsv(tsv, pairs)) return false;
    out = build_amplicon_set(std::move(primers), &pairs);
    return true;
}

bool read_primer_bed_by_chrom(const std::filesystem::path& path, ChromPrimerMap& out, std::vector<std::string>& chroms) {
    std::ifstream file(path);
    if (!file.is_open()) return false;
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream fields(line);
        std::string chrom, start, end, name;
        std::getline(fields, chrom, '\t');
        std::getline(fields, start, '\t');
        std::getline(fields, end, '\t');
        std::getline(fields, name, '\t');
        Index s = 0, e = 0;
        try {
            s = std::stoull(start);
            e = std::stoull(end);
        } catch (const std::invalid_argument&) {
            continue;
        } catch (const std::out_of_range&) {
            continue;
        }
        if (chrom.empty() || start.empty() || end.empty() || name.empty()) continue;
        if (std::find(chroms.begin(), chroms.end(), chrom) == chroms.end()) chroms.push_back(chrom);
        out.emplace(name, ChromPrimer{chrom, s, e});  // emplace: an existing name is kept
    }
    return true;
}

bool build_reference_amplicon_set(ChromPrimerMap primers, const std::vector<std::string>& chroms,
                                  const std::vector<std::pair<std::string, std::string>>* pairs,
                                  const std::vector<std::string>& ref_names, ReferenceAmpliconSet& out,
                                  std::string* err) {
    auto fail = [err](const std::string& msg) {
        if (err) *err = msg;
        return false;
    };
    std::map<std::string, std::uint32_t> ref_of;
    for (std::size_t r = 0; r < ref_names.size(); ++r) ref_of.emplace(ref_names[r], (std::uint32_t)r);
    for (const std::string& chrom : chroms)
        if (ref_of.find(chrom) == ref_of.end())
            return fail("BED chrom \"" + chrom + "\" names no reference of the BAM file (names must match exactly)");
    // an amplicon with what the primer-clipped entries need besides its bounds: the insert [left.end, right.start - 1]
    // (the BED end is exclusive) and the left primer's name
    struct Paired {
        Amplicon amplicon;
        Index insert_start, insert_end;  // insert_start > insert_end: the primers touch or overlap
        std::string left_name, right_name;
    };
    std::vector<std::vector<Paired>> per(ref_names.size());
    auto paired = [](const ChromPrimer& left, const ChromPrimer& right, const std::string& ln, const std::string& rn) {
        const bool empty = right.start == 0 || left.end > right.start - 1;
        return Paired{Amplicon(left.start, right.end), empty ? 1 : left.end, empty ? 0 : right.start - 1, ln, rn};
    };
    if (pairs != nullptr) {
        for (const auto& names : *pairs) {
            const auto il = primers.find(names.first), ir = primers.find(names.second);
            if (il == primers.end() && ir == primers.end())
                return fail("TSV pair " + names.first + " / " + names.second + " names no primer of the BED");
            const std::string chrom = il != primers.end() ? il->second.chrom : ir->second.chrom;
            ChromPrimer& left = primers[names.first];  // (a missing name: a (0, 0) primer on the other's chrom)
            if (left.chrom.empty()) left.chrom = chrom;
            ChromPrimer& right = primers[names.second];
            if (right.chrom.empty()) right.chrom = chrom;
            if (left.chrom != right.chrom)
                return fail("TSV pair " + names.first + " / " + names.second + " crosses references: " + names.first +
                            " on " + left.chrom + ", " + names.second + " on " + right.chrom);
            const bool swapped = left.start > right.start;
            if (swapped) std::swap(left, right);
            per[ref_of[left.chrom]].push_back(paired(left, right, swapped ? names.second : names.first,
                                                     swapped ? names.first : names.second));
        }
    } else {
        // name order within each chrom: the primers map is in name order already
        std::map<std::string, std::vector<const ChromPrimerMap::value_type*>> by_chrom;
        for (const auto& kv : primers) by_chrom[kv.second.chrom].push_back(&kv);
        for (const auto& kv : by_chrom) {
            const auto& v = kv.second;
            std::vector<Paired>& dst = per[ref_of[kv.first]];
            for (std::size_t i = 0; i + 1 < v.size(); i += 2) {
                const auto* left = v[i];
                const auto* right = v[i + 1];
                if (left->second.start > right->second.start) std::swap(left, right);
                dst.push_back(paired(left->second, right->second, left->first, right->first));
            }
        }
    }
    out = ReferenceAmpliconSet();
    for (const auto& v : per) {
        for (const Paired& a : v) {
            out.starts.push_back(a.amplicon.start);
            out.ends.push_back(a.amplicon.end);
            out.insert_starts.push_back(a.insert_start);
            out.insert_ends.push_back(a.insert_end);
            out.left_names.push_back(a.left_name);
            if (a.insert_start > a.insert_end && out.empty_insert.empty())
                out.empty_insert = "primer pair " + a.left_name + " / " + a.right_name +
                                   " leaves no insert: the primers touch or overlap";
        }
        out.offsets.push_back((std::uint32_t)out.starts.size());
    }
    return true;
}

bool reference_amplicon_set_from_files(const std::filesystem::path& bed, const std::filesystem::path& tsv,
                                       const std::vector<std::string>& ref_names, ReferenceAmpliconSet& out,
                                       std::string* err) {
    ChromPrimerMap primers;
    std::vector<std::string> chroms;
    if (!read_primer_bed_by_chrom(bed, primers, chroms)) {
        if (err) *err = "could not open " + bed.string();
        return false;
    }
    if (tsv.empty()) return build_reference_amplicon_set(std::move(primers), chroms, nullptr, ref_names, out, err);
    std::vector<std::pair<std::string, std::string>> pairs;
    if (!read_primer_pairs_tsv(tsv, pairs)) {
        if (err) *err = "could not open " + tsv.string();
        return false;
    }
    return build_reference_amplicon_set(std::move(primers), chroms, &pairs, ref_names, out, err);
}

}  // namespace bam_api
