// locus_plan.hpp — the plan that folds the template positions of a MIP table into genome loci, for `mipgen_count -pileup_loci`: which locus every
// template position x of every table row contributes to, with the strand flag and the insertion rule, the loci in genome terms and their plus-strand ref bytes.
// The device does not know what an arm is: the arms are left out (or kept) HERE.  Nothing but the standard library is included, so a test can compile it alone.
#pragma once
#include <cctype>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace locus {

// what the builder takes of one table row: its RowCoords (ext_probe_start, ext_probe_stop and the strand are the ones the coordinate rule of 4.12 reads), the arm
// lengths and M = ext_probe_sequence + scan_target_sequence + lig_probe_sequence as the table has it
struct Row {
    std::string chr;
    long ext_start = 0, ext_stop = 0;
    bool minus = false;
    size_t n_ext = 0, n_lig = 0;         // M[0, n_ext) is the extension arm, the last n_lig bases the ligation arm, the target lies between
    std::string mol;
};

struct Plan {
    std::vector<int64_t> plan;           // per template position: -1, or locus * 4 + (minus ? 1 : 0) + (minus and t >= 1 ? 2 : 0)
    std::vector<std::string> chroms;     // in order of first appearance in the table
    std::vector<int32_t> locus_chr;      // per locus: index into chroms
    std::vector<long> locus_pos;         // per locus: 1-based genome position
    std::string locus_ref;               // per locus: the upper-case plus-strand base
    std::vector<int32_t> sources;        // per locus: the template positions that contribute to it
};

// two sources give one locus different refs: the 0-based table rows, first the earlier source
struct Conflict { size_t row_a = 0, row_b = 0; char ref_a = 0, ref_b = 0; std::string chr; long position = 0; };

static inline char plus_ref(char c, bool minus)
{
    c = (char)toupper((unsigned char)c);
    if (!minus) return c;
    return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
}

// all_parts: the arms contribute too (-loci_parts all); else the target only.  false: *bad names the conflict, *out is unspecified.
static inline bool build_plan(const std::vector<Row>& rows, bool all_parts, Plan* out, Conflict* bad)
{
    *out = Plan();
    std::map<std::string, int32_t> rank;
    for (const Row& r : rows)
        if (rank.emplace(r.chr, (int32_t)out->chroms.size()).second) out->chroms.push_back(r.chr);
    auto included = [&](const Row& r, size_t t) { return all_parts || (t >= r.n_ext && t + r.n_lig < r.mol.size()); };
    auto position = [](const Row& r, size_t t) { return r.minus ? r.ext_stop - (long)t : r.ext_start + (long)t; };
    struct First { size_t row; char ref; int64_t locus; };
    std::map<std::pair<int32_t, long>, First> loci;                     // ordered by (chromosome rank, position): the locus order
    for (size_t i = 0; i < rows.size(); i++) {
        const Row& r = rows[i];
        const int32_t c = rank[r.chr];
        for (size_t t = 0; t < r.mol.size(); t++) {
            if (!included(r, t)) continue;
            const char ref = plus_ref(r.mol[t], r.minus);
            auto at = loci.emplace(std::make_pair(c, position(r, t)), First{i, ref, 0});
            if (!at.second && at.first->second.ref != ref) {
                *bad = Conflict{at.first->second.row, i, at.first->second.ref, ref, r.chr, position(r, t)};
                return false;
            }
        }
    }
    int64_t n_loci = 0;
    for (auto& kv : loci) {
        kv.second.locus = n_loci++;
        out->locus_chr.push_back(kv.first.first); out->locus_pos.push_back(kv.first.second); out->locus_ref.push_back(kv.second.ref);
    }
    out->sources.assign((size_t)n_loci, 0);
    for (const Row& r : rows) {
        const int32_t c = rank[r.chr];
        for (size_t t = 0; t < r.mol.size(); t++) {
            if (!included(r, t)) { out->plan.push_back(-1); continue; }
            const int64_t l = loci.find(std::make_pair(c, position(r, t)))->second.locus;
            out->sources[(size_t)l]++;
            out->plan.push_back(l * 4 + (r.minus ? 1 : 0) + (r.minus && t >= 1 ? 2 : 0));
        }
    }
    return true;
}

}  // namespace locus
