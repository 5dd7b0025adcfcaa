// mip_table.hpp — the reader of MIP tables (what print_details writes, mipgen.cpp:765-794: all_mips / collapsed_mips / picked_mips / snp_mips) that
// mipgen_rescore and mipgen_count share: the columns, a parsed table, and read_table, which names file and line of a malformed row.
#pragma once
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "mipgen_host.hpp"
#include "svr_problem.hpp"

enum { COL_KEY = 0, COL_SCORE = 1, COL_CHR = 2, COL_EXT_START = 3, COL_EXT_STOP = 4, COL_EXT_COPY = 5, COL_EXT_SEQ = 6, COL_LIG_START = 7, COL_LIG_STOP = 8, COL_LIG_COPY = 9,
       COL_LIG_SEQ = 10, COL_INS_SEQ = 13, COL_MIP_SEQ = 14, COL_FEAT_START = 15, COL_FEAT_STOP = 16, COL_STRAND = 17, COL_NAME = 19, N_COLS = 20 };

struct Table {
    std::string path, header;
    std::vector<std::vector<std::string>> rows;
    std::vector<int32_t> feature;                 // per row: index into `features`
    std::vector<mipgen::Region> features;         // distinct (chr, feature_start_position, feature_stop_position) in order of appearance
};

static inline std::vector<std::string> split_tabs(const std::string& s)
{
    std::vector<std::string> f;
    size_t a = 0;
    for (;;) {
        const size_t b = s.find('\t', a);
        f.push_back(s.substr(a, b == std::string::npos ? std::string::npos : b - a));
        if (b == std::string::npos) break;
        a = b + 1;
    }
    return f;
}

// prog: the program named in the messages; flank: the design's -feature_flank (the flanked feature of every row, for the long-range content)
static inline bool read_table(const char* PROG, const std::string& path, int flank, Table& t)
{
    std::ifstream fh(path);
    if (!fh.is_open()) { fprintf(stderr, "%s: can't open MIP table %s\n", PROG, path.c_str()); return false; }
    t.path = path;
    std::string line;
    if (!std::getline(fh, line) || line.compare(0, 9, ">mip_key\t") != 0 || split_tabs(line).size() != N_COLS ||
        split_tabs(line)[COL_SCORE].find("_score") == std::string::npos) {
        fprintf(stderr, "%s: %s: not a MIP table (the first line is not the \">mip_key ...\" header of %d columns)\n", PROG, path.c_str(), N_COLS);
        return false;
    }
    t.header = line;
    std::map<std::string, int32_t> seen;
    long lineno = 1;
    while (std::getline(fh, line)) {
        lineno++;
        if (line.empty()) continue;
        std::vector<std::string> f = split_tabs(line);
        auto bad = [&](const char* what) { fprintf(stderr, "%s: %s:%ld: malformed row (%s)\n", PROG, path.c_str(), lineno, what); return false; };
        if (f.size() != N_COLS) return bad(("expected " + std::to_string((int)N_COLS) + " tab-separated columns, found " + std::to_string(f.size())).c_str());
        long v;
        double d;
        if (!svr_parse_int(f[COL_EXT_COPY].c_str(), &v) || v < INT32_MIN || v > INT32_MAX) return bad("ext_probe_copy is not an integer");
        if (!svr_parse_int(f[COL_LIG_COPY].c_str(), &v) || v < INT32_MIN || v > INT32_MAX) return bad("lig_probe_copy is not an integer");
        if (f[COL_EXT_SEQ].empty() || f[COL_EXT_SEQ].size() > MIPGEN_MAX_OLIGO) return bad("ext_probe_sequence is empty or longer than 64 bases");
        if (f[COL_LIG_SEQ].empty() || f[COL_LIG_SEQ].size() > MIPGEN_MAX_OLIGO) return bad("lig_probe_sequence is empty or longer than 64 bases");
        if (!svr_parse_double(f[COL_SCORE].c_str(), &d)) return bad("the score is not a number");
        long fs, fe;
        if (!svr_parse_int(f[COL_FEAT_START].c_str(), &fs) || !svr_parse_int(f[COL_FEAT_STOP].c_str(), &fe) || fs < 0 || fe < fs || fe > INT32_MAX - 100000)
            return bad("feature_start_position / feature_stop_position are not a range");
        if (f[COL_CHR].empty()) return bad("chr is empty");
        const std::string key = f[COL_CHR] + "\t" + f[COL_FEAT_START] + "\t" + f[COL_FEAT_STOP];
        auto it = seen.find(key);
        if (it == seen.end()) {
            mipgen::Region r;                                                       // the Featurev5 the row was designed for (mipgen.cpp:788-789)
            r.chr = f[COL_CHR]; r.start = (int)fs + 1; r.stop = (int)fe;
            r.start_fl = r.start - flank; r.stop_fl = r.stop + flank;
            it = seen.emplace(key, (int32_t)t.features.size()).first;
            t.features.push_back(r);
        }
        t.feature.push_back(it->second);
        t.rows.push_back(std::move(f));
    }
    return true;
}

// Where the captured molecule M = ext_probe_sequence + scan_target_sequence + lig_probe_sequence of a row lies on the genome (1-based, as the table prints its
// coordinates).  On '+' M runs from ext_probe_start to lig_probe_stop; on '-' it is the reverse complement of lig_probe_start .. ext_probe_stop.  So base t of M
// is genome position ext_probe_start + t on '+' and ext_probe_stop - t on '-', where it shows the complement of the plus-strand base.
struct RowCoords { long ext_start, ext_stop, lig_start, lig_stop; bool minus; };

// read_table does not look at these columns (its checks stay what they were); a caller that needs them asks here.  false: *what names the column at fault
static inline bool row_coords(const std::vector<std::string>& f, RowCoords* c, const char** what)
{
    if (!svr_parse_int(f[COL_EXT_START].c_str(), &c->ext_start)) { *what = "ext_probe_start is not an integer"; return false; }
    if (!svr_parse_int(f[COL_EXT_STOP].c_str(), &c->ext_stop)) { *what = "ext_probe_stop is not an integer"; return false; }
    if (!svr_parse_int(f[COL_LIG_START].c_str(), &c->lig_start)) { *what = "lig_probe_start is not an integer"; return false; }
    if (!svr_parse_int(f[COL_LIG_STOP].c_str(), &c->lig_stop)) { *what = "lig_probe_stop is not an integer"; return false; }
    if (f[COL_STRAND] != "+" && f[COL_STRAND] != "-") { *what = "probe_strand is neither + nor -"; return false; }
    c->minus = f[COL_STRAND] == "-";
    return true;
}
