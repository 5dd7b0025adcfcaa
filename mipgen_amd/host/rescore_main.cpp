// mipgen_rescore — features and scores of the probes of EXISTING MIP tables, from their own sequence columns, on the device through
// mipgen_accel_score_probes.  A table is what print_details writes (mipgen.cpp:765-794: all_mips / collapsed_mips / picked_mips / snp_mips, this front
// end's or the reference's): its ext_probe_sequence, lig_probe_sequence, scan_target_sequence, mip_sequence and copy columns are everything the two
// scorers read of a probe, so no BED, no bwa tables, no masks and no SNP maps are needed.
//
//   mipgen_rescore [-score_method logistic|svr] [-model mipgen_svr.model] [-bwa_genome_index ref.fa | -genome_dir dir] [-max_capture_size n]
//                  [-feature_flank n] [-o rescored.txt] [-features rows.libsvm [-labels table.tsv]] mip_table [mip_table ...]
//
//   -o         the input rows unchanged except for the score column (printed as the reference prints a score, mipgen.cpp:774), header word
//              logistic_score / svr_score set to the method; several inputs follow one another, each with its header
//   -features  one libsvm row per probe (non-zero features, the format mipgen_svr_train / mipgen_svr_cv read: svr_problem.hpp); the label is the
//              value -labels gives for the row's mip_key or mip_name (tab separated), without -labels the row's existing score
// The long-range content (features 22-65: svr scores and -features) is rebuilt per row from its chr, feature_start_position and
// feature_stop_position columns as the design built it (mipgen.cpp:1114-1129, 1214-1225; Featurev5::get_long_range_content): the flanked feature
// +/- max_capture_size (+14 / +15) +/- 1000 bases, through the input stage's own sequence loaders - so the design's -max_capture_size, -feature_flank
// and genome option have to be given again.  Arguments are checked and every file is parsed before the device is opened; any error ends with a
// message and exit status 1.
#include <map>
#include <string>

#include "mip_table.hpp"

static const char* PROG = "mipgen_rescore";
static int usage(const std::string& msg)
{
    if (!msg.empty()) fprintf(stderr, "mipgen_rescore: %s\n", msg.c_str());
    fprintf(stderr,
            "Usage: mipgen_rescore [options] mip_table [mip_table ...]\n"
            "-score_method logistic|svr : scoring model (default logistic)\n"
            "-model file : libsvm model for svr (default: mipgen_svr.model beside the program)\n"
            "-bwa_genome_index ref.fa | -genome_dir dir : the design's genome, for the long-range content (svr, -features)\n"
            "-max_capture_size n, -feature_flank n : the design's values (long-range content)\n"
            "-o file : the tables with the score column re-derived\n"
            "-features file : libsvm training rows, one per probe; -labels table.tsv : mip_key or mip_name <tab> value\n");
    return 1;
}

// a score as the reference prints it: `ss << mip->score`, default ostream formatting = six significant digits (mipgen.cpp:774); "-nan" is what its
// inf - inf prints as on x86-64
static std::string print_score(double s)
{
    char sc[48];
    if (std::isnan(s)) snprintf(sc, sizeof sc, "-nan"); else snprintf(sc, sizeof sc, "%g", s);
    return sc;
}

int main(int argc, char** argv)
{
    mipgen::Options o;
    o.write_feature_fasta = false;
    o.score_method = MIPGEN_SCORE_LOGISTIC;
    std::string model_path, out_path, feat_path, label_path, genome_dir;
    bool have_max_capture = false;
    int flank = 0;
    std::vector<std::string> inputs;
    {
        const std::string a0(argv[0]);
        const size_t e = a0.find_last_of('/');
        model_path = (e == std::string::npos ? std::string() : a0.substr(0, e + 1)) + "mipgen_svr.model";      // beside the program, as mipgen finds it (mipgen.cpp:137-138, 409)
    }
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a.empty() || a[0] != '-') { inputs.push_back(a); continue; }
        if (i + 1 >= argc) return usage("option " + a + " needs a value");
        const std::string v = argv[++i];
        long iv;
        if (a == "-score_method") {
            if (v == "logistic") o.score_method = MIPGEN_SCORE_LOGISTIC;
            else if (v == "svr") o.score_method = MIPGEN_SCORE_SVR;
            else return usage("-score_method must be logistic or svr");
        } else if (a == "-model") model_path = v;
        else if (a == "-bwa_genome_index") o.bwa_genome_index = v;
        else if (a == "-genome_dir") { genome_dir = v; o.args["-genome_dir"] = v; }
        else if (a == "-max_capture_size") { if (!svr_parse_int(v.c_str(), &iv) || iv <= 0 || iv > 1000000) return usage("bad value for -max_capture_size"); o.max_capture = (int)iv; have_max_capture = true; }
        else if (a == "-feature_flank" || a == "-feature_flanks") { if (!svr_parse_int(v.c_str(), &iv) || iv < 0 || iv > 1000000) return usage("bad value for " + a); flank = (int)iv; }
        else if (a == "-o") out_path = v;
        else if (a == "-features") feat_path = v;
        else if (a == "-labels") label_path = v;
        else return usage("unknown option: " + a);
    }
    const bool svr = o.score_method == MIPGEN_SCORE_SVR;
    const bool need_lrc = svr || !feat_path.empty();
    if (inputs.empty()) return usage("no MIP table");
    if (out_path.empty() && feat_path.empty()) return usage("nothing to do: give -o and / or -features");
    if (!label_path.empty() && feat_path.empty()) return usage("-labels goes with -features");
    if (need_lrc && o.bwa_genome_index.empty() && genome_dir.empty())
        return usage(std::string(svr ? "-score_method svr" : "-features") + " needs the long-range content of every row's feature: -bwa_genome_index <indexed fasta> or "
                     "-genome_dir <directory> is missing");
    if (need_lrc && !have_max_capture)
        return usage(std::string(svr ? "-score_method svr" : "-features") + " needs the long-range content of every row's feature: -max_capture_size is missing");
    o.feature_flank = flank;
    const int lrc_method = o.score_method;
    o.score_method = need_lrc ? MIPGEN_SCORE_SVR : MIPGEN_SCORE_LOGISTIC;         // (what makes the loaders keep the +/- 1000-base sequence)

    // ---- everything is read and checked before the device is opened ----
    std::vector<Table> tables(inputs.size());
    for (size_t k = 0; k < inputs.size(); k++) if (!read_table(PROG, inputs[k], flank, tables[k])) return 1;
    std::map<std::string, double> labels;
    if (!label_path.empty()) {
        std::ifstream fh(label_path);
        if (!fh.is_open()) { fprintf(stderr, "%s: can't open label table %s\n", PROG, label_path.c_str()); return 1; }
        std::string line;
        long lineno = 0;
        while (std::getline(fh, line)) {
            lineno++;
            if (line.empty() || line[0] == '#') continue;
            const std::vector<std::string> f = split_tabs(line);
            double y;
            if (f.size() != 2 || f[0].empty() || !svr_parse_double(f[1].c_str(), &y) || !std::isfinite(y)) {
                fprintf(stderr, "%s: %s:%ld: malformed label row (expected: mip_key or mip_name, tab, a finite number)\n", PROG, label_path.c_str(), lineno);
                return 1;
            }
            labels[f[0]] = y;
        }
        std::map<std::string, bool> used;
        for (const Table& t : tables) for (const auto& r : t.rows) { used[r[COL_KEY]] = true; used[r[COL_NAME]] = true; }
        for (const auto& kv : labels)
            if (!used.count(kv.first)) { fprintf(stderr, "%s: %s: label key '%s' names no probe of the given tables (neither a mip_key nor a mip_name)\n", PROG, label_path.c_str(), kv.first.c_str()); return 1; }
    }
    if (need_lrc)
        for (Table& t : tables) {
            if (t.features.empty()) continue;
            // the loaders walk a chromosome at a time (the reference reloads on every change, mipgen.cpp:1190): hand them the features in that order
            std::vector<size_t> order(t.features.size());
            for (size_t i = 0; i < order.size(); i++) order[i] = i;
            std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return t.features[a].chr < t.features[b].chr; });
            std::vector<mipgen::Region> regs;
            for (size_t i : order) regs.push_back(t.features[i]);
            const bool ok = genome_dir.empty() ? mipgen::load_sequences_from_indexed_fasta(o, regs) : mipgen::load_sequences_from_genome_dir(o, regs);
            if (!ok) { fprintf(stderr, "%s: %s: the sequences of its features could not be read from the genome\n", PROG, t.path.c_str()); return 1; }
            for (size_t k = 0; k < order.size(); k++) t.features[order[k]] = std::move(regs[k]);
        }

    // ---- the device ----
    mipgen_accel* h = nullptr;
    if (svr_tool_handle(&h) != MIPGEN_OK) { fprintf(stderr, "%s: %s\n", PROG, mipgen_accel_last_error()); return 1; }
    auto die = [&]() { fprintf(stderr, "%s: %s\n", PROG, mipgen_accel_last_error()); mipgen_accel_destroy(h); return 1; };
    if (svr && mipgen_accel_load_model_file(h, model_path.c_str()) != MIPGEN_OK) return die();
    FILE* out = nullptr;
    FILE* feat = nullptr;
    if (!out_path.empty() && !(out = fopen(out_path.c_str(), "w"))) { fprintf(stderr, "%s: can't write %s\n", PROG, out_path.c_str()); mipgen_accel_destroy(h); return 1; }
    if (!feat_path.empty() && !(feat = fopen(feat_path.c_str(), "w"))) { fprintf(stderr, "%s: can't write %s\n", PROG, feat_path.c_str()); mipgen_accel_destroy(h); return 1; }
    long n_unlabelled = 0, n_not_finite = 0, n_rows_written = 0;
    for (Table& t : tables) {
        const int32_t n = (int32_t)t.rows.size(), nf = (int32_t)t.features.size();
        std::vector<double> lrc((size_t)std::max(nf, 1) * MIPGEN_N_LRC, 0.0);
        if (need_lrc && nf > 0) {                                                     // one call per file; rows of the same feature share a table row
            std::vector<const char*> seqs((size_t)nf);
            std::vector<int32_t> lens((size_t)nf), starts((size_t)nf), stops((size_t)nf);
            for (int32_t i = 0; i < nf; i++) {
                const mipgen::Region& r = t.features[(size_t)i];
                seqs[(size_t)i] = r.long_range_seq.data(); lens[(size_t)i] = (int32_t)r.long_range_seq.size();
                starts[(size_t)i] = r.seq_start; stops[(size_t)i] = r.seq_stop;       // the denominator of Featurev5.cpp:49,53
            }
            if (mipgen_accel_long_range_content_batch(h, nf, seqs.data(), lens.data(), starts.data(), stops.data(), lrc.data()) != MIPGEN_OK) return die();
        }
        std::vector<mipgen_probe> probes((size_t)std::max(n, 1));
        for (int32_t i = 0; i < n; i++) {
            const std::vector<std::string>& r = t.rows[(size_t)i];
            mipgen_probe& q = probes[(size_t)i];
            q.ext_seq = r[COL_EXT_SEQ].c_str(); q.lig_seq = r[COL_LIG_SEQ].c_str(); q.ins_seq = r[COL_INS_SEQ].c_str(); q.mip_seq = r[COL_MIP_SEQ].c_str();
            q.ext_copy = (int32_t)atol(r[COL_EXT_COPY].c_str()); q.lig_copy = (int32_t)atol(r[COL_LIG_COPY].c_str());
            q.lrc_index = need_lrc ? t.feature[(size_t)i] : -1; q.reserved = 0;
        }
        std::vector<double> scores((size_t)std::max(n, 1)), x;
        if (feat) x.resize((size_t)std::max(n, 1) * MIPGEN_N_FEATURES);
        if (n > 0 && mipgen_accel_score_probes(h, probes.data(), n, need_lrc ? lrc.data() : nullptr, need_lrc ? nf : 0, lrc_method, out ? scores.data() : nullptr,
                                               feat ? x.data() : nullptr, nullptr) != MIPGEN_OK)
            return die();
        if (out) {
            std::vector<std::string> hf = split_tabs(t.header);
            hf[COL_SCORE] = svr ? "svr_score" : "logistic_score";
            // (fwrite: a field is written back byte for byte - the reference prints an uninitialised masking_failed where mapping failed, mipgen.cpp:615-625,
            // 791, and that byte may be a NUL)
            auto put = [&](const std::string& s, size_t c) { if (c) fputc('\t', out); fwrite(s.data(), 1, s.size(), out); };
            for (size_t c = 0; c < hf.size(); c++) put(hf[c], c);
            fputc('\n', out);
            for (int32_t i = 0; i < n; i++) {
                const std::vector<std::string>& r = t.rows[(size_t)i];
                for (size_t c = 0; c < r.size(); c++) put(c == COL_SCORE ? print_score(scores[(size_t)i]) : r[c], c);
                fputc('\n', out);
            }
        }
        if (feat)
            for (int32_t i = 0; i < n; i++) {
                const std::vector<std::string>& r = t.rows[(size_t)i];
                const double* row = x.data() + (size_t)i * MIPGEN_N_FEATURES;
                double y = 0;
                if (!label_path.empty()) {
                    auto it = labels.find(r[COL_KEY]);
                    if (it == labels.end()) it = labels.find(r[COL_NAME]);
                    if (it == labels.end()) { n_unlabelled++; continue; }
                    y = it->second;
                } else if (!svr_parse_double(r[COL_SCORE].c_str(), &y) || !std::isfinite(y)) { n_unlabelled++; continue; }
                bool finite = true;
                for (int j = 0; j < MIPGEN_N_FEATURES; j++) finite = finite && std::isfinite(row[j]);
                if (!finite) { n_not_finite++; continue; }                            // log10 of a copy number <= 0: no training row (svr_read_problem refuses it)
                svr_write_row(feat, y, row);
                n_rows_written++;
            }
    }
    if (out && fclose(out) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, out_path.c_str()); mipgen_accel_destroy(h); return 1; }
    if (feat) {
        if (fclose(feat) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, feat_path.c_str()); mipgen_accel_destroy(h); return 1; }
        fprintf(stderr, "%s: %ld training rows written, %ld probes without a label skipped, %ld probes with a non-finite feature skipped\n", PROG, n_rows_written,
                n_unlabelled, n_not_finite);
    }
    mipgen_accel_destroy(h);
    return 0;
}
