// mipgen_count — the "measure" link of design -> measure -> featurize -> cross-validate -> train -> design: reads and unique molecular tags per
// probe of MIP tables from the FASTQ files of a capture, on the device through mipgen_accel_reads_open / _feed / _finish.  No
// aligner: a smMIP read pair starts, after its tag, with the probe's own arm sequences.
//
//   mipgen_count [-tag_sizes 5,0] [-mismatches 0] [-swap_reads] [-label tags|reads|log10tags] -o counts.tsv [-labels labels.tsv]
//                -reads ext.fq lig.fq  mip_table [mip_table ...]
//
//   -reads     the extension-read file and the ligation-read file (plain FASTQ, four lines per record, pairs in the same order);
//              -swap_reads: the first file holds the ligation reads
//   -o         "mip_key <tab> mip_name <tab> reads <tab> unique_tags" under a header line of those words, one row per probe in table order
//   -labels    "mip_key <tab> value", the file `mipgen_rescore -features ... -labels` reads: unique_tags (tags, the default), reads, or
//              log10(unique_tags + 1) printed with %.17g (log10tags)
//   stderr     "mipgen_count: pairs P assigned A ambiguous B unassigned U tag_n T overflow O"
// Per sample of a multiplexed lane (without -barcodes every line written is what it was):
//   -barcodes samples.tsv   "label <tab> sequence" per sample (blank lines skipped): barcodes of one length (at most 32), upper-case A C G T, distinct;
//                           labels distinct and not "undetermined"
//   -index_reads i1.fq[,i2.fq]  the index read of every pair, in the order of -reads; -index_length j1[,j2]: the pair's index is the first j1 bases
//                           of i1 followed by the first j2 of i2 (one file: j1 defaults to the barcode length; two files: required, j1 + j2 = barcode
//                           length); an index read shorter than its j leaves the pair without a sample
//   -barcode_mismatches 0|1 substitutions allowed between index and barcode (default 0)
//   -o         then "sample <tab> mip_key <tab> mip_name <tab> reads <tab> unique_tags", one line per cell with reads > 0: samples in file order,
//              "undetermined" last, probes in table order
//   -samples   "sample <tab> barcode <tab> pairs <tab> assigned <tab> unique_tags <tab> probes_seen" under a header line of those words, one line per
//              sample, always; the last line is "undetermined" with barcode "*"
//   -labels    the value per probe over the NAMED samples: reads and unique tags summed over their rows (molecules of different samples are different
//              molecules), log10tags of that sum
//   stderr     a second line: "mipgen_count: samples N sample_none X sample_ambiguous Y"
// One consensus read per molecule (without -consensus every byte written is what it was):
//   -consensus PREFIX       PREFIX.ext.fq and PREFIX.lig.fq: per (sample, probe, tag) group the quality-weighted consensus of its extension reads and of its
//                           ligation reads, each behind its tag, in ascending (sample, probe, tag) order.  Header: "@smc<ordinal> <sample label | * without
//                           -barcodes | undetermined> <tab> mip_key <tab> tag <tab> family"; the ordinal is the group's place among ALL groups, from 0
//   -min_family k           only the groups of at least k pairs are written (default 1)
//   stderr     a last line: "mipgen_count: consensus groups G written W members M" (M: the pairs of all G groups)
// Allele counts per captured base (without -pileup every byte written is what it was):
//   -pileup FILE            per (sample, probe, template position) the molecules that show A, C, G, T there and those whose two reads disagree, from the consensus
//                           reads (a consensus session is opened whether or not -consensus is given); needs tag bases.  Header
//                           ">sample <tab> mip_key <tab> chr <tab> position <tab> strand <tab> part <tab> ref <tab> A <tab> C <tab> G <tab> T <tab> discordant"; one line
//                           per position with a non-zero counter, in sample, table and position order; part = ext | target | lig.  Everything is in genome PLUS
//                           orientation: on a '-' probe position = ext_probe_stop - t, ref is the complement of the molecule's base and A/T, C/G swap columns
//   -pileup_min_family k    only molecules of at least k pairs count (default 1); -pileup_min_quality q: only consensus bases of quality >= q, 0..40 (default 0)
//   stderr     a last line: "mipgen_count: pileup molecules U positions P bases B nonref R discordant D" (U: the molecules counted; P: lines written)
//   -pileup_indels W        place every consensus read on its template by a banded alignment of at most W (1..15) inserted or deleted bases first: the
//                           header and every line gain the columns del, ins and ins_discordant (molecules that show a deletion of the base; an insertion between
//                           this base and the next one in genome plus orientation; two different insertion lengths there), a line is written when any of its eight
//                           numbers is non-zero, and a second stderr line follows: "mipgen_count: pileup indels deletions X insertions Y ins_discordant Z gapped_sides S"
//   -pileup_insertions INS  needs -pileup_indels: the inserted bases themselves.  One insertions call per row (undetermined too) feeds BOTH files - FILE is
//                           byte for byte what it is without the option; beside -call or -pileup_loci those routes run unchanged and the insertions call of a row feeds
//                           INS only.  Header ">sample <tab> mip_key <tab> chr <tab> position <tab> strand <tab> length <tab> inserted <tab> count <tab> span <tab> ppm";
//                           one line per allele in row order, then table order, then the order of the records.  position is the lower genome coordinate of the two
//                           bases the insertion lies between, on both strands; inserted is in genome plus orientation (reverse-complemented on a '-' probe) and
//                           `length` times N for the molecules whose inserted bases could not be told; span = the molecules that cover the anchor with one agreed
//                           length, 0 included; ppm = floor(count 10^6 / span)
//   stderr     a last line: "mipgen_count: insertion alleles A events I ambiguous B span S"
//   -pileup_deletions DEL   needs -pileup_indels: the deletions as events, start and length per molecule.  One deletions call per row (undetermined too)
//                           feeds DEL only - a second count of the row beside whatever feeds FILE; FILE and every other file are byte for byte what they are without
//                           the option.  Header ">sample <tab> mip_key <tab> chr <tab> position <tab> strand <tab> length <tab> deleted <tab> ragged <tab> count <tab>
//                           depth <tab> ppm"; one line per allele in row order, then table order, then the order of the records.  position is the LOWEST genome
//                           coordinate of the deleted bases, on both strands; deleted is the template's bytes in genome plus orientation (reverse-complemented on a
//                           '-' probe); ragged = 1 where the two reads of the molecules disagree on the extent; depth = the molecules that vote A C G T or del at
//                           the first deleted base; ppm = floor(count 10^6 / depth)
//   stderr     a last line: "mipgen_count: deletion alleles A events E ragged R deleted_bases B"
//   -call_insertions ICALLS needs -pileup_insertions: the insertion alleles of every row called against a background of the other samples, under the
//                           -call_* options.  One pool call, then one insertion call per row (undetermined too) that takes the place of the insertions call: FILE
//                           and INS are byte for byte what they are without the option.  Header ">sample <tab> mip_key <tab> chr <tab> position <tab> strand <tab>
//                           length <tab> inserted <tab> depth <tab> alt_count <tab> alt_ppm <tab> bg_alt <tab> bg_depth <tab> q"; one line per call in row, table and
//                           record order; position, strand and inserted as in INS; depth = the span of the anchor; alt_ppm = floor(alt_count 10^6 / depth)
//   stderr     a last line: "mipgen_count: insertion calls C candidates K tested P too_deep D"
// Variant calls from the pileup against a background of the other samples (without -call every byte written is what it was):
//   -call CALLS             needs -pileup and uses -pileup_min_family, -pileup_min_quality and -pileup_indels as given: one pool over the sample rows, then one call per
//                           row (undetermined too) that feeds BOTH files - FILE is byte for byte what it is without -call.  Header
//                           ">sample <tab> mip_key <tab> chr <tab> position <tab> strand <tab> part <tab> ref <tab> alt <tab> depth <tab> alt_count <tab> alt_ppm <tab>
//                           bg_alt <tab> bg_depth <tab> q"; one line per call in row, table and position order, within a position in the order A C G T - of the printed
//                           alt; genome plus orientation as in -pileup (ref and alt complemented on a '-' probe; a deleted base prints alt "-" on the line of that
//                           base); alt_ppm = floor(alt_count 10^6 / depth); bg_alt, bg_depth: the background without this row
//   -call_min_depth 20  -call_min_alt 3  -call_min_ppm 0  -call_min_q 30  -call_prior 1,1000  -call_background_max_ppm 200000     the parameters of the model
//   stderr     a last line: "mipgen_count: calls C candidates K tested P too_deep D"
// Pileup and calls per genome locus, merged over the probes that cover it (without these options every byte written is what it was):
//   -pileup_loci LOCI       needs -pileup: per (sample, genome base) the counts of -pileup summed over every probe whose template covers the base, minus-strand probes
//                           folded into plus orientation first.  Header ">sample <tab> chr <tab> position <tab> ref <tab> probes <tab> A <tab> C <tab> G <tab> T <tab>
//                           discordant" (and del, ins, ins_discordant under -pileup_indels); one line per (sample, locus) with a non-zero counter, samples in row order,
//                           loci by chromosome in order of first appearance in the tables, then by position; probes = the template positions that land on the locus
//   -loci_parts target|all  what of a probe contributes: its target only (the default: a read's arm bases are the probe oligo, not the sample) or the arms too.  Two
//                           probes that give one locus different ref bases are an error that names both table rows
//   -call_loci CALLS        needs -pileup_loci: the calls of -call made per locus on the merged counts - pool, leave-one-out, filters and score over loci - under the
//                           -call_* options, which now apply to -call, -call_loci or both.  Header ">sample <tab> chr <tab> position <tab> ref <tab> alt <tab> depth
//                           <tab> alt_count <tab> alt_ppm <tab> bg_alt <tab> bg_depth <tab> q <tab> probes"; a deleted base prints alt "-"
//   stderr     after the lines above: "mipgen_count: loci L lines P bases B nonref R discordant D" and, with -call_loci, "mipgen_count: locus calls C candidates K
//              tested P too_deep D"
// Insertion alleles per genome locus, folded over the probes that cover it (without these options every byte written is what it was):
//   -insertion_loci ILOCI   needs -pileup_insertions and -pileup_loci: the allele records of INS folded under the plan of LOCI - minus-strand probes turned into plus
//                           orientation, equal alleles of one locus added up, span the spanning molecules of every probe whose anchor lands there.  ONE more call per
//                           row (undetermined too), the locus insertions call, feeds ILOCI only: FILE, INS, ICALLS, LOCI and CALLS are byte for byte what they are
//                           without the option.  Header ">sample <tab> chr <tab> position <tab> length <tab> inserted <tab> count <tab> span <tab> ppm <tab> probes"; one
//                           line per locus allele in row order, then record order (locus, then allele key); chr, position and probes as LOCI prints them for the locus,
//                           which is the lower genome coordinate of the two bases the insertion lies between; inserted is in plus orientation, `length` times N for an
//                           ambiguous record; ppm = floor(count 10^6 / span).  A plus and a minus probe place an insertion inside a repeat at opposite ends of it: those
//                           stay two lines
//   -call_insertion_loci ILCALLS   needs -insertion_loci: the locus alleles of every row called against a background of the other samples, under the -call_* options.  One
//                           pool call, then the locus insertion call takes the place of the locus insertions call of every row and feeds ILOCI and ILCALLS.  Header
//                           ">sample <tab> chr <tab> position <tab> length <tab> inserted <tab> depth <tab> alt_count <tab> alt_ppm <tab> bg_alt <tab> bg_depth <tab> q
//                           <tab> probes"; the numbers as -call_insertions prints them
//   stderr     last lines: "mipgen_count: insertion loci L alleles A events I ambiguous B span S" (L: the loci of the plan) and, with -call_insertion_loci,
//              "mipgen_count: insertion locus calls C candidates K tested P too_deep D"
// Sequencing errors in molecular tags, corrected before the consensus (without -tag_mismatches 1 every byte written is what it was):
//   -tag_mismatches 0|1     1: the (sample, probe, tag) groups whose tags differ in one base are merged by the count rule - a group joins its neighbour of the largest
//                           family when that family is at least twice its own minus one, and larger - before anything is counted or voted.  The session then keeps its
//                           reads even without -consensus or -pileup (the rule needs family sizes), which costs the arena of DESIGN 4.11.  Every output carries the
//                           corrected groups: unique_tags in -o, -samples and -labels, the consensus FASTQ (the tag of the header is the corrected one, the family the
//                           merged one) and every pileup, call, locus and insertion file
//   -tag_map FILE           needs -tag_mismatches 1: "sample <tab> mip_key <tab> raw_tag <tab> raw_family <tab> tag" under a header line of those words, one line per RAW
//                           group in group order (sample, probe, raw tag), tags as bases, the sample as the consensus header writes it
//   stderr     after the lines above: "mipgen_count: tag_mismatches 1 raw R groups G absorbed A moved_pairs P max_depth D"
// Arguments are checked, the tables are parsed and both FASTQ files are read through once (record structure, equal record counts) before the
// device is opened: a malformed row or record names its file and line.  Then the reads stream to the device in chunks of at most 2^19 pairs, and a
// second thread reads and packs the next chunk while the device works on the current one.  Any error ends with a message and exit status 1.
#include <cctype>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

#include "locus_plan.hpp"
#include "mip_table.hpp"

static const char* PROG = "mipgen_count";
static const int64_t CHUNK_PAIRS = (int64_t)1 << 19;

static int usage(const std::string& msg)
{
    if (!msg.empty()) fprintf(stderr, "mipgen_count: %s\n", msg.c_str());
    fprintf(stderr,
            "Usage: mipgen_count [options] -o counts.tsv -reads ext.fq lig.fq mip_table [mip_table ...]\n"
            "-tag_sizes e,l : molecular tag bases at the head of the extension / ligation read (default 5,0; at most 16 in all)\n"
            "-mismatches n : substitutions allowed per arm, 0..2 (default 0)\n"
            "-swap_reads : the first file of -reads holds the ligation reads\n"
            "-o file : mip_key, mip_name, reads, unique_tags per probe\n"
            "-labels file : mip_key <tab> value for mipgen_rescore -labels; -label tags|reads|log10tags : the value (default tags)\n"
            "-barcodes samples.tsv : label <tab> barcode per sample: counts per sample (-o gains a sample column); needs -index_reads\n"
            "-index_reads i1.fq[,i2.fq] : the index reads of the pairs; -index_length j1[,j2] : bases taken from each (default: the barcode length)\n"
            "-barcode_mismatches n : substitutions allowed between index and barcode, 0 or 1 (default 0)\n"
            "-samples file : sample, barcode, pairs, assigned, unique_tags, probes_seen per sample\n"
            "-consensus prefix : prefix.ext.fq and prefix.lig.fq, one consensus read pair per (sample, probe, tag) group; -min_family k : groups of at least k pairs (default 1)\n"
            "-pileup file : A, C, G, T and discordant molecules per captured base, in genome plus orientation; -pileup_min_family k (default 1), -pileup_min_quality q, 0..40 (default 0)\n"
            "-pileup_indels W : with -pileup, place the reads with up to W (1..15) inserted or deleted bases first; adds the columns del, ins, ins_discordant\n"
            "-pileup_insertions file : with -pileup_indels, the inserted bases per anchor: length, bases, molecules, spanning molecules and ppm per allele\n"
            "-pileup_deletions file : with -pileup_indels, the deletions as events: start, length, deleted bases, ragged, molecules, depth at the first base and ppm per allele\n"
            "-call_insertions file : with -pileup_insertions, the insertion alleles of every sample called against the background of the others, under the -call_* options\n"
            "-call file : with -pileup, variant calls of every sample against the background of the others; -call_min_depth n (default 20), -call_min_alt k (3), -call_min_ppm p (0),\n"
            "    -call_min_q q, 0..9999 (30), -call_prior a,n : error prior a/n, 0 < a < n <= 2^30 (1,1000), -call_background_max_ppm p, 0..1000000 (200000)\n"
            "-pileup_loci file : with -pileup, the counts per genome base, summed over the probes that cover it; -loci_parts target|all : what of a probe counts (default target)\n"
            "-call_loci file : with -pileup_loci, the variant calls per genome base on the merged counts, under the -call_* options\n"
            "-insertion_loci file : with -pileup_insertions and -pileup_loci, the insertion alleles per genome base, folded over the probes that cover it\n"
            "-call_insertion_loci file : with -insertion_loci, the insertion alleles per genome base called against the background of the other samples, under the -call_* options\n"
            "-tag_mismatches 0|1 : 1 merges tags one base apart by family size before anything is counted (default 0); the reads are then kept on the device as for -consensus\n"
            "-tag_map file : with -tag_mismatches 1, sample, mip_key, raw_tag, raw_family and corrected tag per uncorrected group\n");
    return 1;
}

// one FASTQ file read record by record; an error names file and line
struct Fastq {
    std::string path;
    FILE* fp = nullptr;
    char* line = nullptr;
    size_t cap = 0;
    long lineno = 0;
    ~Fastq() { if (fp) fclose(fp); free(line); }
    bool open() { fp = fopen(path.c_str(), "r"); lineno = 0; return fp != nullptr; }
    // a line without its end-of-line bytes: its length, or -1 at the end of the file
    ssize_t get()
    {
        ssize_t n = getline(&line, &cap, fp);
        if (n < 0) return -1;
        lineno++;
        while (n > 0 && (line[n - 1] == '\n' || line[n - 1] == '\r')) n--;
        return n;
    }
    // 1: a record, its sequence appended to *seq (NULL: checked only) and its quality line to *qual (NULL: dropped); 0: end of file; -1: malformed
    // (message printed)
    int next(std::string* seq, std::string* qual = nullptr)
    {
        ssize_t n = get();
        if (n < 0) return 0;
        auto bad = [&](const char* what) { fprintf(stderr, "%s: %s:%ld: malformed FASTQ record (%s)\n", PROG, path.c_str(), lineno, what); return -1; };
        if (n == 0 || line[0] != '@') return bad("the header line does not start with '@'");
        if ((n = get()) < 0) { lineno++; return bad("the file ends after a header line"); }
        const ssize_t len = n;
        if (seq) seq->append(line, (size_t)len);
        if ((n = get()) < 0) { lineno++; return bad("the file ends after a sequence line"); }
        if (n == 0 || line[0] != '+') return bad("the third line of a record does not start with '+'");
        if ((n = get()) < 0) { lineno++; return bad("the file ends before the quality line"); }
        if (n != len) return bad("sequence and quality differ in length");
        if (qual) qual->append(line, (size_t)len);
        return 1;
    }
};

struct Chunk {
    std::string ext, lig, idx, ext_qual, lig_qual;          // (the qualities only with -consensus: they share the offsets of their bases)
    std::vector<int64_t> ext_off, lig_off, idx_off;
    int64_t n = 0;
    bool last = false, failed = false;
};

// "label <tab> sequence" per line; false with a message that names file and line
static bool read_barcodes(const std::string& path, std::vector<std::string>& labels, std::vector<std::string>& seqs)
{
    FILE* fp = fopen(path.c_str(), "r");
    if (!fp) { fprintf(stderr, "%s: can't open barcode file %s\n", PROG, path.c_str()); return false; }
    char* line = nullptr;
    size_t cap = 0;
    long lineno = 0;
    bool ok = true;
    auto bad = [&](const std::string& what) { fprintf(stderr, "%s: %s:%ld: %s\n", PROG, path.c_str(), lineno, what.c_str()); ok = false; };
    for (ssize_t n; ok && (n = getline(&line, &cap, fp)) >= 0;) {
        lineno++;
        while (n > 0 && (line[n - 1] == '\n' || line[n - 1] == '\r')) n--;
        const std::string l(line, (size_t)n);
        if (l.find_first_not_of(" \t") == std::string::npos) continue;
        const size_t tab = l.find('\t');
        if (tab == std::string::npos || tab == 0 || tab + 1 >= l.size() || l.find('\t', tab + 1) != std::string::npos) { bad("malformed line (expected label <tab> sequence)"); break; }
        const std::string label = l.substr(0, tab), seq = l.substr(tab + 1);
        if (label == "undetermined") { bad("the label undetermined is taken (it names the pairs without a sample)"); break; }
        if (seq.size() > 32) { bad("barcode of " + std::to_string(seq.size()) + " bases (at most 32)"); break; }
        if (!seqs.empty() && seq.size() != seqs[0].size()) {
            bad("barcode of " + std::to_string(seq.size()) + " bases, the first has " + std::to_string(seqs[0].size()) + " (barcodes of unequal length)");
            break;
        }
        const size_t q = seq.find_first_not_of("ACGT");
        if (q != std::string::npos) { bad("barcode " + seq + ": byte " + std::to_string(q + 1) + " is not one of upper-case A C G T"); break; }
        if (std::find(seqs.begin(), seqs.end(), seq) != seqs.end()) { bad("barcode " + seq + " is there twice"); break; }
        if (std::find(labels.begin(), labels.end(), label) != labels.end()) { bad("label " + label + " is there twice"); break; }
        labels.push_back(label); seqs.push_back(seq);
    }
    free(line);
    fclose(fp);
    if (ok && seqs.empty()) { fprintf(stderr, "%s: %s holds no barcode\n", PROG, path.c_str()); ok = false; }
    return ok;
}

static bool parse_int_list(const std::string& v, std::vector<long>& out)
{
    for (size_t a = 0;;) {
        const size_t c = v.find(',', a);
        long x;
        if (!svr_parse_int(v.substr(a, c == std::string::npos ? c : c - a).c_str(), &x)) return false;
        out.push_back(x);
        if (c == std::string::npos) return true;
        a = c + 1;
    }
}

int main(int argc, char** argv)
{
    int te = 5, tl = 0, mism = 0, bc_mism = 0;
    long min_family = 1, pile_family = 1, pile_quality = 0, pile_indels = 0;
    bool swap = false, bc_mism_given = false, min_family_given = false, pile_option_given = false;
    std::string consensus_prefix, pileup_path, call_path, ins_path, call_ins_path, del_path;
    mipgen_call_params call_prm{20, 3, 0, 30, 1, 1000, 200000};
    bool call_option_given = false, loci_parts_given = false, loci_all = false;
    std::string loci_path, call_loci_path, ins_loci_path, call_ins_loci_path, tag_map_path;
    int tag_mism = 0;
    std::string out_path, label_path, label_kind = "tags", reads_a, reads_b, barcode_path, samples_path, index_arg, index_len_arg;
    std::vector<std::string> inputs;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a.empty() || a[0] != '-') { inputs.push_back(a); continue; }
        if (a == "-swap_reads") { swap = true; continue; }
        if (a == "-reads") {
            if (i + 2 > argc - 1) return usage("option -reads needs two files");
            reads_a = argv[++i]; reads_b = argv[++i];
            continue;
        }
        if (i + 1 >= argc) return usage("option " + a + " needs a value");
        const std::string v = argv[++i];
        long iv;
        if (a == "-tag_sizes") {
            const size_t c = v.find(',');
            long e, l;
            if (c == std::string::npos || !svr_parse_int(v.substr(0, c).c_str(), &e) || !svr_parse_int(v.substr(c + 1).c_str(), &l) || e < 0 || l < 0 || e + l > 16)
                return usage("-tag_sizes takes two sizes e,l of at most 16 bases in all");
            te = (int)e; tl = (int)l;
        } else if (a == "-mismatches") { if (!svr_parse_int(v.c_str(), &iv) || iv < 0 || iv > 2) return usage("-mismatches must be 0, 1 or 2"); mism = (int)iv; }
        else if (a == "-label") { if (v != "tags" && v != "reads" && v != "log10tags") return usage("-label must be tags, reads or log10tags"); label_kind = v; }
        else if (a == "-o") out_path = v;
        else if (a == "-labels") label_path = v;
        else if (a == "-barcodes") barcode_path = v;
        else if (a == "-samples") samples_path = v;
        else if (a == "-index_reads") index_arg = v;
        else if (a == "-index_length") index_len_arg = v;
        else if (a == "-consensus") { if (v.empty()) return usage("-consensus takes a prefix"); consensus_prefix = v; }
        else if (a == "-min_family") { if (!svr_parse_int(v.c_str(), &min_family) || min_family < 1) return usage("-min_family must be 1 or more"); min_family_given = true; }
        else if (a == "-pileup") { if (v.empty()) return usage("-pileup takes a file"); pileup_path = v; }
        else if (a == "-pileup_min_family") { if (!svr_parse_int(v.c_str(), &pile_family) || pile_family < 1 || pile_family > INT32_MAX) return usage("-pileup_min_family must be 1 or more"); pile_option_given = true; }
        else if (a == "-pileup_min_quality") { if (!svr_parse_int(v.c_str(), &pile_quality) || pile_quality < 0 || pile_quality > 40) return usage("-pileup_min_quality must be 0 to 40"); pile_option_given = true; }
        else if (a == "-pileup_indels") { if (!svr_parse_int(v.c_str(), &pile_indels) || pile_indels < 1 || pile_indels > 15) return usage("-pileup_indels must be 1 to 15"); }
        else if (a == "-pileup_insertions") { if (v.empty()) return usage("-pileup_insertions takes a file"); ins_path = v; }
        else if (a == "-pileup_deletions") { if (v.empty()) return usage("-pileup_deletions takes a file"); del_path = v; }
        else if (a == "-call_insertions") { if (v.empty()) return usage("-call_insertions takes a file"); call_ins_path = v; }
        else if (a == "-call") { if (v.empty()) return usage("-call takes a file"); call_path = v; }
        else if (a == "-pileup_loci") { if (v.empty()) return usage("-pileup_loci takes a file"); loci_path = v; }
        else if (a == "-call_loci") { if (v.empty()) return usage("-call_loci takes a file"); call_loci_path = v; }
        else if (a == "-insertion_loci") { if (v.empty()) return usage("-insertion_loci takes a file"); ins_loci_path = v; }
        else if (a == "-call_insertion_loci") { if (v.empty()) return usage("-call_insertion_loci takes a file"); call_ins_loci_path = v; }
        else if (a == "-loci_parts") { if (v != "target" && v != "all") return usage("-loci_parts must be target or all"); loci_all = v == "all"; loci_parts_given = true; }
        else if (a == "-call_min_depth") { if (!svr_parse_int(v.c_str(), &iv) || iv < 1 || iv > INT32_MAX) return usage("-call_min_depth must be 1 or more"); call_prm.min_depth = (int32_t)iv; call_option_given = true; }
        else if (a == "-call_min_alt") { if (!svr_parse_int(v.c_str(), &iv) || iv < 1 || iv > INT32_MAX) return usage("-call_min_alt must be 1 or more"); call_prm.min_alt = (int32_t)iv; call_option_given = true; }
        else if (a == "-call_min_ppm") { if (!svr_parse_int(v.c_str(), &iv) || iv < 0 || iv > 1000000) return usage("-call_min_ppm must be 0 to 1000000"); call_prm.min_ppm = (int32_t)iv; call_option_given = true; }
        else if (a == "-call_min_q") { if (!svr_parse_int(v.c_str(), &iv) || iv < 0 || iv > 9999) return usage("-call_min_q must be 0 to 9999"); call_prm.min_q = (int32_t)iv; call_option_given = true; }
        else if (a == "-call_background_max_ppm") { if (!svr_parse_int(v.c_str(), &iv) || iv < 0 || iv > 1000000) return usage("-call_background_max_ppm must be 0 to 1000000"); call_prm.bg_max_ppm = (int32_t)iv; call_option_given = true; }
        else if (a == "-call_prior") {
            std::vector<long> pr;
            if (!parse_int_list(v, pr) || pr.size() != 2 || !(pr[0] > 0 && pr[0] < pr[1] && pr[1] <= (1L << 30))) return usage("-call_prior takes a,n with 0 < a < n <= 2^30");
            call_prm.a0 = (int32_t)pr[0]; call_prm.n0 = (int32_t)pr[1]; call_option_given = true;
        }
        else if (a == "-tag_mismatches") { if (!svr_parse_int(v.c_str(), &iv) || iv < 0 || iv > 1) return usage("-tag_mismatches must be 0 or 1"); tag_mism = (int)iv; }
        else if (a == "-tag_map") { if (v.empty()) return usage("-tag_map takes a file"); tag_map_path = v; }
        else if (a == "-barcode_mismatches") {
            if (!svr_parse_int(v.c_str(), &iv) || iv < 0 || iv > 1) return usage("-barcode_mismatches must be 0 or 1");
            bc_mism = (int)iv; bc_mism_given = true;
        }
        else return usage("unknown option: " + a);
    }
    if (inputs.empty()) return usage("no MIP table");
    if (out_path.empty()) return usage("no output: -o counts.tsv is missing");
    if (reads_a.empty() || reads_b.empty()) return usage("no reads: -reads ext.fq lig.fq is missing");
    for (const std::string* p : {&reads_a, &reads_b})
        if (p->size() >= 3 && p->compare(p->size() - 3, 3, ".gz") == 0) return usage(*p + ": compressed FASTQ is not read (plain FASTQ only: decompress it first)");
    const bool by_sample = !barcode_path.empty();
    if (by_sample && index_arg.empty()) return usage("-barcodes needs -index_reads i1.fq[,i2.fq]");
    if (!by_sample && !index_arg.empty()) return usage("-index_reads needs -barcodes samples.tsv");
    if (!by_sample && (!samples_path.empty() || !index_len_arg.empty() || bc_mism_given)) return usage("-samples, -index_length and -barcode_mismatches need -barcodes samples.tsv");
    const bool consensus = !consensus_prefix.empty();
    if (min_family_given && !consensus) return usage("-min_family needs -consensus prefix");
    if (consensus && te + tl == 0) return usage("-consensus needs tag bases: with -tag_sizes 0,0 there are no molecules to collapse");
    if (tag_mism && te + tl == 0) return usage("-tag_mismatches 1 needs tag bases: with -tag_sizes 0,0 there are no tags to correct");
    const bool tag_map = !tag_map_path.empty();
    if (tag_map && !tag_mism) return usage("-tag_map needs -tag_mismatches 1");
    // (-pileup reads the consensus reads: its session keeps the reads too; -tag_mismatches 1 merges by family size, which only such a session has)
    const bool pileup = !pileup_path.empty(), keep_reads = consensus || pileup || tag_mism;
    if (pile_option_given && !pileup) return usage("-pileup_min_family and -pileup_min_quality need -pileup file");
    if (pile_indels && !pileup) return usage("-pileup_indels needs -pileup file");
    const bool insertions = !ins_path.empty();
    if (insertions && !pile_indels) return usage("-pileup_insertions needs -pileup file -pileup_indels W");
    const bool deletions = !del_path.empty();
    if (deletions && !pile_indels) return usage("-pileup_deletions needs -pileup file -pileup_indels W");
    const bool call = !call_path.empty();
    if (call && !pileup) return usage("-call needs -pileup file");
    const bool loci = !loci_path.empty(), call_loci = !call_loci_path.empty();
    if (loci && !pileup) return usage("-pileup_loci needs -pileup file");
    if ((call_loci || loci_parts_given) && !loci) return usage("-call_loci and -loci_parts need -pileup_loci file");
    const bool call_ins = !call_ins_path.empty();
    if (call_ins && !insertions) return usage("-call_insertions needs -pileup_insertions file");
    const bool ins_loci = !ins_loci_path.empty(), call_ins_loci = !call_ins_loci_path.empty();
    if (ins_loci && (!insertions || !loci)) return usage("-insertion_loci needs -pileup_insertions file and -pileup_loci file");
    if (call_ins_loci && !ins_loci) return usage("-call_insertion_loci needs -insertion_loci file");
    if (call_option_given && !call && !call_loci && !call_ins && !call_ins_loci) return usage("the -call_* options need -call file or -call_loci file");
    if (pileup && te + tl == 0) return usage("-pileup needs tag bases: with -tag_sizes 0,0 there are no molecules to count");
    std::vector<std::string> index_paths;
    std::vector<long> index_len;
    if (by_sample) {
        const size_t c = index_arg.find(',');
        index_paths.push_back(index_arg.substr(0, c));
        if (c != std::string::npos) index_paths.push_back(index_arg.substr(c + 1));
        for (const std::string& p : index_paths) {
            if (p.empty() || p.find(',') != std::string::npos) return usage("-index_reads takes one file or two, i1.fq[,i2.fq]");
            if (p.size() >= 3 && p.compare(p.size() - 3, 3, ".gz") == 0) return usage(p + ": compressed FASTQ is not read (plain FASTQ only: decompress it first)");
        }
        if (!index_len_arg.empty()) {
            if (!parse_int_list(index_len_arg, index_len) || index_len.size() != index_paths.size()) return usage("-index_length takes one length per index file, j1[,j2]");
            for (long j : index_len) if (j < 1 || j > 32) return usage("-index_length: a length is 1 to 32");
        } else if (index_paths.size() == 2) return usage("two index files need -index_length j1,j2");
    }

    // ---- everything is read and checked before the device is opened ----
    std::vector<std::string> sample_labels, barcodes;
    if (by_sample) {
        if (!read_barcodes(barcode_path, sample_labels, barcodes)) return 1;
        const long J = (long)barcodes[0].size();
        if (index_len.empty()) index_len.push_back(J);
        long sum = 0;
        for (long j : index_len) sum += j;
        if (sum != J) { fprintf(stderr, "%s: -index_length %s: the lengths must sum to the barcode length %ld\n", PROG, index_len_arg.c_str(), J); return 1; }
    }
    std::vector<Table> tables(inputs.size());
    for (size_t k = 0; k < inputs.size(); k++) if (!read_table(PROG, inputs[k], 0, tables[k])) return 1;
    std::vector<mipgen_probe> probes;
    std::vector<const std::vector<std::string>*> rows;
    size_t shortest = MIPGEN_MAX_OLIGO;
    for (const Table& t : tables)
        for (const auto& r : t.rows) {
            mipgen_probe q;
            memset(&q, 0, sizeof q);
            q.ext_seq = r[COL_EXT_SEQ].c_str(); q.lig_seq = r[COL_LIG_SEQ].c_str(); q.ins_seq = r[COL_INS_SEQ].c_str(); q.mip_seq = r[COL_MIP_SEQ].c_str();
            q.lrc_index = -1;
            probes.push_back(q); rows.push_back(&r);
            shortest = std::min(shortest, std::min(r[COL_EXT_SEQ].size(), r[COL_LIG_SEQ].size()));
        }
    if (probes.empty()) { fprintf(stderr, "%s: the tables hold no probe\n", PROG); return 1; }
    if (probes.size() > (size_t)INT32_MAX) { fprintf(stderr, "%s: too many probes\n", PROG); return 1; }
    // -pileup: the length of every probe's molecule and where it lies on the genome
    std::vector<int32_t> mol_len;
    std::string mol_seq;                                                                 // -pileup_indels, -call: the templates, upper-cased, in probe order
    std::vector<RowCoords> coords;
    if (pileup)
        for (const auto* r : rows) {
            RowCoords c;
            const char* what = nullptr;
            if (!row_coords(*r, &c, &what)) { fprintf(stderr, "%s: -pileup: probe %s: %s\n", PROG, (*r)[COL_KEY].c_str(), what); return 1; }
            coords.push_back(c);
            mol_len.push_back((int32_t)((*r)[COL_EXT_SEQ].size() + (*r)[COL_INS_SEQ].size() + (*r)[COL_LIG_SEQ].size()));
            if (pile_indels || call || loci) {                                           // (-call, -pileup_loci: the templates supply the ref bytes)
                if (pile_indels && mol_len.back() > MIPGEN_GAPPED_MAX_MOL) {
                    fprintf(stderr, "%s: -pileup_indels: probe %s: a molecule of %d bases (at most %d are placed)\n", PROG, (*r)[COL_KEY].c_str(), mol_len.back(), MIPGEN_GAPPED_MAX_MOL);
                    return 1;
                }
                for (const std::string* part : {&(*r)[COL_EXT_SEQ], &(*r)[COL_INS_SEQ], &(*r)[COL_LIG_SEQ]})
                    for (char ch : *part) mol_seq.push_back((char)toupper((unsigned char)ch));
            }
        }
    // -pileup_loci: the plan, before the device is opened
    locus::Plan lplan;
    if (loci) {
        std::vector<locus::Row> lrows;
        for (size_t i = 0, at = 0; i < rows.size(); at += (size_t)mol_len[i], i++) {
            const auto& f = *rows[i];
            locus::Row r;
            r.chr = f[COL_CHR]; r.ext_start = coords[i].ext_start; r.ext_stop = coords[i].ext_stop; r.minus = coords[i].minus;
            r.n_ext = f[COL_EXT_SEQ].size(); r.n_lig = f[COL_LIG_SEQ].size(); r.mol = mol_seq.substr(at, (size_t)mol_len[i]);
            lrows.push_back(r);
        }
        locus::Conflict bad;
        if (!locus::build_plan(lrows, loci_all, &lplan, &bad))
            return usage("-pileup_loci: locus " + bad.chr + ":" + std::to_string(bad.position) + ": table row " + std::to_string(bad.row_a + 1) + " (" + (*rows[bad.row_a])[COL_KEY] +
                         ") gives ref " + std::string(1, bad.ref_a) + ", table row " + std::to_string(bad.row_b + 1) + " (" + (*rows[bad.row_b])[COL_KEY] + ") gives ref " +
                         std::string(1, bad.ref_b));
        if (lplan.locus_pos.empty()) return usage("-pileup_loci: no template position is included: the targets of the tables are empty (-loci_parts all keeps the arms)");
        if (lplan.plan.size() > ((size_t)1 << 29) - 1) return usage("-pileup_loci: more than 2^29 - 1 template positions");
    }
    if (shortest < 12) { fprintf(stderr, "%s: the shortest arm of the tables has %zu bases: a seed of fewer than 12 bases is refused\n", PROG, shortest); return 1; }
    Fastq fe, fl;
    fe.path = swap ? reads_b : reads_a; fl.path = swap ? reads_a : reads_b;
    Fastq fi[2];
    std::vector<Fastq*> files = {&fe, &fl};
    for (size_t k = 0; k < index_paths.size(); k++) { fi[k].path = index_paths[k]; files.push_back(&fi[k]); }
    for (Fastq* f : files) if (!f->open()) { fprintf(stderr, "%s: can't open FASTQ file %s\n", PROG, f->path.c_str()); return 1; }
    int64_t n_records = 0;
    for (;;) {
        const int a = fe.next(nullptr), b = fl.next(nullptr);
        if (a < 0 || b < 0) return 1;
        if (a != b) {
            fprintf(stderr, "%s: %s holds %s records than %s (%lld pairs read)\n", PROG, fe.path.c_str(), a ? "more" : "fewer", fl.path.c_str(), (long long)n_records);
            return 1;
        }
        for (size_t k = 0; k < index_paths.size(); k++) {
            const int c = fi[k].next(nullptr);
            if (c < 0) return 1;
            if (c != a) {
                fprintf(stderr, "%s: %s holds %s records than %s (%lld pairs read)\n", PROG, fi[k].path.c_str(), c ? "more" : "fewer", fe.path.c_str(), (long long)n_records);
                return 1;
            }
        }
        if (!a) break;
        n_records++;
    }
    for (Fastq* f : files) { fclose(f->fp); f->fp = nullptr; if (!f->open()) { fprintf(stderr, "%s: can't open FASTQ file %s\n", PROG, f->path.c_str()); return 1; } }

    FILE* cons_out[2] = {nullptr, nullptr};
    const std::string cons_path[2] = {consensus_prefix + ".ext.fq", consensus_prefix + ".lig.fq"};
    if (consensus)
        for (int k = 0; k < 2; k++)
            if (!(cons_out[k] = fopen(cons_path[k].c_str(), "w"))) return usage("-consensus " + consensus_prefix + ": can't write " + cons_path[k]);
    FILE* pile_out = nullptr;
    if (pileup && !(pile_out = fopen(pileup_path.c_str(), "w"))) return usage("-pileup " + pileup_path + ": can't write " + pileup_path);
    FILE* ins_out = nullptr;
    if (insertions && !(ins_out = fopen(ins_path.c_str(), "w"))) return usage("-pileup_insertions " + ins_path + ": can't write " + ins_path);
    FILE* del_out = nullptr;
    if (deletions && !(del_out = fopen(del_path.c_str(), "w"))) return usage("-pileup_deletions " + del_path + ": can't write " + del_path);
    FILE* call_ins_out = nullptr;
    if (call_ins && !(call_ins_out = fopen(call_ins_path.c_str(), "w"))) return usage("-call_insertions " + call_ins_path + ": can't write " + call_ins_path);
    FILE* call_out = nullptr;
    if (call && !(call_out = fopen(call_path.c_str(), "w"))) return usage("-call " + call_path + ": can't write " + call_path);
    FILE *loci_out = nullptr, *call_loci_out = nullptr;
    if (loci && !(loci_out = fopen(loci_path.c_str(), "w"))) return usage("-pileup_loci " + loci_path + ": can't write " + loci_path);
    if (call_loci && !(call_loci_out = fopen(call_loci_path.c_str(), "w"))) return usage("-call_loci " + call_loci_path + ": can't write " + call_loci_path);
    FILE *ins_loci_out = nullptr, *call_ins_loci_out = nullptr;
    if (ins_loci && !(ins_loci_out = fopen(ins_loci_path.c_str(), "w"))) return usage("-insertion_loci " + ins_loci_path + ": can't write " + ins_loci_path);
    if (call_ins_loci && !(call_ins_loci_out = fopen(call_ins_loci_path.c_str(), "w")))
        return usage("-call_insertion_loci " + call_ins_loci_path + ": can't write " + call_ins_loci_path);

    FILE* tag_map_out = nullptr;
    if (tag_map && !(tag_map_out = fopen(tag_map_path.c_str(), "w"))) return usage("-tag_map " + tag_map_path + ": can't write " + tag_map_path);

    // ---- the device ----
    mipgen_accel* h = nullptr;
    if (svr_tool_handle(&h) != MIPGEN_OK) { fprintf(stderr, "%s: %s\n", PROG, mipgen_accel_last_error()); return 1; }
    auto die = [&]() { fprintf(stderr, "%s: %s\n", PROG, mipgen_accel_last_error()); mipgen_accel_destroy(h); return 1; };
    // the three kinds of session (plain, -barcodes, -consensus with or without -barcodes) behind one open / feed / finish each
    std::vector<const char*> bc;
    for (const std::string& b : barcodes) bc.push_back(b.c_str());
    const int32_t n_probes32 = (int32_t)probes.size(), n_bc = (int32_t)bc.size();
    auto open_session = [&]() {
        return keep_reads ? mipgen_accel_reads_open_consensus(h, probes.data(), n_probes32, te, tl, mism, by_sample ? bc.data() : nullptr, n_bc, bc_mism, 0)
               : by_sample ? mipgen_accel_reads_open_samples(h, probes.data(), n_probes32, te, tl, mism, bc.data(), n_bc, bc_mism)
                           : mipgen_accel_reads_open(h, probes.data(), n_probes32, te, tl, mism);
    };
    auto feed_chunk = [&](const Chunk& c) {
        return keep_reads ? mipgen_accel_reads_feed_consensus(h, c.n, c.ext.data(), c.ext_qual.data(), c.ext_off.data(), c.lig.data(), c.lig_qual.data(), c.lig_off.data(),
                                                             by_sample ? c.idx.data() : nullptr, by_sample ? c.idx_off.data() : nullptr)
               : by_sample ? mipgen_accel_reads_feed_samples(h, c.n, c.ext.data(), c.ext_off.data(), c.lig.data(), c.lig_off.data(), c.idx.data(), c.idx_off.data())
                           : mipgen_accel_reads_feed(h, c.n, c.ext.data(), c.ext_off.data(), c.lig.data(), c.lig_off.data());
    };
    auto finish_session = [&](int64_t* reads, int64_t* unique, mipgen_read_totals* tot, mipgen_sample_totals* stot, int64_t* row_pairs, mipgen_consensus_sizes* csz) {
        return keep_reads ? mipgen_accel_reads_finish_consensus(h, reads, unique, tot, stot, row_pairs, csz)
               : by_sample ? mipgen_accel_reads_finish_samples(h, reads, unique, tot, stot, row_pairs)
                           : mipgen_accel_reads_finish(h, reads, unique, tot);
    };
    if (open_session() != MIPGEN_OK) return die();
    if (tag_mism && mipgen_accel_reads_set_tag_mismatches(h, tag_mism) != MIPGEN_OK) return die();

    // two chunks: the reader thread fills one while the device works on the other
    Chunk chunks[2];
    std::mutex mu;
    std::condition_variable cv;
    bool full[2] = {false, false}, stop = false;
    std::thread reader([&]() {
        for (int k = 0;; k ^= 1) {
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return !full[k] || stop; }); if (stop) return; }
            Chunk& c = chunks[k];
            c.ext.clear(); c.lig.clear(); c.idx.clear(); c.ext_qual.clear(); c.lig_qual.clear(); c.ext_off.assign(1, 0); c.lig_off.assign(1, 0); c.idx_off.assign(1, 0); c.n = 0; c.last = false;
            std::string part[2];
            while (c.n < CHUNK_PAIRS) {
                const int a = fe.next(&c.ext, keep_reads ? &c.ext_qual : nullptr), b = fl.next(&c.lig, keep_reads ? &c.lig_qual : nullptr);
                if (a < 0 || b < 0 || a != b) { c.failed = true; break; }          // (the files changed since they were checked)
                bool whole = true;
                for (size_t k = 0; k < index_paths.size() && !c.failed; k++) {
                    part[k].clear();
                    if (fi[k].next(&part[k]) != a) c.failed = true;
                    whole = whole && part[k].size() >= (size_t)index_len[k];
                }
                if (c.failed) break;
                if (!a) { c.last = true; break; }
                // the pair's index: the first j bases of each index read, or nothing when one of them is shorter than its j
                for (size_t k = 0; whole && k < index_paths.size(); k++) c.idx.append(part[k], 0, (size_t)index_len[k]);
                c.idx_off.push_back((int64_t)c.idx.size());
                c.ext_off.push_back((int64_t)c.ext.size()); c.lig_off.push_back((int64_t)c.lig.size());
                c.n++;
            }
            const bool done = c.last || c.failed;
            { std::lock_guard<std::mutex> lk(mu); full[k] = true; }
            cv.notify_all();
            if (done) return;
        }
    });
    int rc = 0;
    for (int k = 0;; k ^= 1) {
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return full[k]; }); }
        Chunk& c = chunks[k];
        if (c.failed) { fprintf(stderr, "%s: the FASTQ files changed while they were read\n", PROG); rc = 1; }
        else if (c.n > 0 && feed_chunk(c) != MIPGEN_OK) {
            fprintf(stderr, "%s: %s\n", PROG, mipgen_accel_last_error()); rc = 1;
        }
        const bool done = rc != 0 || c.last;
        { std::lock_guard<std::mutex> lk(mu); full[k] = false; if (done) stop = true; }
        cv.notify_all();
        if (done) break;
    }
    reader.join();
    if (rc) { mipgen_accel_destroy(h); return 1; }
    const size_t n_probes = probes.size(), n_rows = by_sample ? barcodes.size() + 1 : 1;
    std::vector<int64_t> reads(n_probes * n_rows), unique(n_probes * n_rows), row_pairs(n_rows);
    mipgen_read_totals tot;
    mipgen_sample_totals stot{0, 0};
    mipgen_consensus_sizes csz{0, 0, 0};
    if (finish_session(reads.data(), unique.data(), &tot, &stot, row_pairs.data(), &csz) != MIPGEN_OK) return die();
    // -tag_mismatches 1: what was merged, and the map of the raw groups
    mipgen_tag_merge_totals tmt{0, 0, 0, 0, 0};
    if (tag_mism && mipgen_accel_reads_last_tag_merge(h, &tmt) != MIPGEN_OK) return die();
    if (tag_map) {
        const size_t G0 = (size_t)tmt.raw_groups;
        std::vector<int32_t> m_cell(G0), m_family(G0);
        std::vector<uint32_t> m_raw(G0), m_tag(G0);
        if (mipgen_accel_reads_tag_map_fetch(h, m_cell.data(), m_raw.data(), m_family.data(), m_tag.data()) != MIPGEN_OK) return die();
        const int T = te + tl;
        const size_t n_p = probes.size(), n_r = by_sample ? barcodes.size() + 1 : 1;
        fprintf(tag_map_out, "sample\tmip_key\traw_tag\traw_family\ttag\n");
        for (size_t g = 0; g < G0; g++) {
            const size_t r = (size_t)m_cell[g] / n_p, i = (size_t)m_cell[g] % n_p;
            char raw[17], cor[17];
            for (int j = 0; j < T; j++) { raw[j] = "ACGT"[(m_raw[g] >> (2 * (T - 1 - j))) & 3u]; cor[j] = "ACGT"[(m_tag[g] >> (2 * (T - 1 - j))) & 3u]; }
            raw[T] = cor[T] = 0;
            fprintf(tag_map_out, "%s\t%s\t%s\t%d\t%s\n", !by_sample ? "*" : r + 1 < n_r ? sample_labels[r].c_str() : "undetermined", (*rows[i])[COL_KEY].c_str(), raw, m_family[g], cor);
        }
        if (fclose(tag_map_out) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, tag_map_path.c_str()); mipgen_accel_destroy(h); return 1; }
    }
    const mipgen_consensus_sizes fsz = consensus ? csz : mipgen_consensus_sizes{0, 0, 0};      // (-pileup alone downloads no consensus read)
    std::vector<int32_t> g_cell((size_t)fsz.n_groups), g_family((size_t)fsz.n_groups);
    std::vector<uint32_t> g_tag((size_t)fsz.n_groups);
    std::vector<int64_t> g_off[2] = {std::vector<int64_t>((size_t)fsz.n_groups + 1), std::vector<int64_t>((size_t)fsz.n_groups + 1)};
    std::string g_seq[2] = {std::string((size_t)fsz.ext_bytes, '\0'), std::string((size_t)fsz.lig_bytes, '\0')}, g_qual[2] = {g_seq[0], g_seq[1]};
    if (consensus && mipgen_accel_reads_consensus_fetch(h, g_cell.data(), g_tag.data(), g_family.data(), g_off[0].data(), &g_seq[0][0], &g_qual[0][0], g_off[1].data(), &g_seq[1][0],
                                                        &g_qual[1][0]) != MIPGEN_OK) return die();
    // -pileup: one call per row; a second thread turns the counts of a row into lines while the device counts the next row
    long long pile_used = 0, pile_lines = 0, pile_bases = 0, pile_nonref = 0, pile_disc = 0, pile_del = 0, pile_ins = 0, pile_insd = 0, pile_gapped = 0;
    long long call_calls = 0, call_cands = 0, call_tested = 0, call_deep = 0;
    long long loci_lines = 0, loci_bases = 0, loci_nonref = 0, loci_disc = 0, lcall_calls = 0, lcall_cands = 0, lcall_tested = 0, lcall_deep = 0;
    long long ins_alleles = 0, ins_events = 0, ins_amb = 0, ins_span = 0;
    long long del_alleles = 0, del_events = 0, del_ragged = 0, del_bases = 0;
    long long icall_calls = 0, icall_cands = 0, icall_tested = 0, icall_deep = 0;
    long long iloci_alleles = 0, iloci_events = 0, iloci_amb = 0, iloci_span = 0, ilcall_calls = 0, ilcall_cands = 0, ilcall_tested = 0, ilcall_deep = 0;
    const size_t pile_cols = pile_indels ? 8 : 5;
    if (pileup) {
        int64_t n_pos = 0;
        std::vector<int64_t> pos_off;
        for (int32_t l : mol_len) { pos_off.push_back(n_pos); n_pos += l; }
        std::vector<int32_t> table[2] = {std::vector<int32_t>((size_t)n_pos * pile_cols), std::vector<int32_t>(n_rows > 1 ? (size_t)n_pos * pile_cols : 0)};
        auto write_row = [&](size_t r, const std::vector<int32_t>& counts) {
            const char* sample = !by_sample ? "*" : r + 1 < n_rows ? sample_labels[r].c_str() : "undetermined";
            std::string text;
            char buf[160];
            for (size_t i = 0; i < n_probes; i++) {
                const std::vector<std::string>& f = *rows[i];
                const RowCoords& c = coords[i];
                const size_t n_ext = f[COL_EXT_SEQ].size(), n_ins = f[COL_INS_SEQ].size();
                for (int32_t t = 0; t < mol_len[i]; t++) {
                    const int32_t* k = &counts[(size_t)(pos_off[i] + t) * pile_cols];
                    // -pileup_indels: del at t; the insertion columns of the anchor whose LOWER genome coordinate this line is - anchor t (between t and t + 1) on
                    // the plus strand, anchor t - 1 on the minus strand
                    int32_t indel[3] = {0, 0, 0};
                    if (pile_indels) {
                        indel[0] = k[5];
                        const int32_t* a = c.minus ? (t > 0 ? k - 8 : nullptr) : k;
                        if (a) { indel[1] = a[6]; indel[2] = a[7]; }
                    }
                    if (!(k[0] | k[1] | k[2] | k[3] | k[4] | indel[0] | indel[1] | indel[2])) continue;
                    const size_t ut = (size_t)t;
                    char ref = (char)toupper((unsigned char)(ut < n_ext ? f[COL_EXT_SEQ][ut] : ut < n_ext + n_ins ? f[COL_INS_SEQ][ut - n_ext] : f[COL_LIG_SEQ][ut - n_ext - n_ins]));
                    int32_t plus[4] = {k[0], k[1], k[2], k[3]};
                    if (c.minus) {                                                       // the molecule shows the minus strand: complement everything
                        ref = ref == 'A' ? 'T' : ref == 'C' ? 'G' : ref == 'G' ? 'C' : ref == 'T' ? 'A' : ref;
                        plus[0] = k[3]; plus[1] = k[2]; plus[2] = k[1]; plus[3] = k[0];
                    }
                    for (int b = 0; b < 4; b++) { pile_bases += plus[b]; if ("ACGT"[b] != ref) pile_nonref += plus[b]; }
                    pile_disc += k[4];
                    int at = snprintf(buf, sizeof buf, "\t%ld\t%c\t%s\t%c\t%d\t%d\t%d\t%d\t%d", c.minus ? c.ext_stop - t : c.ext_start + t, c.minus ? '-' : '+',
                                      ut < n_ext ? "ext" : ut < n_ext + n_ins ? "target" : "lig", ref, plus[0], plus[1], plus[2], plus[3], k[4]);
                    if (pile_indels) {
                        at += snprintf(buf + at, sizeof buf - (size_t)at, "\t%d\t%d\t%d", indel[0], indel[1], indel[2]);
                        pile_del += indel[0]; pile_ins += indel[1]; pile_insd += indel[2];
                    }
                    snprintf(buf + at, sizeof buf - (size_t)at, "\n");
                    text.append(sample).append("\t").append(f[COL_KEY]).append("\t").append(f[COL_CHR]).append(buf);
                    pile_lines++;
                }
            }
            fwrite(text.data(), 1, text.size(), pile_out);
        };
        // -pileup_insertions: the records of a row (ascending anchor, so table order) as lines; span comes from the anchor table of the row
        std::vector<int32_t> ianch[2] = {std::vector<int32_t>(insertions ? (size_t)n_pos * 4 : 0), std::vector<int32_t>(insertions && n_rows > 1 ? (size_t)n_pos * 4 : 0)};
        std::vector<mipgen_insertion_record> irecs[2];
        // what a line of INS and a line of ICALLS share of an allele: sample, mip_key, chr, position, strand, length and the inserted bases, appended to *text
        auto append_allele = [&](const char* sample, int64_t pos, int32_t length, uint32_t bases, bool ambiguous, std::string* text) {
            const size_t i = (size_t)(std::upper_bound(pos_off.begin(), pos_off.end(), pos) - pos_off.begin()) - 1;
            const std::vector<std::string>& f = *rows[i];
            const RowCoords& c = coords[i];
            const long t = (long)(pos - pos_off[i]);
            std::string inserted((size_t)length, 'N');
            if (!ambiguous)
                for (int j = 0; j < length; j++) {                                       // base j of the molecule; on a '-' probe the plus strand reads it from the far end, complemented
                    const unsigned code = (bases >> (2 * (length - 1 - j))) & 3u;
                    if (c.minus) inserted[(size_t)(length - 1 - j)] = "TGCA"[code]; else inserted[(size_t)j] = "ACGT"[code];
                }
            char buf[120];
            snprintf(buf, sizeof buf, "\t%ld\t%c\t%d\t", c.minus ? c.ext_stop - (t + 1) : c.ext_start + t, c.minus ? '-' : '+', length);
            text->append(sample).append("\t").append(f[COL_KEY]).append("\t").append(f[COL_CHR]).append(buf).append(inserted);
        };
        auto write_insertions = [&](size_t r, const std::vector<int32_t>& anch, const std::vector<mipgen_insertion_record>& rec) {
            const char* sample = !by_sample ? "*" : r + 1 < n_rows ? sample_labels[r].c_str() : "undetermined";
            std::string text;
            char buf[120];
            for (const mipgen_insertion_record& q : rec) {
                append_allele(sample, q.pos, q.length, q.bases, q.ambiguous != 0, &text);
                const int32_t span = anch[(size_t)q.pos * 4];
                snprintf(buf, sizeof buf, "\t%d\t%d\t%lld\n", q.count, span, (long long)q.count * 1000000ll / span);
                text.append(buf);
            }
            fwrite(text.data(), 1, text.size(), ins_out);
        };
        // -call_insertions: the call records of a row (ascending allele key, so table order) as lines
        std::vector<mipgen_insertion_call_record> icrecs[2];
        auto write_insertion_calls = [&](size_t r, const std::vector<mipgen_insertion_call_record>& rec) {
            const char* sample = !by_sample ? "*" : r + 1 < n_rows ? sample_labels[r].c_str() : "undetermined";
            std::string text;
            char buf[160];
            for (const mipgen_insertion_call_record& q : rec) {
                append_allele(sample, q.pos, q.length, q.bases, false, &text);
                snprintf(buf, sizeof buf, "\t%d\t%d\t%lld\t%d\t%d\t%d\n", q.depth, q.alt, (long long)q.alt * 1000000ll / q.depth, q.bg_alt, q.bg_depth, q.q);
                text.append(buf);
            }
            fwrite(text.data(), 1, text.size(), call_ins_out);
        };
        // the insertions of a row, for INS (and FILE, when counts is not NULL): the insertions call, or under -call_insertions the insertion call, which returns the same
        auto row_insertions = [&](size_t r, int32_t* counts, mipgen_insertion_totals* it) {
            int prc;
            if (call_ins) {
                mipgen_call_totals ict{0, 0, 0, 0};
                prc = mipgen_accel_reads_consensus_insertion_call(h, (int32_t)r, &call_prm, counts, ianch[r & 1].data(), it, &ict);
                if (prc == MIPGEN_OK) { icrecs[r & 1].resize((size_t)ict.calls); prc = mipgen_accel_insertion_call_fetch(h, icrecs[r & 1].data(), ict.calls); }
                if (prc == MIPGEN_OK) { icall_calls += ict.calls; icall_cands += ict.candidates; icall_tested += ict.tested; icall_deep += ict.too_deep; }
            } else
                prc = mipgen_accel_reads_consensus_insertions(h, mol_seq.data(), mol_len.data(), n_probes32, (int32_t)r, (int32_t)pile_family, (int32_t)pile_quality,
                                                              (int32_t)pile_indels, counts, ianch[r & 1].data(), it);
            if (prc == MIPGEN_OK) { irecs[r & 1].resize((size_t)it->alleles); prc = mipgen_accel_insertions_fetch(h, irecs[r & 1].data(), it->alleles); }
            if (prc == MIPGEN_OK) { ins_alleles += it->alleles; ins_events += it->insertions; ins_amb += it->ambiguous; ins_span += it->span; }
            return prc;
        };
        // -pileup_deletions: one more call per row, the deletions call, feeds DEL only; its records (ascending position, so table order) as lines.  The deleted bytes
        // are the template's, reverse-complemented on a '-' probe (only A C G T complement)
        std::vector<mipgen_deletion_record> drecs[2];
        auto row_deletions = [&](size_t r) {
            mipgen_deletion_totals dt{0, 0, 0, 0, 0, 0, 0, 0};
            int prc = mipgen_accel_reads_consensus_deletions(h, mol_seq.data(), mol_len.data(), n_probes32, (int32_t)r, (int32_t)pile_family, (int32_t)pile_quality,
                                                             (int32_t)pile_indels, nullptr, nullptr, &dt);
            if (prc == MIPGEN_OK) { drecs[r & 1].resize((size_t)dt.alleles); prc = mipgen_accel_deletions_fetch(h, drecs[r & 1].data(), dt.alleles); }
            if (prc == MIPGEN_OK) { del_alleles += dt.alleles; del_events += dt.events; del_ragged += dt.ragged; del_bases += dt.deleted_bases; }
            return prc;
        };
        auto write_deletions = [&](size_t r, const std::vector<mipgen_deletion_record>& rec) {
            const char* sample = !by_sample ? "*" : r + 1 < n_rows ? sample_labels[r].c_str() : "undetermined";
            std::string text;
            char buf[160];
            for (const mipgen_deletion_record& q : rec) {
                const size_t i = (size_t)(std::upper_bound(pos_off.begin(), pos_off.end(), q.pos) - pos_off.begin()) - 1;
                const std::vector<std::string>& f = *rows[i];
                const RowCoords& c = coords[i];
                const long a = (long)(q.pos - pos_off[i]);
                std::string deleted = mol_seq.substr((size_t)q.pos, (size_t)q.length);
                if (c.minus) {
                    std::reverse(deleted.begin(), deleted.end());
                    for (char& ch : deleted) ch = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch;
                }
                snprintf(buf, sizeof buf, "\t%ld\t%c\t%d\t", c.minus ? c.ext_stop - (a + q.length - 1) : c.ext_start + a, c.minus ? '-' : '+', q.length);
                text.append(sample).append("\t").append(f[COL_KEY]).append("\t").append(f[COL_CHR]).append(buf).append(deleted);
                snprintf(buf, sizeof buf, "\t%d\t%d\t%d\t%lld\n", q.ragged, q.count, q.depth, (long long)q.count * 1000000ll / q.depth);
                text.append(buf);
            }
            fwrite(text.data(), 1, text.size(), del_out);
        };
        // -call: the records of a row (ascending position, then allele class) as lines; within a position the printed alts go A C G T -, which on a '-' probe is
        // the reverse of the class order of the four bases
        std::vector<mipgen_call_record> recs[2];
        auto write_calls = [&](size_t r, const std::vector<mipgen_call_record>& rec) {
            const char* sample = !by_sample ? "*" : r + 1 < n_rows ? sample_labels[r].c_str() : "undetermined";
            std::string text;
            char buf[200];
            for (size_t a = 0; a < rec.size();) {
                size_t b = a;
                while (b < rec.size() && rec[b].pos == rec[a].pos) b++;
                const size_t i = (size_t)(std::upper_bound(pos_off.begin(), pos_off.end(), rec[a].pos) - pos_off.begin()) - 1;
                const std::vector<std::string>& f = *rows[i];
                const RowCoords& c = coords[i];
                const size_t n_ext = f[COL_EXT_SEQ].size(), n_ins = f[COL_INS_SEQ].size(), ut = (size_t)(rec[a].pos - pos_off[i]);
                char ref = (char)toupper((unsigned char)(ut < n_ext ? f[COL_EXT_SEQ][ut] : ut < n_ext + n_ins ? f[COL_INS_SEQ][ut - n_ext] : f[COL_LIG_SEQ][ut - n_ext - n_ins]));
                if (c.minus) ref = ref == 'A' ? 'T' : ref == 'C' ? 'G' : ref == 'G' ? 'C' : ref == 'T' ? 'A' : ref;
                for (int printed = 0; printed < 5; printed++) {                          // A C G T - as printed
                    const int cls = printed < 4 && c.minus ? 3 - printed : printed;
                    for (size_t k = a; k < b; k++) {
                        if (rec[k].allele != cls) continue;
                        const mipgen_call_record& q = rec[k];
                        snprintf(buf, sizeof buf, "\t%ld\t%c\t%s\t%c\t%c\t%d\t%d\t%lld\t%d\t%d\t%d\n", c.minus ? c.ext_stop - (long)ut : c.ext_start + (long)ut, c.minus ? '-' : '+',
                                 ut < n_ext ? "ext" : ut < n_ext + n_ins ? "target" : "lig", ref, "ACGT-"[printed], q.depth, q.alt, (long long)q.alt * 1000000ll / q.depth, q.bg_alt,
                                 q.bg_depth, q.q);
                        text.append(sample).append("\t").append(f[COL_KEY]).append("\t").append(f[COL_CHR]).append(buf);
                    }
                }
                a = b;
            }
            fwrite(text.data(), 1, text.size(), call_out);
        };
        // -pileup_loci: the merged table of a row as lines (it is in plus orientation already, the insertion columns on their lower coordinate); -call_loci: the
        // records of a row, ascending (locus, allele class), which is the printed order A C G T -
        const size_t n_loci = lplan.locus_pos.size();
        std::vector<int32_t> ltable[2] = {std::vector<int32_t>(n_loci * pile_cols), std::vector<int32_t>(n_rows > 1 ? n_loci * pile_cols : 0)};
        std::vector<mipgen_call_record> lrecs[2];
        auto write_loci = [&](size_t r, const std::vector<int32_t>& merged, const std::vector<mipgen_call_record>& rec) {
            const char* sample = !by_sample ? "*" : r + 1 < n_rows ? sample_labels[r].c_str() : "undetermined";
            std::string text;
            char buf[200];
            for (size_t l = 0; l < n_loci; l++) {
                const int32_t* k = &merged[l * pile_cols];
                int32_t any = 0;
                for (size_t c = 0; c < pile_cols; c++) any |= k[c];
                if (!any) continue;
                const char ref = lplan.locus_ref[l];
                for (int b = 0; b < 4; b++) { loci_bases += k[b]; if ("ACGT"[b] != ref) loci_nonref += k[b]; }
                loci_disc += k[4];
                int at = snprintf(buf, sizeof buf, "\t%ld\t%c\t%d\t%d\t%d\t%d\t%d\t%d", lplan.locus_pos[l], ref, lplan.sources[l], k[0], k[1], k[2], k[3], k[4]);
                if (pile_indels) at += snprintf(buf + at, sizeof buf - (size_t)at, "\t%d\t%d\t%d", k[5], k[6], k[7]);
                snprintf(buf + at, sizeof buf - (size_t)at, "\n");
                text.append(sample).append("\t").append(lplan.chroms[(size_t)lplan.locus_chr[l]]).append(buf);
                loci_lines++;
            }
            fwrite(text.data(), 1, text.size(), loci_out);
            if (!call_loci) return;
            text.clear();
            for (const mipgen_call_record& q : rec) {
                const size_t l = (size_t)q.pos;
                snprintf(buf, sizeof buf, "\t%ld\t%c\t%c\t%d\t%d\t%lld\t%d\t%d\t%d\t%d\n", lplan.locus_pos[l], lplan.locus_ref[l], "ACGT-"[q.allele], q.depth, q.alt,
                         (long long)q.alt * 1000000ll / q.depth, q.bg_alt, q.bg_depth, q.q, lplan.sources[l]);
                text.append(sample).append("\t").append(lplan.chroms[(size_t)lplan.locus_chr[l]]).append(buf);
            }
            fwrite(text.data(), 1, text.size(), call_loci_out);
        };
        // -insertion_loci: the locus records of a row (ascending locus, then allele key) as lines - the fold has turned the bases into plus orientation already -;
        // span comes from the locus anchor table of the row; -call_insertion_loci: the call records of a row likewise
        std::vector<int32_t> lanch[2] = {std::vector<int32_t>(ins_loci ? n_loci * 4 : 0), std::vector<int32_t>(ins_loci && n_rows > 1 ? n_loci * 4 : 0)};
        std::vector<mipgen_insertion_record> lirecs[2];
        std::vector<mipgen_insertion_call_record> licrecs[2];
        auto append_locus_allele = [&](const char* sample, int64_t l, int32_t length, uint32_t bases, bool ambiguous, std::string* text) {
            std::string inserted((size_t)length, 'N');
            for (int j = 0; !ambiguous && j < length; j++) inserted[(size_t)j] = "ACGT"[(bases >> (2 * (length - 1 - j))) & 3u];
            char buf[80];
            snprintf(buf, sizeof buf, "\t%ld\t%d\t", lplan.locus_pos[(size_t)l], length);
            text->append(sample).append("\t").append(lplan.chroms[(size_t)lplan.locus_chr[(size_t)l]]).append(buf).append(inserted);
        };
        auto write_insertion_loci = [&](size_t r, const std::vector<int32_t>& anch, const std::vector<mipgen_insertion_record>& rec, const std::vector<mipgen_insertion_call_record>& crec) {
            const char* sample = !by_sample ? "*" : r + 1 < n_rows ? sample_labels[r].c_str() : "undetermined";
            std::string text;
            char buf[160];
            for (const mipgen_insertion_record& q : rec) {
                append_locus_allele(sample, q.pos, q.length, q.bases, q.ambiguous != 0, &text);
                const int32_t span = anch[(size_t)q.pos * 4];
                snprintf(buf, sizeof buf, "\t%d\t%d\t%lld\t%d\n", q.count, span, (long long)q.count * 1000000ll / span, lplan.sources[(size_t)q.pos]);
                text.append(buf);
            }
            fwrite(text.data(), 1, text.size(), ins_loci_out);
            if (!call_ins_loci) return;
            text.clear();
            for (const mipgen_insertion_call_record& q : crec) {
                append_locus_allele(sample, q.pos, q.length, q.bases, false, &text);
                snprintf(buf, sizeof buf, "\t%d\t%d\t%lld\t%d\t%d\t%d\t%d\n", q.depth, q.alt, (long long)q.alt * 1000000ll / q.depth, q.bg_alt, q.bg_depth, q.q,
                         lplan.sources[(size_t)q.pos]);
                text.append(buf);
            }
            fwrite(text.data(), 1, text.size(), call_ins_loci_out);
        };
        // the ONE more call of a row under -insertion_loci: the locus insertions call, or under -call_insertion_loci the locus insertion call, which folds the same
        auto row_insertion_loci = [&](size_t r) {
            mipgen_locus_insertion_totals lit{0, 0, 0, 0, 0, 0, 0, 0};
            mipgen_call_totals ict{0, 0, 0, 0};
            int prc = call_ins_loci ? mipgen_accel_reads_consensus_locus_insertion_call(h, (int32_t)r, &call_prm, nullptr, nullptr, lanch[r & 1].data(), nullptr, &lit, &ict)
                                    : mipgen_accel_reads_consensus_locus_insertions(h, mol_seq.data(), mol_len.data(), n_probes32, (int32_t)r, (int32_t)pile_family,
                                                                                    (int32_t)pile_quality, (int32_t)pile_indels, nullptr, nullptr, lanch[r & 1].data(), nullptr, &lit);
            if (prc == MIPGEN_OK) { lirecs[r & 1].resize((size_t)lit.alleles); prc = mipgen_accel_locus_insertions_fetch(h, lirecs[r & 1].data(), lit.alleles); }
            if (prc == MIPGEN_OK && call_ins_loci) { licrecs[r & 1].resize((size_t)ict.calls); prc = mipgen_accel_locus_insertion_call_fetch(h, licrecs[r & 1].data(), ict.calls); }
            if (prc == MIPGEN_OK) {
                iloci_alleles += lit.alleles; iloci_events += lit.insertions; iloci_amb += lit.ambiguous; iloci_span += lit.span;
                ilcall_calls += ict.calls; ilcall_cands += ict.candidates; ilcall_tested += ict.tested; ilcall_deep += ict.too_deep;
            }
            return prc;
        };
        if (loci) {
            fputs(pile_indels ? ">sample\tchr\tposition\tref\tprobes\tA\tC\tG\tT\tdiscordant\tdel\tins\tins_discordant\n" : ">sample\tchr\tposition\tref\tprobes\tA\tC\tG\tT\tdiscordant\n",
                  loci_out);
            if (mipgen_accel_reads_consensus_locus_plan(h, lplan.plan.data(), (int64_t)lplan.plan.size(), (const uint8_t*)lplan.locus_ref.data(), (int64_t)n_loci) != MIPGEN_OK)
                return die();
        }
        if (call_loci) {
            fputs(">sample\tchr\tposition\tref\talt\tdepth\talt_count\talt_ppm\tbg_alt\tbg_depth\tq\tprobes\n", call_loci_out);
            if (mipgen_accel_reads_consensus_locus_call_pool(h, mol_seq.data(), mol_len.data(), n_probes32, (int32_t)pile_family, (int32_t)pile_quality, (int32_t)pile_indels,
                                                             call_prm.bg_max_ppm) != MIPGEN_OK) return die();
        }
        if (call) {
            fputs(">sample\tmip_key\tchr\tposition\tstrand\tpart\tref\talt\tdepth\talt_count\talt_ppm\tbg_alt\tbg_depth\tq\n", call_out);
            if (mipgen_accel_reads_consensus_call_pool(h, mol_seq.data(), mol_len.data(), n_probes32, (int32_t)pile_family, (int32_t)pile_quality, (int32_t)pile_indels,
                                                       call_prm.bg_max_ppm) != MIPGEN_OK) return die();
        }
        if (insertions) fputs(">sample\tmip_key\tchr\tposition\tstrand\tlength\tinserted\tcount\tspan\tppm\n", ins_out);
        if (deletions) fputs(">sample\tmip_key\tchr\tposition\tstrand\tlength\tdeleted\tragged\tcount\tdepth\tppm\n", del_out);
        if (call_ins) {
            fputs(">sample\tmip_key\tchr\tposition\tstrand\tlength\tinserted\tdepth\talt_count\talt_ppm\tbg_alt\tbg_depth\tq\n", call_ins_out);
            if (mipgen_accel_reads_consensus_insertion_pool(h, mol_seq.data(), mol_len.data(), n_probes32, (int32_t)pile_family, (int32_t)pile_quality, (int32_t)pile_indels,
                                                            call_prm.bg_max_ppm, nullptr) != MIPGEN_OK) return die();
        }
        if (ins_loci) fputs(">sample\tchr\tposition\tlength\tinserted\tcount\tspan\tppm\tprobes\n", ins_loci_out);
        if (call_ins_loci) {
            fputs(">sample\tchr\tposition\tlength\tinserted\tdepth\talt_count\talt_ppm\tbg_alt\tbg_depth\tq\tprobes\n", call_ins_loci_out);
            if (mipgen_accel_reads_consensus_locus_insertion_pool(h, mol_seq.data(), mol_len.data(), n_probes32, (int32_t)pile_family, (int32_t)pile_quality, (int32_t)pile_indels,
                                                                  call_prm.bg_max_ppm, nullptr) != MIPGEN_OK) return die();
        }
        fputs(pile_indels ? ">sample\tmip_key\tchr\tposition\tstrand\tpart\tref\tA\tC\tG\tT\tdiscordant\tdel\tins\tins_discordant\n"
                          : ">sample\tmip_key\tchr\tposition\tstrand\tpart\tref\tA\tC\tG\tT\tdiscordant\n", pile_out);
        std::thread writer;
        for (size_t r = 0; r < n_rows; r++) {
            mipgen_pileup_totals pt{0, 0, 0, 0};
            mipgen_gapped_totals gt{0, 0, 0, 0, 0, 0, 0, 0};
            mipgen_call_totals ct{0, 0, 0, 0};
            int prc;
            if (call) {                                                                  // one call per row feeds both files: its counts are the pileup's
                prc = mipgen_accel_reads_consensus_call(h, (int32_t)r, &call_prm, table[r & 1].data(), &ct);
                if (prc == MIPGEN_OK) prc = mipgen_accel_reads_consensus_call_pileup_totals(h, &gt);
                if (!loci && writer.joinable()) writer.join();                           // (not needed for the buffers - the running writer, of row r - 1, owns index
                                                                                         // (r - 1) & 1 of each - and kept where no locus option is given; with one, the join
                                                                                         // below lets the locus count of the row run beside the writing too)
                if (prc == MIPGEN_OK) { recs[r & 1].resize((size_t)ct.calls); prc = mipgen_accel_call_fetch(h, recs[r & 1].data(), ct.calls); }
                pt.used = gt.used;
                call_calls += ct.calls; call_cands += ct.candidates; call_tested += ct.tested; call_deep += ct.too_deep;
                if (loci && prc == MIPGEN_OK) {                                          // beside -call: the locus call of the row feeds LOCI (and CALLS of -call_loci) only
                    mipgen_call_totals lct{0, 0, 0, 0};
                    prc = call_loci ? mipgen_accel_reads_consensus_locus_call(h, (int32_t)r, &call_prm, nullptr, ltable[r & 1].data(), &lct)
                                    : mipgen_accel_reads_consensus_locus_pileup(h, pile_indels ? mol_seq.data() : nullptr, mol_len.data(), n_probes32, (int32_t)r, (int32_t)pile_family,
                                                                                (int32_t)pile_quality, (int32_t)pile_indels, nullptr, ltable[r & 1].data(), nullptr, nullptr);
                    if (prc == MIPGEN_OK && call_loci) { lrecs[r & 1].resize((size_t)lct.calls); prc = mipgen_accel_call_fetch(h, lrecs[r & 1].data(), lct.calls); }
                    lcall_calls += lct.calls; lcall_cands += lct.candidates; lcall_tested += lct.tested; lcall_deep += lct.too_deep;
                }
            } else if (loci) {                                                           // one locus call per row feeds FILE and LOCI (and CALLS of -call_loci)
                mipgen_locus_totals lt;
                mipgen_call_totals lct{0, 0, 0, 0};
                prc = call_loci ? mipgen_accel_reads_consensus_locus_call(h, (int32_t)r, &call_prm, table[r & 1].data(), ltable[r & 1].data(), &lct)
                                : mipgen_accel_reads_consensus_locus_pileup(h, pile_indels ? mol_seq.data() : nullptr, mol_len.data(), n_probes32, (int32_t)r, (int32_t)pile_family,
                                                                            (int32_t)pile_quality, (int32_t)pile_indels, table[r & 1].data(), ltable[r & 1].data(), &gt, &lt);
                if (prc == MIPGEN_OK && call_loci) prc = mipgen_accel_reads_consensus_locus_call_pileup_totals(h, &gt);
                if (prc == MIPGEN_OK && call_loci) { lrecs[r & 1].resize((size_t)lct.calls); prc = mipgen_accel_call_fetch(h, lrecs[r & 1].data(), lct.calls); }
                pt.used = gt.used;
                lcall_calls += lct.calls; lcall_cands += lct.candidates; lcall_tested += lct.tested; lcall_deep += lct.too_deep;
            } else if (insertions) {                                                     // one insertions call per row feeds FILE and INS: its counts are the gapped pileup's
                mipgen_insertion_totals it;
                prc = row_insertions(r, table[r & 1].data(), &it);
                if (prc == MIPGEN_OK) { gt.used = it.used; gt.gapped_sides = it.gapped_sides; }
            } else
            prc = pile_indels ? mipgen_accel_reads_consensus_pileup_gapped(h, mol_seq.data(), mol_len.data(), n_probes32, (int32_t)r, (int32_t)pile_family,
                                                                                     (int32_t)pile_quality, (int32_t)pile_indels, table[r & 1].data(), &gt)
                                        : mipgen_accel_reads_consensus_pileup(h, mol_len.data(), n_probes32, (int32_t)r, (int32_t)pile_family, (int32_t)pile_quality,
                                                                              table[r & 1].data(), &pt);
            if (insertions && (call || loci) && prc == MIPGEN_OK) {                      // beside -call or -pileup_loci: the insertions call of the row feeds INS only
                mipgen_insertion_totals it;
                prc = row_insertions(r, nullptr, &it);
            }
            if (ins_loci && prc == MIPGEN_OK) prc = row_insertion_loci(r);              // one more call per row: it feeds ILOCI (and ILCALLS) only
            if (deletions && prc == MIPGEN_OK) prc = row_deletions(r);                  // one more call per row: it feeds DEL only
            if (pile_indels) { pt.used = gt.used; pile_gapped += gt.gapped_sides; }
            if (writer.joinable()) writer.join();
            if (prc != MIPGEN_OK) return die();
            pile_used += pt.used;
            writer = std::thread([&, r]() {
                write_row(r, table[r & 1]);
                if (call) write_calls(r, recs[r & 1]);
                if (loci) write_loci(r, ltable[r & 1], lrecs[r & 1]);
                if (insertions) write_insertions(r, ianch[r & 1], irecs[r & 1]);
                if (call_ins) write_insertion_calls(r, icrecs[r & 1]);
                if (deletions) write_deletions(r, drecs[r & 1]);
                if (ins_loci) write_insertion_loci(r, lanch[r & 1], lirecs[r & 1], licrecs[r & 1]);
            });
        }
        if (writer.joinable()) writer.join();
        if (fclose(pile_out) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, pileup_path.c_str()); mipgen_accel_destroy(h); return 1; }
        if (insertions && fclose(ins_out) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, ins_path.c_str()); mipgen_accel_destroy(h); return 1; }
        if (deletions && fclose(del_out) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, del_path.c_str()); mipgen_accel_destroy(h); return 1; }
        if (call_ins && fclose(call_ins_out) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, call_ins_path.c_str()); mipgen_accel_destroy(h); return 1; }
        if (call && fclose(call_out) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, call_path.c_str()); mipgen_accel_destroy(h); return 1; }
        if (loci && fclose(loci_out) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, loci_path.c_str()); mipgen_accel_destroy(h); return 1; }
        if (call_loci && fclose(call_loci_out) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, call_loci_path.c_str()); mipgen_accel_destroy(h); return 1; }
        if (ins_loci && fclose(ins_loci_out) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, ins_loci_path.c_str()); mipgen_accel_destroy(h); return 1; }
        if (call_ins_loci && fclose(call_ins_loci_out) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, call_ins_loci_path.c_str()); mipgen_accel_destroy(h); return 1; }
    }
    mipgen_accel_destroy(h);

    FILE* out = fopen(out_path.c_str(), "w");
    if (!out) { fprintf(stderr, "%s: can't write %s\n", PROG, out_path.c_str()); return 1; }
    if (by_sample) {
        fprintf(out, "sample\tmip_key\tmip_name\treads\tunique_tags\n");
        for (size_t r = 0; r < n_rows; r++)
            for (size_t i = 0; i < n_probes; i++)
                if (reads[r * n_probes + i] > 0)
                    fprintf(out, "%s\t%s\t%s\t%lld\t%lld\n", r + 1 < n_rows ? sample_labels[r].c_str() : "undetermined", (*rows[i])[COL_KEY].c_str(), (*rows[i])[COL_NAME].c_str(),
                            (long long)reads[r * n_probes + i], (long long)unique[r * n_probes + i]);
    } else {
        fprintf(out, "mip_key\tmip_name\treads\tunique_tags\n");
        for (size_t i = 0; i < rows.size(); i++)
            fprintf(out, "%s\t%s\t%lld\t%lld\n", (*rows[i])[COL_KEY].c_str(), (*rows[i])[COL_NAME].c_str(), (long long)reads[i], (long long)unique[i]);
    }
    if (fclose(out) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, out_path.c_str()); return 1; }
    if (!samples_path.empty()) {
        FILE* sf = fopen(samples_path.c_str(), "w");
        if (!sf) { fprintf(stderr, "%s: can't write %s\n", PROG, samples_path.c_str()); return 1; }
        fprintf(sf, "sample\tbarcode\tpairs\tassigned\tunique_tags\tprobes_seen\n");
        for (size_t r = 0; r < n_rows; r++) {
            long long assigned = 0, tags = 0, seen = 0;
            for (size_t i = 0; i < n_probes; i++) { assigned += reads[r * n_probes + i]; tags += unique[r * n_probes + i]; seen += reads[r * n_probes + i] > 0; }
            fprintf(sf, "%s\t%s\t%lld\t%lld\t%lld\t%lld\n", r + 1 < n_rows ? sample_labels[r].c_str() : "undetermined", r + 1 < n_rows ? barcodes[r].c_str() : "*",
                    (long long)row_pairs[r], assigned, tags, seen);
        }
        if (fclose(sf) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, samples_path.c_str()); return 1; }
    }
    long long cons_written = 0, cons_members = 0;
    if (consensus) {
        const int T = te + tl;
        for (int64_t g = 0; g < csz.n_groups; g++) {
            cons_members += g_family[(size_t)g];
            if (g_family[(size_t)g] < min_family) continue;
            const size_t r = (size_t)g_cell[(size_t)g] / n_probes, i = (size_t)g_cell[(size_t)g] % n_probes;
            char tag[33];
            for (int j = 0; j < T; j++) tag[j] = "ACGT"[(g_tag[(size_t)g] >> (2 * (T - 1 - j))) & 3u];
            tag[T] = 0;
            for (int k = 0; k < 2; k++) {
                const int64_t a = g_off[k][(size_t)g], len = g_off[k][(size_t)g + 1] - a;
                fprintf(cons_out[k], "@smc%lld %s\t%s\t%s\t%d\n", (long long)g, !by_sample ? "*" : r + 1 < n_rows ? sample_labels[r].c_str() : "undetermined",
                        (*rows[i])[COL_KEY].c_str(), tag, g_family[(size_t)g]);
                fwrite(g_seq[k].data() + a, 1, (size_t)len, cons_out[k]);
                fputs("\n+\n", cons_out[k]);
                fwrite(g_qual[k].data() + a, 1, (size_t)len, cons_out[k]);
                fputc('\n', cons_out[k]);
            }
            cons_written++;
        }
        for (int k = 0; k < 2; k++)
            if (fclose(cons_out[k]) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, cons_path[k].c_str()); return 1; }
    }
    if (by_sample) {
        // the labels are over the NAMED samples: rows summed into row 0 (molecules of different samples are different molecules)
        for (size_t i = 0; i < n_probes; i++) {
            int64_t r_sum = 0, u_sum = 0;
            for (size_t r = 0; r + 1 < n_rows; r++) { r_sum += reads[r * n_probes + i]; u_sum += unique[r * n_probes + i]; }
            reads[i] = r_sum; unique[i] = u_sum;
        }
    }
    if (!label_path.empty()) {
        FILE* lab = fopen(label_path.c_str(), "w");
        if (!lab) { fprintf(stderr, "%s: can't write %s\n", PROG, label_path.c_str()); return 1; }
        for (size_t i = 0; i < rows.size(); i++) {
            fprintf(lab, "%s\t", (*rows[i])[COL_KEY].c_str());
            if (label_kind == "log10tags") fprintf(lab, "%.17g\n", log10((double)unique[i] + 1.0));
            else fprintf(lab, "%lld\n", (long long)(label_kind == "reads" ? reads[i] : unique[i]));
        }
        if (fclose(lab) != 0) { fprintf(stderr, "%s: error writing %s\n", PROG, label_path.c_str()); return 1; }
    }
    fprintf(stderr, "%s: pairs %lld assigned %lld ambiguous %lld unassigned %lld tag_n %lld overflow %lld\n", PROG, (long long)tot.pairs, (long long)tot.assigned,
            (long long)tot.ambiguous, (long long)tot.unassigned, (long long)tot.tag_n, (long long)tot.overflow);
    if (by_sample)
        fprintf(stderr, "%s: samples %zu sample_none %lld sample_ambiguous %lld\n", PROG, barcodes.size(), (long long)stot.sample_none, (long long)stot.sample_ambiguous);
    if (consensus) fprintf(stderr, "%s: consensus groups %lld written %lld members %lld\n", PROG, (long long)csz.n_groups, cons_written, cons_members);
    if (pileup) fprintf(stderr, "%s: pileup molecules %lld positions %lld bases %lld nonref %lld discordant %lld\n", PROG, pile_used, pile_lines, pile_bases, pile_nonref, pile_disc);
    if (pile_indels) fprintf(stderr, "%s: pileup indels deletions %lld insertions %lld ins_discordant %lld gapped_sides %lld\n", PROG, pile_del, pile_ins, pile_insd, pile_gapped);
    if (call) fprintf(stderr, "%s: calls %lld candidates %lld tested %lld too_deep %lld\n", PROG, call_calls, call_cands, call_tested, call_deep);
    if (loci) fprintf(stderr, "%s: loci %zu lines %lld bases %lld nonref %lld discordant %lld\n", PROG, lplan.locus_pos.size(), loci_lines, loci_bases, loci_nonref, loci_disc);
    if (call_loci) fprintf(stderr, "%s: locus calls %lld candidates %lld tested %lld too_deep %lld\n", PROG, lcall_calls, lcall_cands, lcall_tested, lcall_deep);
    if (insertions) fprintf(stderr, "%s: insertion alleles %lld events %lld ambiguous %lld span %lld\n", PROG, ins_alleles, ins_events, ins_amb, ins_span);
    if (call_ins) fprintf(stderr, "%s: insertion calls %lld candidates %lld tested %lld too_deep %lld\n", PROG, icall_calls, icall_cands, icall_tested, icall_deep);
    if (ins_loci) fprintf(stderr, "%s: insertion loci %zu alleles %lld events %lld ambiguous %lld span %lld\n", PROG, lplan.locus_pos.size(), iloci_alleles, iloci_events, iloci_amb, iloci_span);
    if (call_ins_loci) fprintf(stderr, "%s: insertion locus calls %lld candidates %lld tested %lld too_deep %lld\n", PROG, ilcall_calls, ilcall_cands, ilcall_tested, ilcall_deep);
    if (tag_mism)
        fprintf(stderr, "%s: tag_mismatches 1 raw %lld groups %lld absorbed %lld moved_pairs %lld max_depth %lld\n", PROG, (long long)tmt.raw_groups, (long long)tmt.groups,
                (long long)tmt.absorbed, (long long)tmt.moved_pairs, (long long)tmt.max_depth);
    if (deletions) fprintf(stderr, "%s: deletion alleles %lld events %lld ragged %lld deleted_bases %lld\n", PROG, del_alleles, del_events, del_ragged, del_bases);
    return 0;
}
