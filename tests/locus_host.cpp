// locus_host.cpp — the plan builder of mipgen_amd/host/locus_plan.hpp run on tables from a file, for tests/test_locus_cpu.py (built with the address and
// undefined-behaviour sanitizers).  Input: per case a line "case <rows> <all_parts>", then per row "chr ext_start ext_stop strand n_ext n_lig M".  Output per
// case: "conflict chr position row_a ref_a row_b ref_b", or "ok <n_loci>" followed by the lines "plan ...", "loci chr:position ...", "ref <bytes>" and
// "sources ...".
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../mipgen_amd/host/locus_plan.hpp"

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: locus_host cases.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in.is_open()) { fprintf(stderr, "locus_host: can't open %s\n", argv[1]); return 2; }
    std::string word;
    while (in >> word) {
        size_t n_rows = 0;
        int all_parts = 0;
        if (word != "case" || !(in >> n_rows >> all_parts)) { fprintf(stderr, "locus_host: malformed case line\n"); return 2; }
        std::vector<locus::Row> rows(n_rows);
        for (locus::Row& r : rows) {
            std::string strand;
            if (!(in >> r.chr >> r.ext_start >> r.ext_stop >> strand >> r.n_ext >> r.n_lig >> r.mol)) { fprintf(stderr, "locus_host: malformed row\n"); return 2; }
            r.minus = strand == "-";
        }
        locus::Plan P;
        locus::Conflict bad;
        if (!locus::build_plan(rows, all_parts != 0, &P, &bad)) {
            printf("conflict %s %ld %zu %c %zu %c\n", bad.chr.c_str(), bad.position, bad.row_a, bad.ref_a, bad.row_b, bad.ref_b);
            continue;
        }
        printf("ok %zu\nplan", P.locus_pos.size());
        for (int64_t e : P.plan) printf(" %lld", (long long)e);
        printf("\nloci");
        for (size_t l = 0; l < P.locus_pos.size(); l++) printf(" %s:%ld", P.chroms[(size_t)P.locus_chr[l]].c_str(), P.locus_pos[l]);
        printf("\nref %s\nsources", P.locus_ref.c_str());
        for (int32_t s : P.sources) printf(" %d", s);
        printf("\n");
    }
    return 0;
}
