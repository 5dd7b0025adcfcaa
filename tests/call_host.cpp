// call_host.cpp — the host functions of mipgen_amd/csrc/call_model.h run as a plain C++ program (test infrastructure for tests/test_call_cpu.py, built with
// -fsanitize=address,undefined): one cell per input line, every array in a heap block of its exact size.
//   call_host CASES        CASES: one cell per line, "columns c0 .. c[columns-1] K N a own min_depth min_alt min_ppm min_q a0 n0 bg_max_ppm": the row of the count table,
//                          the pool's sums for allele class a, whether the row is a sample row, and the seven parameters
//   stdout                 per cell "candidate K_o N_o q phred": 0 / 1, the leave-one-out sums, and for a candidate its score (q -1 and phred 0 otherwise; phred with
//                          17 significant digits, before the floor and the cap)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "../mipgen_amd/csrc/call_model.h"

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: call_host CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "call_host: can't read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        int columns = 0;
        if (!(ls >> columns) || (columns != 5 && columns != 8)) { fprintf(stderr, "call_host: bad case: %s\n", line.c_str()); return 2; }
        int32_t* row = (int32_t*)malloc((size_t)columns * sizeof(int32_t));
        CallModel* P = (CallModel*)malloc(sizeof(CallModel));
        long long K = 0, N = 0;
        int a = 0, own = 0;
        bool ok = true;
        for (int c = 0; c < columns; c++) ok = ok && (ls >> row[c]);
        ok = ok && (ls >> K >> N >> a >> own >> P->min_depth >> P->min_alt >> P->min_ppm >> P->min_q >> P->a0 >> P->n0 >> P->bg_max_ppm) && a >= 0 && a < call_alleles(columns);
        if (!ok) { fprintf(stderr, "call_host: bad case: %s\n", line.c_str()); return 2; }
        const int64_t n = call_depth(row, columns), k = call_allele_count(row, columns, a);
        int64_t K_o = 0, N_o = 0;
        call_leave_one_out(K, N, k, n, own != 0, P->bg_max_ppm, &K_o, &N_o);
        const bool cand = call_candidate(k, n, K_o, N_o, *P);
        double phred = 0.0;
        const int q = cand ? call_tail_q(k, n, K_o + P->a0, N_o + P->n0, &phred) : -1;
        printf("%d %lld %lld %d %.17g\n", cand ? 1 : 0, (long long)K_o, (long long)N_o, q, phred);
        free(P); free(row);
    }
    return 0;
}
