// insertion_call_host.cpp — insertion_call_model.h (and through it call_model.h and gapped_align.h) as a plain C++ program, for the sanitizers: TEST
// INFRASTRUCTURE ONLY.  tests/test_insertion_call_cpu.py builds it with -fsanitize=address,undefined, runs it on a file of cases and compares what it prints with
// the oracle.  Every array sits in a heap block of its exact size, so a search that reads one element beyond either end is an error the sanitizer reports.
//
// The case file is a sequence of blocks:
//   pool P                      then P lines "key K X" (keys in hex, strictly ascending)
//   cell key k n S own min_depth min_alt min_ppm min_q a0 n0 bg_max_ppm     -> "K_o N_o candidate q" (q = -1 unless a candidate) against the pool read last
//   find key                    -> the index of the key in the pool read last, or -1
//   add k n bg_max_ppm          -> "K X": what a sample row's record adds to its entry
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../mipgen_amd/csrc/insertion_call_model.h"

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: insertion_call_host cases.txt\n"); return 2; }
    FILE* fp = fopen(argv[1], "r");
    if (!fp) { fprintf(stderr, "can't open %s\n", argv[1]); return 2; }
    uint64_t* keys = (uint64_t*)malloc(0);
    InsPoolSums* sums = (InsPoolSums*)malloc(0);
    long long n_pool = 0;
    char word[16];
    while (fscanf(fp, "%15s", word) == 1) {
        if (!strcmp(word, "pool")) {
            if (fscanf(fp, "%lld", &n_pool) != 1 || n_pool < 0) return 2;
            free(keys); free(sums);
            keys = (uint64_t*)malloc((size_t)n_pool * sizeof(uint64_t));
            sums = (InsPoolSums*)malloc((size_t)n_pool * sizeof(InsPoolSums));
            for (long long i = 0; i < n_pool; i++) {
                unsigned long long key;
                int K, X;
                if (fscanf(fp, "%llx %d %d", &key, &K, &X) != 3) return 2;
                keys[i] = key; sums[i] = {K, X};
            }
        } else if (!strcmp(word, "cell")) {
            unsigned long long key;
            long long k, n, S;
            int own;
            CallModel P;
            if (fscanf(fp, "%llx %lld %lld %lld %d %d %d %d %d %d %d %d", &key, &k, &n, &S, &own, &P.min_depth, &P.min_alt, &P.min_ppm, &P.min_q, &P.a0, &P.n0, &P.bg_max_ppm) != 12)
                return 2;
            int64_t K_o = 0, N_o = 0;
            const bool cand = ins_call_cell(keys, sums, n_pool, key, k, n, S, own != 0, P, &K_o, &N_o);
            const int q = cand ? call_tail_q(k, n, K_o + P.a0, N_o + P.n0, nullptr) : -1;
            printf("%lld %lld %d %d\n", (long long)K_o, (long long)N_o, cand ? 1 : 0, q);
        } else if (!strcmp(word, "find")) {
            unsigned long long key;
            if (fscanf(fp, "%llx", &key) != 1) return 2;
            printf("%lld\n", (long long)ins_pool_find(keys, n_pool, key));
        } else if (!strcmp(word, "add")) {
            long long k, n;
            int bg;
            if (fscanf(fp, "%lld %lld %d", &k, &n, &bg) != 3) return 2;
            const InsPoolSums c = ins_pool_contribution(k, n, bg);
            printf("%d %d\n", c.K, c.X);
        } else {
            fprintf(stderr, "unknown word %s\n", word);
            return 2;
        }
    }
    free(keys); free(sums);
    fclose(fp);
    return 0;
}
