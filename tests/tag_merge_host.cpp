// tag_merge_host.cpp — the host functions of mipgen_amd/csrc/tag_merge.h run as a plain C++ program (test infrastructure for tests/test_tag_merge_cpu.py, built
// with -fsanitize=address,undefined): every raw group of a sorted key list through tag_parent and tag_root, as k_tag_parent and k_tag_root run them a lane per group;
// every array in a heap block of its exact size.
//   tag_merge_host CASES   CASES: one case per line, "L n key_0 family_0 ... key_(n-1) family_(n-1)" (L tag bases; the keys ascending, distinct, decimal 64-bit)
//   stdout                 per case one line of n "parent:root:depth" entries (parent -1: a root), or "unended" where a walk did not end
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../mipgen_amd/csrc/tag_merge.h"

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: tag_merge_host CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "tag_merge_host: can't read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        int L = 0;
        long long n = 0;
        if (!(ls >> L >> n) || L < 1 || L > 16 || n < 1) { fprintf(stderr, "tag_merge_host: bad case: %s\n", line.c_str()); return 2; }
        uint64_t* keys = (uint64_t*)malloc((size_t)n * sizeof(uint64_t));
        int32_t* family = (int32_t*)malloc((size_t)n * sizeof(int32_t));
        int32_t* parent = (int32_t*)malloc((size_t)n * sizeof(int32_t));
        for (long long g = 0; g < n; g++) {
            unsigned long long k = 0;
            long long f = 0;
            if (!(ls >> k >> f) || f < 1 || f > 0x7fffffffLL || (g && k <= keys[g - 1])) { fprintf(stderr, "tag_merge_host: bad group %lld: %s\n", g, line.c_str()); return 2; }
            keys[g] = k; family[g] = (int32_t)f;
        }
        for (long long g = 0; g < n; g++) parent[g] = (int32_t)tag_parent(keys, family, n, g, L);
        for (long long g = 0; g < n; g++) {
            int64_t root = 0;
            int depth = 0;
            if (tag_root(parent, n, g, &root, &depth)) printf("%s%d:%lld:%d", g ? " " : "", parent[g], (long long)root, depth);
            else printf("%sunended", g ? " " : "");
        }
        printf("\n");
        free(parent); free(family); free(keys);
    }
    return 0;
}
