// gapped_host.cpp — the host functions of mipgen_amd/csrc/gapped_align.h run as a plain C++ program (test infrastructure for tests/test_gapped_cpu.py, built
// with -fsanitize=address,undefined): the band row by row as k_gap_align runs it, every array in a heap block of its exact size.
//   gapped_host CASES      CASES: one case per line, "q M W side" (q: the consensus read, at least one byte; M: the template; side 0 extension, 1 ligation)
//   stdout                 per case "ie je score path bases ins": the end cell, its score, the path from (0, 0) as M / D / I, the projection's base bytes per
//                          template position ('.' for none) and its insertion bytes (comma separated, 255 = anchor not covered)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../mipgen_amd/csrc/gapped_align.h"

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: gapped_host CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "gapped_host: can't read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string qs, ms;
        int W = 0, side = 0;
        if (!(ls >> qs >> ms >> W >> side) || qs.empty() || ms.empty() || W < 1 || W > GAP_MAX_INDEL || (side != GAP_EXT && side != GAP_LIG)) {
            fprintf(stderr, "gapped_host: bad case: %s\n", line.c_str());
            return 2;
        }
        const int m = (int)qs.size(), L = (int)ms.size(), rows = std::min(m, L + W);
        uint8_t* q = (uint8_t*)malloc((size_t)m);
        uint8_t* qq = (uint8_t*)malloc((size_t)m);
        uint8_t* M = (uint8_t*)malloc((size_t)L);
        int* h_prev = (int*)malloc(GAP_LANES * sizeof(int));
        int* h = (int*)malloc(GAP_LANES * sizeof(int));
        uint32_t* dirs = (uint32_t*)malloc((size_t)rows * 2 * sizeof(uint32_t));
        uint8_t* proj = (uint8_t*)malloc((size_t)L * 3);
        memcpy(q, qs.data(), (size_t)m); memcpy(M, ms.data(), (size_t)L);
        memset(qq, 'I', (size_t)m);
        for (int t = 0; t < L; t++) { proj[t] = 0; proj[L + t] = 0; proj[2 * L + t] = GAP_NOT_COVERED; }
        gap_row0(W, L, h_prev);
        uint64_t best = 0;
        for (int d = 0; d < GAP_LANES; d++)
            if (gap_in_band(0, d, W, L) && d - W == L) best = std::max(best, gap_end_key(h_prev[d], 0, L));
        for (int i = 1; i <= rows; i++) {
            gap_row_serial(i, W, L, side, q[i - 1], M, h_prev, h, dirs + 2 * (size_t)(i - 1));
            for (int d = 0; d < GAP_LANES; d++) {
                const int j = i + d - W;
                if (gap_in_band(i, d, W, L) && (j == L || i == m)) best = std::max(best, gap_end_key(h[d], i, j));
            }
            std::swap(h, h_prev);
        }
        const int ie = gap_end_i(best), je = gap_end_j(best);
        char* path = (char*)malloc((size_t)ie + (size_t)je + 1);
        gap_traceback(dirs, W, L, side, ie, je, q, qq, proj, proj + L, proj + 2 * L, path);
        std::string fwd(path);
        std::reverse(fwd.begin(), fwd.end());
        std::string bases((size_t)L, '.');
        for (int t = 0; t < L; t++) if (proj[t]) bases[(size_t)t] = (char)proj[t];
        printf("%d %d %d %s %s ", ie, je, gap_end_score(best), fwd.c_str(), bases.c_str());
        for (int t = 0; t < L; t++) printf("%s%d", t ? "," : "", (int)proj[2 * L + t]);
        printf("\n");
        free(path); free(proj); free(dirs); free(h); free(h_prev); free(M); free(qq); free(q);
    }
    return 0;
}
