// insertions_host.cpp — gap_traceback_runs and the allele helpers of mipgen_amd/csrc/gapped_align.h run as a plain C++ program (test infrastructure for
// tests/test_insertions_cpu.py, built with -fsanitize=address,undefined): the band row by row as k_gap_align runs it, the five-plane projection, then the key
// of every insertion run as InsPile packs it for a molecule this side alone observes.  Every array lies in a heap block of its exact size.
//   insertions_host CASES  CASES: one case per line, "q qq M W side min_quality" (q: the consensus read, qq: its quality bytes, M: the template)
//   stdout                 per case "ins runs keys": the insertion bytes per template position (comma separated, 255 = anchor not covered), the run index of
//                          every anchor with a length above 0 (-1 elsewhere) and, for those anchors in ascending t, the key in hex (- if there is none)
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
    if (argc != 2) { fprintf(stderr, "usage: insertions_host CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "insertions_host: can't read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string qs, qqs, ms;
        int W = 0, side = 0, min_q = 0;
        if (!(ls >> qs >> qqs >> ms >> W >> side >> min_q) || qs.empty() || qqs.size() != qs.size() || ms.empty() || W < 1 || W > GAP_MAX_INDEL ||
            (side != GAP_EXT && side != GAP_LIG)) {
            fprintf(stderr, "insertions_host: bad case: %s\n", line.c_str());
            return 2;
        }
        const int m = (int)qs.size(), L = (int)ms.size(), rows = std::min(m, L + W);
        uint8_t* q = (uint8_t*)malloc((size_t)m);
        uint8_t* qq = (uint8_t*)malloc((size_t)m);
        uint8_t* M = (uint8_t*)malloc((size_t)L);
        int* h_prev = (int*)malloc(GAP_LANES * sizeof(int));
        int* h = (int*)malloc(GAP_LANES * sizeof(int));
        uint32_t* dirs = (uint32_t*)malloc((size_t)rows * 2 * sizeof(uint32_t));
        uint8_t* proj = (uint8_t*)malloc((size_t)L * 5);
        uint8_t* plain = (uint8_t*)malloc((size_t)L * 3);
        memcpy(q, qs.data(), (size_t)m); memcpy(qq, qqs.data(), (size_t)m); memcpy(M, ms.data(), (size_t)L);
        for (int t = 0; t < L; t++) {
            proj[t] = plain[t] = 0; proj[L + t] = plain[L + t] = 0; proj[2 * L + t] = plain[2 * L + t] = GAP_NOT_COVERED;
            proj[3 * L + t] = proj[4 * L + t] = 0xEE;                   // (never read where the insertion byte is 0 or 255)
        }
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
        const int gaps = gap_traceback_runs(dirs, W, L, side, ie, je, q, qq, proj, proj + L, proj + 2 * L, proj + 3 * L, proj + 4 * L, nullptr);
        // the sibling leaves the three planes of DESIGN 4.13 as the function of old does
        if (gap_traceback(dirs, W, L, side, ie, je, q, qq, plain, plain + L, plain + 2 * L, nullptr) != gaps || memcmp(plain, proj, (size_t)L * 3) != 0) {
            fprintf(stderr, "insertions_host: the two tracebacks differ: %s\n", line.c_str());
            return 1;
        }
        for (int t = 0; t < L; t++) printf("%s%d", t ? "," : "", (int)proj[2 * L + t]);
        printf(" ");
        for (int t = 0; t < L; t++) {
            const int l = proj[2 * L + t];
            printf("%s%d", t ? "," : "", l > 0 && l != GAP_NOT_COVERED ? (int)proj[3 * L + t] | ((int)proj[4 * L + t] << 8) : -1);
        }
        printf(" ");
        bool any = false;
        for (int t = 0; t < L; t++) {
            const int l = proj[2 * L + t];
            if (l == 0 || l == GAP_NOT_COVERED) continue;
            const int at = (int)proj[3 * L + t] | ((int)proj[4 * L + t] << 8);
            uint32_t bases = 0;
            bool amb = l > GAP_ALLELE_MAX_LEN;
            for (int j = 0; j < l && !amb; j++) {
                const int x = gap_run_index(side, at, l, j);
                if (x < 0 || x >= m) { fprintf(stderr, "insertions_host: run index %d of a read of %d bases: %s\n", x, m, line.c_str()); return 1; }
                const int b = side == GAP_LIG ? gap_complement(q[x]) : q[x];
                const bool usable = gap_base_code(b) < 4 && (int)qq[x] - 33 >= min_q;
                const int c = side == GAP_LIG ? gap_allele_base(0, false, b, usable) : gap_allele_base(b, usable, 0, false);
                amb = c > 3;
                bases = (bases << 2) | (uint32_t)(c & 3);
            }
            const uint64_t key = gap_allele_key(t, l, amb, bases);
            if (gap_allele_pos(key) != t || gap_allele_length(key) != l || gap_allele_ambiguous(key) != amb || gap_allele_bases(key) != (amb ? 0u : bases)) {
                fprintf(stderr, "insertions_host: a key does not decode to what it was made of: %s\n", line.c_str());
                return 1;
            }
            printf("%s%llx", any ? "," : "", (unsigned long long)key);
            any = true;
        }
        printf("%s\n", any ? "" : "-");
        free(plain); free(proj); free(dirs); free(h); free(h_prev); free(M); free(qq); free(q);
    }
    return 0;
}
