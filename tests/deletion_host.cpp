// deletion_host.cpp — the deletion helpers of mipgen_amd/csrc/gapped_align.h run as a plain C++ program (test infrastructure for tests/test_deletions_cpu.py, built
// with -fsanitize=address,undefined): the class of a molecule from two observations, the ragged bit, the run length inside a 64-bit mask, the packed key and its
// decoders, and a lane-by-lane transcription of DelPile's group body (kernels_gapped.hip) - 64 lanes per round, the shuffle from the lane below, lane 0's extra
// observation, the ballots, the continuation past lane 63, the clamped lanes.  Every array lies in a heap block of its exact size.
//   deletion_host CASES    CASES: one molecule per line, "ce cl": each side's usable observation per template position as a digit (0..3 = A C G T, 4 = del, 5 = none)
//   stdout                 per molecule "classes flanks keys": the voted class per position as a digit (6 = discordant), the ragged-flank bit per position, and the
//                          keys (x = the run's start) of its events in ascending start, in hex, comma separated (- if there is none)
//   deletion_host -self    the in-mask run length against a serial count, and the transcription against the serial rule on random class arrays of 1 to 200 positions
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../mipgen_amd/csrc/gapped_align.h"

struct Event { int a, l; bool ragged; };

// the serial rule: maximal runs of del in the voted classes
static std::vector<Event> serial_events(const uint8_t* ce, const uint8_t* cl, int L)
{
    std::vector<Event> out;
    for (int t = 0; t < L;) {
        if (gap_molecule_class(ce[t], cl[t]) != GAP_CLASS_DEL) { t++; continue; }
        const int a = t;
        while (t < L && gap_molecule_class(ce[t], cl[t]) == GAP_CLASS_DEL) t++;
        out.push_back({a, t - a, (a > 0 && gap_ragged_flank(ce[a - 1], cl[a - 1])) || (t < L && gap_ragged_flank(ce[t], cl[t]))});
    }
    return out;
}

// one observation of the pass: a lane clamped at t == L reads SOMETHING (the device clamps its index); here the worst it could read - a deletion on one side and a
// base on the other, a ragged flank - so that only the `live` guards keep it out
static void observe(const uint8_t* ce, const uint8_t* cl, int L, int t, uint32_t& e, uint32_t& l)
{
    if (t >= L) { e = GAP_CLASS_DEL; l = (uint32_t)(t & 1 ? 0 : GAP_CLASS_DEL); return; }
    e = ce[t]; l = cl[t];
}

// DelPile::groups for one molecule, round after round, lane after lane
static std::vector<Event> lanes_events(const uint8_t* ce, const uint8_t* cl, int L)
{
    std::vector<Event> out;
    bool* del = (bool*)malloc(64 * sizeof(bool));
    bool* rag = (bool*)malloc(64 * sizeof(bool));
    for (int r = 0; r * 64 < L; r++) {
        const int t0 = r * 64;
        uint64_t dels = 0, rags = 0;
        for (int lane = 0; lane < 64; lane++) {
            const int t = t0 + lane < L ? t0 + lane : L;
            uint32_t e, l;
            observe(ce, cl, L, t, e, l);
            const bool live = t < L;
            del[lane] = live && gap_molecule_class(e, l) == GAP_CLASS_DEL;
            rag[lane] = live && gap_ragged_flank(e, l);
            dels |= (uint64_t)del[lane] << lane; rags |= (uint64_t)rag[lane] << lane;
        }
        if (dels == 0) continue;
        bool below_del0 = false, below_rag0 = false;                            // lane 0's neighbour
        if ((dels & 1u) && t0 > 0) {
            uint32_t e, l;
            observe(ce, cl, L, t0 - 1, e, l);
            below_del0 = gap_molecule_class(e, l) == GAP_CLASS_DEL; below_rag0 = gap_ragged_flank(e, l);
        }
        uint64_t starts = 0;
        for (int lane = 0; lane < 64; lane++) {
            const bool below_del = lane ? del[lane - 1] : below_del0;
            if (del[lane] && !below_del) starts |= (uint64_t)1 << lane;
        }
        if (starts == 0) continue;
        bool any_reaches = false;
        for (int lane = 0; lane < 64; lane++)
            if (((starts >> lane) & 1u) && lane + gap_mask_run(dels, lane) == 64) any_reaches = true;
        int more = 0;
        bool end_rag = false;
        if (any_reaches && t0 + 64 < L) {
            for (int tt = t0 + 64; tt < L; tt++) {
                uint32_t e, l;
                observe(ce, cl, L, tt, e, l);
                if (gap_molecule_class(e, l) != GAP_CLASS_DEL) { end_rag = gap_ragged_flank(e, l); break; }
                more++;
            }
        }
        for (int lane = 0; lane < 64; lane++) {
            if (!((starts >> lane) & 1u)) continue;
            int l = gap_mask_run(dels, lane);
            const int after = lane + l;
            bool above_rag = after < 64 && ((rags >> (after & 63)) & 1u);
            if (after == 64 && any_reaches && t0 + 64 < L) { l += more; above_rag = end_rag; }
            const bool below_rag = lane ? rag[lane - 1] : below_rag0;
            out.push_back({t0 + lane, l, below_rag || above_rag});
        }
    }
    free(rag); free(del);
    return out;
}

static bool same(const std::vector<Event>& a, const std::vector<Event>& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].a != b[i].a || a[i].l != b[i].l || a[i].ragged != b[i].ragged) return false;
    return true;
}

static int serial_run(uint64_t mask, int lane)
{
    int n = 0;
    while (lane + n < 64 && ((mask >> (lane + n)) & 1u)) n++;
    return n;
}

static int check_mask(uint64_t mask)
{
    for (int lane = 0; lane < 64; lane++)
        if (gap_mask_run(mask, lane) != serial_run(mask, lane)) {
            fprintf(stderr, "deletion_host: mask %016llx lane %d: %d, serially %d\n", (unsigned long long)mask, lane, gap_mask_run(mask, lane), serial_run(mask, lane));
            return 1;
        }
    return 0;
}

static uint64_t next_random(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s ^ (s >> 29); }

static int self_test()
{
    long masks = 0, arrays = 0, with_events = 0, long_runs = 0;
    if (check_mask(0) || check_mask(~0ull)) return 1;
    masks += 2;
    const int first[4] = {0, 1, 62, 63};
    for (int k = 0; k < 4; k++)
        for (int len = 1; first[k] + len <= 64; len++) {                        // every run from lanes 0, 1, 62, 63: those that end at lane 63 included
            const uint64_t run = (len == 64 ? ~0ull : (((uint64_t)1 << len) - 1)) << first[k];
            if (check_mask(run) || check_mask(run | ((uint64_t)1 << 40)) || check_mask(run | (run >> 7))) return 1;
            masks += 3;
        }
    for (int start = 0; start < 64; start++) {                                  // runs that end at lane 63
        if (check_mask(~0ull << start)) return 1;
        masks++;
    }
    uint64_t s = 88172645463325252ull;
    for (int k = 0; k < 20000; k++) {
        const uint64_t a = next_random(s), b = next_random(s), c = next_random(s);
        if (check_mask(a) || check_mask(a | b) || check_mask(a | b | c)) return 1;
        masks += 3;
    }
    // random class arrays of 1 to 200 positions: long runs of deletions, flanks of every kind, arrays that end inside a run
    for (int k = 0; k < 20000; k++) {
        const int L = 1 + (int)(next_random(s) % 200);
        uint8_t* ce = (uint8_t*)malloc((size_t)L);
        uint8_t* cl = (uint8_t*)malloc((size_t)L);
        const int mode = k % 4;
        for (int t = 0; t < L;) {
            const int kind = (int)(next_random(s) % 6), len = 1 + (int)(next_random(s) % (mode == 0 ? 3 : mode == 1 ? 20 : 90));
            for (int j = 0; j < len && t < L; j++, t++) {
                if (kind <= 1 || (mode == 3 && kind <= 3)) { ce[t] = GAP_CLASS_DEL; cl[t] = (uint8_t)(next_random(s) % 3 ? GAP_CLASS_DEL : GAP_CLASS_NONE); }
                else if (kind == 2) { ce[t] = GAP_CLASS_NONE; cl[t] = GAP_CLASS_DEL; }
                else if (kind == 3) { ce[t] = (uint8_t)(next_random(s) % 4); cl[t] = GAP_CLASS_DEL; }
                else if (kind == 4) { ce[t] = (uint8_t)(next_random(s) % 6); cl[t] = (uint8_t)(next_random(s) % 6); }
                else { ce[t] = cl[t] = (uint8_t)(next_random(s) % 4); }
            }
        }
        const std::vector<Event> want = serial_events(ce, cl, L), got = lanes_events(ce, cl, L);
        if (!same(want, got)) {
            fprintf(stderr, "deletion_host: the lanes differ from the serial rule on an array of %d positions (case %d)\n", L, k);
            return 1;
        }
        arrays++; with_events += !want.empty();
        for (const Event& e : want) long_runs += e.l > 64;
        free(cl); free(ce);
    }
    printf("masks %ld arrays %ld with_events %ld long_runs %ld\n", masks, arrays, with_events, long_runs);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: deletion_host CASES | -self\n"); return 2; }
    if (!strcmp(argv[1], "-self")) return self_test();
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "deletion_host: can't read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string es, lgs;
        if (!(ls >> es >> lgs) || es.empty() || es.size() != lgs.size() || es.size() > GAP_MAX_MOL) { fprintf(stderr, "deletion_host: bad case: %s\n", line.c_str()); return 2; }
        const int L = (int)es.size();
        uint8_t* ce = (uint8_t*)malloc((size_t)L);
        uint8_t* cl = (uint8_t*)malloc((size_t)L);
        for (int t = 0; t < L; t++) {
            if (es[(size_t)t] < '0' || es[(size_t)t] > '5' || lgs[(size_t)t] < '0' || lgs[(size_t)t] > '5') { fprintf(stderr, "deletion_host: bad case: %s\n", line.c_str()); return 2; }
            ce[t] = (uint8_t)(es[(size_t)t] - '0'); cl[t] = (uint8_t)(lgs[(size_t)t] - '0');
        }
        const std::vector<Event> want = serial_events(ce, cl, L), got = lanes_events(ce, cl, L);
        if (!same(want, got)) { fprintf(stderr, "deletion_host: the lanes differ from the serial rule: %s\n", line.c_str()); return 1; }
        for (int t = 0; t < L; t++) printf("%u", gap_molecule_class(ce[t], cl[t]));
        printf(" ");
        for (int t = 0; t < L; t++) printf("%d", gap_ragged_flank(ce[t], cl[t]) ? 1 : 0);
        printf(" ");
        for (size_t k = 0; k < got.size(); k++) {
            const uint64_t key = gap_deletion_key(got[k].a, got[k].l, got[k].ragged);
            if (gap_deletion_pos(key) != got[k].a || gap_deletion_length(key) != got[k].l || gap_deletion_ragged(key) != got[k].ragged) {
                fprintf(stderr, "deletion_host: a key does not decode to what it was made of: %s\n", line.c_str());
                return 1;
            }
            printf("%s%llx", k ? "," : "", (unsigned long long)key);
        }
        printf("%s\n", got.empty() ? "-" : "");
        free(cl); free(ce);
    }
    // the corners of the key: the largest position and the longest run
    const uint64_t top = gap_deletion_key(((int64_t)1 << 29) - 2, GAP_MAX_MOL, true);
    if (gap_deletion_pos(top) != ((int64_t)1 << 29) - 2 || gap_deletion_length(top) != GAP_MAX_MOL || !gap_deletion_ragged(top) ||
        !(gap_deletion_key(5, 3, false) < gap_deletion_key(5, 3, true) && gap_deletion_key(5, 3, true) < gap_deletion_key(5, 4, false) &&
          gap_deletion_key(5, GAP_MAX_MOL, true) < gap_deletion_key(6, 1, false))) {
        fprintf(stderr, "deletion_host: the key's corners or its order are wrong\n");
        return 1;
    }
    return 0;
}
