// gapped_align.h — the banded, anchored alignment of one consensus read against its probe's template, as the pieces k_gap_align (kernels_gapped.hip)
// is made of: the score, the cell, the step of the in-row scan, the direction under each side's preference, the end rule and the traceback.  Every piece is
// __host__ __device__ and reads nothing but its arguments, so a plain C++ program can include this file without HIP and run the same band row by row
// (gap_row_serial below; tests/gapped_host.cpp does, under the sanitizers).
//
// Layout of the band: row i holds its 2W + 1 cells in LANES, lane d being the cell (i, j = i + d - W).  The diagonal predecessor (i - 1, j - 1) is then the same
// lane of the row before, the insertion predecessor (i - 1, j) lane d + 1 of the row before, and the deletion predecessor (i, j - 1) lane d - 1 of the SAME row.
// Because the gap is linear, that in-row dependency is a prefix maximum: with V[d] the best of the two candidates from the row before,
// H[d] = max over k <= d of (V[k] - 2 (d - k)) = (prefix max of V[k] + 2 k) - 2 d.  Serially that is run = max(run - 2, V[d]) (gap_scan_step).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GAP_HD __host__ __device__ static inline
#else
#define GAP_HD static inline
#endif

#define GAP_MAX_INDEL 15             // W: the band is |i - j| <= W, 2 W + 1 <= 31 lanes
#define GAP_MAX_MOL 2048             // the longest template a call accepts: k_gap_align keeps 8 bytes of directions per row in LDS, (2048 + 15) rows x 2 sides = 33,008 bytes
#define GAP_LANES 32
#define GAP_NEG (-(1 << 24))         // "minus infinity": every real score lies within +-2 (GAP_MAX_MOL + GAP_MAX_INDEL) x 2
#define GAP_STOP 0
#define GAP_DIAG 1
#define GAP_DEL 2                    // a template base without a read base: (i, j - 1) -> (i, j)
#define GAP_INS 3                    // a read base without a template base: (i - 1, j) -> (i, j)
#define GAP_EXT 0
#define GAP_LIG 1
#define GAP_NOT_COVERED 0xFF         // the insertion byte of a template position whose anchor (t, t + 1) the side does not cover

GAP_HD int gap_base_code(int c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

GAP_HD int gap_complement(int c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

// +1 equal, -1 different, 0 if either byte is not one of A C G T
GAP_HD int gap_score(int a, int b)
{
    if (gap_base_code(a) > 3 || gap_base_code(b) > 3) return 0;
    return a == b ? 1 : -1;
}

// byte x of r: the template itself on the extension side, its reverse complement on the ligation side
GAP_HD int gap_template_byte(const uint8_t* M, int L, int side, int x) { return side == GAP_LIG ? gap_complement(M[L - 1 - x]) : M[x]; }

GAP_HD bool gap_in_band(int i, int d, int W, int L)
{
    const int j = i + d - W;
    return d <= 2 * W && j >= 0 && j <= L;
}

GAP_HD int gap_clip(int h) { return h < GAP_NEG / 2 ? GAP_NEG : h; }

// the two candidates that come from the row before
GAP_HD int gap_cand_diag(int h_diag, int score) { return gap_clip(h_diag + score); }
GAP_HD int gap_cand_ins(int h_up) { return gap_clip(h_up - 2); }
GAP_HD int gap_cand_del(int h_left) { return gap_clip(h_left - 2); }

// one step of the serial scan over the lanes of a row: what the prefix maximum of V[k] + 2 k computes in registers
GAP_HD int gap_scan_step(int run, int v) { return run - 2 > v ? run - 2 : v; }

// the direction stored for a cell whose value is h: the first candidate that reaches it, in the side's order (extension: diagonal, deletion, insertion;
// ligation: deletion, insertion, diagonal - an indel inside a repeat then lands on the same, lowest template position in M's orientation from both sides)
GAP_HD int gap_dir(int h, int cand_diag, int cand_del, int cand_ins, int side)
{
    if (h == GAP_NEG) return GAP_STOP;
    const bool di = cand_diag == h, de = cand_del == h, in = cand_ins == h;
    if (side == GAP_LIG) return de ? GAP_DEL : in ? GAP_INS : di ? GAP_DIAG : GAP_STOP;
    return di ? GAP_DIAG : de ? GAP_DEL : in ? GAP_INS : GAP_STOP;
}

// The end rule as one comparable number: the larger key wins.  Largest H; then the smallest |j - i|; then the larger j; then (a tie the three leave open: two
// cells of column L, k rows above and k rows below the diagonal) the smaller i.  0 is below every key.
GAP_HD uint64_t gap_end_key(int h, int i, int j)
{
    const int off = j > i ? j - i : i - j;
    return ((uint64_t)(uint32_t)(h + (1 << 20)) << 40) | ((uint64_t)(uint32_t)(GAP_MAX_INDEL - off) << 32) | ((uint64_t)(uint32_t)j << 16) | (uint64_t)(uint32_t)(65535 - i);
}
GAP_HD int gap_end_score(uint64_t key) { return (int)(uint32_t)(key >> 40) - (1 << 20); }
GAP_HD int gap_end_i(uint64_t key) { return 65535 - (int)(key & 0xffffu); }
GAP_HD int gap_end_j(uint64_t key) { return (int)((key >> 16) & 0xffffu); }

// the direction of cell (i, j) from the two bit planes a row leaves (dirs[2 (i - 1)]: bit 0 of every lane, dirs[2 (i - 1) + 1]: bit 1); row 0 is not stored: its
// cells have the deletion as their one candidate
GAP_HD int gap_dir_at(const uint32_t* dirs, int i, int j, int W)
{
    if (i == 0) return j > 0 ? GAP_DEL : GAP_STOP;
    const int d = j - i + W;
    const uint32_t* w = dirs + 2 * (size_t)(i - 1);
    return (int)((w[0] >> d) & 1u) | (int)(((w[1] >> d) & 1u) << 1);
}

// The walk back from the end cell (ie, je) to (0, 0), writing the side's projection onto the template for every column it consumes (1..je): per template position
// t (orientation of M: column j is t = j - 1 on the extension side, t = L - j on the ligation side) the base byte - the read base, complemented on the ligation
// side, or '-' for a deletion -, its quality byte (0 for a deletion) and the insertion byte: the insertion steps between t and t + 1 if the side consumes both,
// GAP_NOT_COVERED if not.  Insertion steps at column 0 and after column je are dropped.  The caller writes the positions the path does not consume (0, 0,
// GAP_NOT_COVERED).  Returns the gap steps of the path, dropped insertion steps included; path (may be null) receives the steps from the end cell backwards as
// 'M', 'D', 'I' and a closing 0 - at most ie + je + 1 bytes.
// RUNS: beside every insertion byte it writes, the walk also leaves the read index of the run - the i it holds when it consumes the column in front
// of the run, so that the run is q[i .. i + length - 1] - as two byte planes run_lo / run_hi (i <= GAP_MAX_MOL + GAP_MAX_INDEL < 2^16).  The insertion steps dropped
// at column 0 have moved i like any other.
template <bool RUNS>
GAP_HD int gap_traceback_core(const uint32_t* dirs, int W, int L, int side, int ie, int je, const uint8_t* q, const uint8_t* qq, uint8_t* base, uint8_t* qual, uint8_t* ins,
                              uint8_t* run_lo, uint8_t* run_hi, char* path)
{
    int i = ie, j = je, run = 0, gaps = 0, n = 0;
    while (i > 0 || j > 0) {
        const int dir = gap_dir_at(dirs, i, j, W);
        if (dir == GAP_STOP) break;                                             // (never for a cell the fill reached)
        if (dir == GAP_INS) {
            i--; run++; gaps++;
            if (path) path[n++] = 'I';
            continue;
        }
        const int t = side == GAP_LIG ? L - j : j - 1;
        const int at = i;                                                       // q[0, at) is consumed through column j: the run behind it starts at q[at]
        if (dir == GAP_DIAG) {
            base[t] = (uint8_t)(side == GAP_LIG ? gap_complement(q[i - 1]) : q[i - 1]);
            qual[t] = qq[i - 1];
            i--;
        } else {
            base[t] = '-'; qual[t] = 0; gaps++;
        }
        // `run` insertion steps lie between column j and column j + 1
        if (side == GAP_LIG) {
            if (j < je) {                                                       // the anchor is the lower position: that of column j + 1
                ins[t - 1] = (uint8_t)run;
                if (RUNS) { run_lo[t - 1] = (uint8_t)at; run_hi[t - 1] = (uint8_t)(at >> 8); }
            }
            if (j == 1) ins[t] = GAP_NOT_COVERED;                               // t = L - 1 anchors nothing
        } else {
            ins[t] = j < je ? (uint8_t)run : (uint8_t)GAP_NOT_COVERED;
            if (RUNS && j < je) { run_lo[t] = (uint8_t)at; run_hi[t] = (uint8_t)(at >> 8); }
        }
        if (path) path[n++] = dir == GAP_DIAG ? 'M' : 'D';
        run = 0; j--;
    }
    if (path) path[n] = 0;
    return gaps;
}

GAP_HD int gap_traceback(const uint32_t* dirs, int W, int L, int side, int ie, int je, const uint8_t* q, const uint8_t* qq, uint8_t* base, uint8_t* qual, uint8_t* ins, char* path)
{
    return gap_traceback_core<false>(dirs, W, L, side, ie, je, q, qq, base, qual, ins, nullptr, nullptr, path);
}

GAP_HD int gap_traceback_runs(const uint32_t* dirs, int W, int L, int side, int ie, int je, const uint8_t* q, const uint8_t* qq, uint8_t* base, uint8_t* qual, uint8_t* ins,
                              uint8_t* run_lo, uint8_t* run_hi, char* path)
{
    return gap_traceback_core<true>(dirs, W, L, side, ie, je, q, qq, base, qual, ins, run_lo, run_hi, path);
}

// ---- insertion alleles ----------------------------------------------------------------------------------------------------------------------
#define GAP_ALLELE_MAX_LEN 15        // the bases an allele spells out: 2 bits each in the 30 low bits of its key

// Base j (orientation of M) of a side's run of l read bases starting at q[at]: its index in the read.  Extension: at + j; ligation: at + l - 1 - j (the byte is then
// complemented).
GAP_HD int gap_run_index(int side, int at, int l, int j) { return side == GAP_LIG ? at + l - 1 - j : at + j; }

// One base of an event from the one or two contributing sides: 0..3, or 4 = ambiguous.  be / bl: each side's byte in M's orientation (the ligation byte complemented
// already), ue / ul: the side contributes and its byte is usable (one of A C G T, quality - 33 >= min_quality).
GAP_HD int gap_allele_base(int be, bool ue, int bl, bool ul)
{
    if (ue && ul) return be == bl ? gap_base_code(be) : 4;
    return ue ? gap_base_code(be) : ul ? gap_base_code(bl) : 4;
}

// The 64-bit key of an allele: x << 35 | l << 31 | ambiguous << 30 | bases, x < 2^29, bases 2 bits per base with base 0 in the most significant of the 2 l used
// bits.  A run of more than GAP_ALLELE_MAX_LEN bases (up to 2 W: deletions in front of it make the room inside the band) spells nothing out: it is ambiguous,
// its length field is 0 - no other event has that - and its length stands in the low bits.
GAP_HD uint64_t gap_allele_key(int64_t x, int l, bool ambiguous, uint32_t bases)
{
    if (l > GAP_ALLELE_MAX_LEN) return ((uint64_t)x << 35) | ((uint64_t)1 << 30) | (uint64_t)(uint32_t)l;
    return ((uint64_t)x << 35) | ((uint64_t)(uint32_t)l << 31) | ((uint64_t)(ambiguous ? 1u : 0u) << 30) | (uint64_t)(ambiguous ? 0u : bases);
}
GAP_HD int64_t gap_allele_pos(uint64_t key) { return (int64_t)(key >> 35); }
GAP_HD bool gap_allele_ambiguous(uint64_t key) { return ((key >> 30) & 1u) != 0; }
GAP_HD int gap_allele_length(uint64_t key) { const int l = (int)((key >> 31) & 15u); return l ? l : (int)(key & 0x3fffffffu); }
GAP_HD uint32_t gap_allele_bases(uint64_t key) { return ((key >> 31) & 15u) ? (uint32_t)(key & 0x3fffffffu) : 0u; }

// ---- insertion alleles per genome locus -----------------------------------------------------------------------------------------------------
// The reverse complement of the l bases (1..GAP_ALLELE_MAX_LEN) of an allele over the 2-bit codes: base j becomes 3 - base(l - 1 - j), base 0 still in the most
// significant of the 2 l used bits.  Complement = every used bit flipped; the reverse = the sixteen 2-bit groups of the word swapped end for end, then shifted down.
GAP_HD uint32_t gap_allele_revcomp(uint32_t bases, int l)
{
    uint32_t v = ~bases & ((1u << (2 * l)) - 1u);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32 - 2 * l);
}

// The key of the locus allele a record (length l, ambiguous, bases) becomes under the plan word `word` = locus << 2 | flags of the source that pulls it: the
// position is the locus; a non-ambiguous record turns under bit 0; an ambiguous one - a run above GAP_ALLELE_MAX_LEN included - stays bit for bit what it is.
GAP_HD uint64_t gap_locus_allele_key(uint32_t word, int l, bool ambiguous, uint32_t bases)
{
    const bool turn = (word & 1u) && !ambiguous && l >= 1 && l <= GAP_ALLELE_MAX_LEN;
    return gap_allele_key((int64_t)(word >> 2), l, ambiguous, turn ? gap_allele_revcomp(bases, l) : bases);
}
#define GAP_LOCUS_NONE 0xFFFFFFFFu   // own[a] / prev[a] of an anchor row no source pulls

// ---- deletion alleles -----------------------------------------------------------------------------------------------------------------------
// the class of one observation, and of a molecule at a position: 0..3 = A C G T
#define GAP_CLASS_DEL 4u
#define GAP_CLASS_NONE 5u
#define GAP_CLASS_DISC 6u

// The vote of one molecule at one position from its two usable observations (each 0..3, GAP_CLASS_DEL or GAP_CLASS_NONE; a molecule that is not used brings
// GAP_CLASS_NONE twice): nothing, the one class, the shared class, or discordant.
GAP_HD uint32_t gap_molecule_class(uint32_t ce, uint32_t cl)
{
    const bool ue = ce < GAP_CLASS_NONE, ul = cl < GAP_CLASS_NONE;
    return ue && ul && ce != cl ? GAP_CLASS_DISC : ue ? ce : ul ? cl : GAP_CLASS_NONE;
}

// The molecule is discordant here and one of its two usable observations is a deletion: next to a run of deletions, the two sides disagree on its extent.
GAP_HD bool gap_ragged_flank(uint32_t ce, uint32_t cl) { return gap_molecule_class(ce, cl) == GAP_CLASS_DISC && (ce == GAP_CLASS_DEL || cl == GAP_CLASS_DEL); }

// The consecutive set bits of mask from bit `lane` upwards (0 if that bit is clear, 64 - lane at most): the part of a run of deletions that lies in the 64
// positions of one round.
GAP_HD int gap_mask_run(uint64_t mask, int lane)
{
    const uint64_t clear = ~(mask >> lane);                                     // (the shift brings zeros in from above: set bits here, unless lane is 0)
    return clear == 0 ? 64 : __builtin_ctzll(clear);
}

// The 64-bit key of a deletion allele: x << 35 | l << 1 | ragged, x < 2^29, l <= GAP_MAX_MOL < 2^12.  Ascending: position, then length, then clean before ragged.
GAP_HD uint64_t gap_deletion_key(int64_t x, int l, bool ragged) { return ((uint64_t)x << 35) | ((uint64_t)(uint32_t)l << 1) | (uint64_t)(ragged ? 1u : 0u); }
GAP_HD int64_t gap_deletion_pos(uint64_t key) { return (int64_t)(key >> 35); }
GAP_HD int gap_deletion_length(uint64_t key) { return (int)((key >> 1) & 0xfffu); }
GAP_HD bool gap_deletion_ragged(uint64_t key) { return (key & 1u) != 0; }

// ---- the serial row: what k_gap_align's lanes do for row i >= 1, one lane after the other (host only) ----------------------------------------------------
// h_prev / h: the GAP_LANES values of row i - 1 / i (GAP_NEG outside the band); q_byte = q[i - 1]; two words of directions go to dirs2.
static inline void gap_row_serial(int i, int W, int L, int side, int q_byte, const uint8_t* M, const int* h_prev, int* h, uint32_t* dirs2)
{
    int run = GAP_NEG;
    dirs2[0] = dirs2[1] = 0;
    for (int d = 0; d < GAP_LANES; d++) {
        const int j = i + d - W;
        if (!gap_in_band(i, d, W, L)) { h[d] = GAP_NEG; run = GAP_NEG; continue; }
        const int cd = j >= 1 ? gap_cand_diag(h_prev[d], gap_score(q_byte, gap_template_byte(M, L, side, j - 1))) : GAP_NEG;
        const int ci = d < 2 * W ? gap_cand_ins(h_prev[d + 1]) : GAP_NEG;
        const int cl = d > 0 ? gap_cand_del(h[d - 1]) : GAP_NEG;
        run = gap_clip(gap_scan_step(run, cd > ci ? cd : ci));
        h[d] = run;
        const int dir = gap_dir(run, cd, cl, ci, side);
        dirs2[0] |= (uint32_t)(dir & 1) << d; dirs2[1] |= (uint32_t)((dir >> 1) & 1) << d;
    }
}

// row 0: H(0, j) = -2 j
static inline void gap_row0(int W, int L, int* h)
{
    for (int d = 0; d < GAP_LANES; d++) h[d] = gap_in_band(0, d, W, L) ? -2 * (d - W) : GAP_NEG;
}
