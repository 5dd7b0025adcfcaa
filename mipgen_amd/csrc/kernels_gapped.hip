// kernels_gapped.hip — the pileup with indels: every consensus read placed on its probe's template by a banded, anchored alignment, then allele, deletion and
// insertion counts per template position.  The cell boundaries, the (cell, round) units and the used groups are kernels_pileup.hip's
// (mipgen_launch_pileup_prepare); the pieces of the alignment are gapped_align.h's.
//
//  k_gap_screen   a WAVEFRONT per group of the row, LANES OVER POSITIONS, both sides in turn: does the side need the dynamic program?  THE EXACT SHORTCUT: a side
//                 whose k = min(m, L) leading bases all equal r (A C G T on both) has the ungapped path as its model path.  (1) A path holds at most min(i, j) <= k
//                 diagonal steps, each worth at most +1, and every gap step costs 2: k is the largest score any path reaches, and only the path of k diagonal
//                 steps reaches it.  (2) That path ends at (k, k), an end cell (i == m or j == L) with |j - i| = 0; every other end cell scores less, so no tie
//                 is broken.  (3) On the path H(c, c) = c, while the gap candidates are H(c, c - 1) - 2 <= c - 3 and H(c - 1, c) - 2 <= c - 3: no cell of the
//                 path has a tied candidate, so the traceback has no choice.  Such a side gets no projection; the count reads its consensus read as 4.12 does.
//                 A side of an unused group (family < min_family) or of length 0 is not listed either: it observes nothing.
//  k_gap_list     a lane per (group, side): the listed sides reserve a slot of list[] and 3 L bytes of the projection buffer, by a wavefront scan and one atomic
//                 per wavefront and counter, as k_pileup_partition reserves its slots.  The order of the slots is not defined; nothing depends on it.
//  k_gap_align    HALF A WAVEFRONT per listed side, lanes over the 2 W + 1 <= 31 diagonals of the band, rows in sequence.  The template byte of a lane moves one
//                 lane down per row (the new one enters at lane 2 W); query and template come in 32-row chunks, a byte per lane, loaded one chunk ahead and
//                 handed out by __shfl, so no row waits for memory.  The in-row dependency is a prefix maximum of V + 2 d over the 32 lanes (five __shfl_up
//                 steps of width 32).  Per row two words of directions (two ballots) go to LDS: 8 bytes per row and side.  Then the 32 lanes reduce the end
//                 key, lane 0 walks back and writes the projection of the consumed columns, and the half fills the rest.
//  GapPile        the vote of the gapped table, plugged into the count frame of pileup_frame.h: k_gapped_wave = k_pile_wave<GapPile, GapProj>, k_gapped_wg =
//                 k_pile_wg<GapPile, GapProj>, k_gapped_sum = k_pile_sum<GapPile>.  Eight counters; a side with a projection is read from it (base, quality and
//                 insertion byte at t), any other from its consensus read.  32 bytes per position, two 16-byte stores.  Column sums: bases (columns 0..3),
//                 discordant, deletions, insertions, ins_discordant (columns 4..7).
//
// Insertion alleles.  k_gap_list<5> and k_gap_align<true> are the same kernels with the WIDER projection: two more byte planes hold, per anchor, the
// read index of the insertion run (gap_traceback_runs).  The 3-plane instances are the code of 4.13 as it was.
//  InsPile        a second policy of the count frame, k_ins_wave / k_ins_wg: four counters per anchor (span, ins, ins_discordant, ambiguous; one 16-byte store) from
//                 the insertion bytes alone, and THE EVENTS as a side effect: a ballot of the lanes whose molecule carries an agreed insertion at their anchor;
//                 only where it is non-zero, one atomic per wavefront reserves the slots, every such lane reads its <= 15 bases and qualities from the one or two
//                 consensus reads through the run indices, votes per base, packs the key (gap_allele_key) and writes it with one 8-byte store.  The group loop is
//                 wave-uniform, so the ballot sees the whole wavefront.  The slots are exact beforehand: the `insertions` total of the GapPile count.
//  k_ins_records  a lane per run of the sorted keys (mipgen_consensus_sort, mipgen_consensus_runs): key and count decoded into a 24-byte record.
//
// Deletion alleles, over the three-plane projections of 4.13.
//  DelPile        a third policy of the count frame, k_del_wave / k_del_wg: four counters per position (depth, starts, ragged, del; one 16-byte store) from the voted
//                 class of every molecule, and the maximal runs of `del` along a molecule as events: a start lane is one that votes del while the lane below does
//                 not (a shuffle; lane 0 of a later round observes t - 1 itself), the length the consecutive set bits of the ballot of del lanes and, past lane 63,
//                 direct observations.  The slots are bounded beforehand by the `deletions` total of the GapPile count.
//  k_del_records  a lane per run of the sorted keys: key and count decoded into a 24-byte record, its depth read from the sites table.
#include "pileup_frame.h"
#include "gapped_align.h"

struct GapIn {
    ConsensusView C;
    PileRow R;
    const uint8_t* __restrict__ mol_seq;      // the templates, concatenated: probe p at R.pos_off[p]
    uint32_t g_first;                         // the row's first group
    int W;
};

// need[2 gi + side] for the row's groups gi = g - g_first
__global__ __launch_bounds__(256) void k_gap_screen(GapIn I, int64_t n_row_groups, uint8_t* __restrict__ need)
{
    const int64_t gi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gi >= n_row_groups) return;                                                         // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const uint32_t g = I.g_first + (uint32_t)gi;
    const uint32_t p = (uint32_t)(I.C.keys[g] >> 32) - I.R.cell0;
    const int L = I.R.mol_len[p];
    const uint8_t* __restrict__ M = I.mol_seq + I.R.pos_off[p];
    const bool used = I.C.family[g] >= I.R.min_family;
    for (int side = 0; side < 2; side++) {
        const int64_t o = side ? I.C.lig_off[g] : I.C.ext_off[g];
        const int m = (int)((side ? I.C.lig_off[g + 1] : I.C.ext_off[g + 1]) - o);
        const uint8_t* __restrict__ q = (side ? I.C.lig_seq : I.C.ext_seq) + o;
        const int k = used ? min(m, L) : 0;
        bool differs = false;
        for (int x0 = 0; x0 < k && !differs; x0 += 64) {                                    // (differs is the wavefront's: it comes from a ballot)
            const int x = x0 + lane;
            bool bad = false;
            if (x < k) {
                const int a = q[x], b = gap_template_byte(M, L, side, x);
                bad = a != b || gap_base_code(a) > 3;
            }
            differs = __ballot(bad) != 0ull;
        }
        if (lane == 0) need[2 * gi + side] = differs ? 1 : 0;
    }
}

// PLANES: the byte planes of a projection - 3 (base, quality, insertion length: DESIGN 4.13) or 5 (and the two bytes of the run index: 4.16)
template <int PLANES>
__global__ __launch_bounds__(256) void k_gap_list(GapIn I, int64_t n_row_sides, const uint8_t* __restrict__ need, uint32_t* __restrict__ list, int64_t* __restrict__ proj_off,
                                                  GappedCounters* __restrict__ ctr)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool listed = s < n_row_sides && need[s];
    uint32_t bytes = 0;
    if (listed) {
        const uint32_t g = I.g_first + (uint32_t)(s >> 1);
        bytes = (uint32_t)PLANES * (uint32_t)I.R.mol_len[(uint32_t)(I.C.keys[g] >> 32) - I.R.cell0];
    }
    const uint32_t in = wave_inclusive_sum_u32(listed ? 1u : 0u, lane), ib = wave_inclusive_sum_u32(bytes, lane);       // (at most 64 x 5 x GAP_MAX_MOL bytes per wavefront)
    const uint32_t tn = __shfl(in, 63), tb = __shfl(ib, 63);
    unsigned long long bn = 0, bb = 0;
    if (lane == 0 && tn) { bn = atomicAdd(&ctr->n_sides, (unsigned long long)tn); bb = atomicAdd(&ctr->proj_bytes, (unsigned long long)tb); }
    bn = __shfl(bn, 0); bb = __shfl(bb, 0);
    if (s < n_row_sides) proj_off[s] = listed ? (int64_t)(bb + (ib - bytes)) : -1;
    if (listed) list[bn + (in - 1u)] = (uint32_t)s;
}

// ---- the alignment ------------------------------------------------------------------------------------------------------------------------------------
// Dynamic LDS: [2 halves][rows_cap][2] words of directions; rows_cap = (the longest template of the call) + W >= min(m, L + W), the rows of any side.
extern __shared__ uint32_t gap_dirs[];

// RUNS: the side's projection has five planes and the walk back leaves the run indices in the last two
template <bool RUNS>
__global__ __launch_bounds__(64) void k_gap_align(const uint32_t* __restrict__ list, int64_t n_sides, const int64_t* __restrict__ proj_off, uint8_t* __restrict__ proj, GapIn I,
                                                  int rows_cap, GappedCounters* __restrict__ ctr)
{
    const int lane = threadIdx.x, half = lane >> 5, d = lane & 31;
    const int64_t slot = (int64_t)blockIdx.x * 2 + half;
    const bool live = slot < n_sides;
    const int W = I.W;
    const uint32_t s = list[live ? slot : 0];                                               // (a half without a side reads slot 0 and does nothing with it)
    const uint32_t g = I.g_first + (s >> 1);
    const int side = (int)(s & 1u);
    const uint32_t p = (uint32_t)(I.C.keys[g] >> 32) - I.R.cell0;
    const int L = I.R.mol_len[p];
    const uint8_t* __restrict__ M = I.mol_seq + I.R.pos_off[p];
    const int64_t qo = side ? I.C.lig_off[g] : I.C.ext_off[g];
    const int m = live ? (int)((side ? I.C.lig_off[g + 1] : I.C.ext_off[g + 1]) - qo) : 0;
    const uint8_t* __restrict__ q = (side ? I.C.lig_seq : I.C.ext_seq) + qo;
    const uint8_t* __restrict__ qq = (side ? I.C.lig_qual : I.C.ext_qual) + qo;
    const int rows = min(min(m, L + W), rows_cap);                                          // rows beyond L + W lie outside the band; (rows_cap >= L + W: the host's)
    const int rows_all = max(rows, __shfl_xor(rows, 32));
    uint32_t* dirs = gap_dirs + (size_t)half * (size_t)rows_cap * 2;

    // row 0
    int H = gap_in_band(0, d, W, L) ? -2 * (d - W) : GAP_NEG;
    uint64_t best = 0;
    if (live && H != GAP_NEG && d - W == L) best = gap_end_key(H, 0, L);                    // (m >= 1 for a listed side: row 0 is an end row for column L only)
    // lane d holds the template byte of its cell's column: r[i + d - W - 1] in row i
    int rwin = 0;
    { const int x = d - W - 1; if (live && x >= 0 && x < L) rwin = gap_template_byte(M, L, side, x); }
    // chunks of 32 rows: lane k holds q[c + k] and r[c + k + W], c = 32 (chunk)
    auto q_at = [&](int x) { return live && x < m ? (int)q[x] : 0; };
    auto r_at = [&](int x) { return live && x < L ? gap_template_byte(M, L, side, x) : 0; };
    int q_next = q_at(d), r_next = r_at(d + W), q_chunk = 0, r_chunk = 0;
    for (int i = 1; i <= rows_all; i++) {
        const int k = (i - 1) & 31;
        if (k == 0) { q_chunk = q_next; r_chunk = r_next; q_next = q_at(i + 31 + d); r_next = r_at(i + 31 + d + W); }
        const int qb = __shfl(q_chunk, k, 32), r_new = __shfl(r_chunk, k, 32);
        const int r_down = __shfl_down(rwin, 1, 32);
        rwin = d == 2 * W ? r_new : r_down;
        const int j = i + d - W;
        const bool valid = i <= rows && gap_in_band(i, d, W, L);
        int up = __shfl_down(H, 1, 32);
        if (d >= 2 * W) up = GAP_NEG;
        const int cd = j >= 1 ? gap_cand_diag(H, gap_score(qb, rwin)) : GAP_NEG, ci = gap_cand_ins(up);
        int X = (valid ? max(cd, ci) : GAP_NEG) + 2 * d;
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
            const int u = __shfl_up(X, off, 32);
            if (d >= off) X = max(X, u);
        }
        H = valid ? gap_clip(X - 2 * d) : GAP_NEG;
        int left = __shfl_up(H, 1, 32);
        if (d == 0) left = GAP_NEG;
        const int dir = valid ? gap_dir(H, cd, gap_cand_del(left), ci, side) : GAP_STOP;
        const unsigned long long b0 = __ballot(dir & 1), b1 = __ballot(dir & 2);
        if (d == 0 && i <= rows) { dirs[2 * (i - 1)] = (uint32_t)(b0 >> (32 * half)); dirs[2 * (i - 1) + 1] = (uint32_t)(b1 >> (32 * half)); }
        if (valid && (j == L || i == m)) { const uint64_t key = gap_end_key(H, i, j); best = key > best ? key : best; }
    }
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)best, off, 32);
        best = o > best ? o : best;
    }
    // the walk back: lane 0 of the half (the lane that wrote the directions)
    const int je = gap_end_j(best);
    const int64_t po = live ? proj_off[s] : 0;
    uint8_t* base = proj + po;
    int gaps = 0;
    if constexpr (RUNS) {
        if (live && d == 0 && best != 0)
            gaps = gap_traceback_runs(dirs, W, L, side, gap_end_i(best), je, q, qq, base, base + L, base + 2 * (size_t)L, base + 3 * (size_t)L, base + 4 * (size_t)L, nullptr);
    } else {
        if (live && d == 0 && best != 0) gaps = gap_traceback(dirs, W, L, side, gap_end_i(best), je, q, qq, base, base + L, base + 2 * (size_t)L, nullptr);
    }
    // the positions the path does not consume: columns je + 1 .. L
    if (live) {
        const int t0 = side ? 0 : je, t1 = side ? L - je : L;                               // [t0, t1)
        for (int t = t0 + d; t < t1; t += 32) { base[t] = 0; base[L + t] = 0; base[2 * (size_t)L + t] = GAP_NOT_COVERED; }
    }
    const int n_gapped = __popcll(__ballot(gaps > 0));
    if (lane == 0 && n_gapped) atomicAdd(&ctr->gapped_sides, (unsigned long long)n_gapped);
}

// ---- the count ------------------------------------------------------------------------------------------------------------------------------------------
// (the classes GAP_CLASS_DEL, GAP_CLASS_NONE and GAP_CLASS_DISC are gapped_align.h's)
// where the count finds the projections: proj_off[2 (g - g_first) + side] into proj, or -1
struct GapProj { uint32_t g_first; const int64_t* __restrict__ off; const uint8_t* __restrict__ bytes; };

// one side of group g at template position t (t < L, or t == L for a lane beyond the template: its index is clamped and its value discarded).  po is the
// wavefront's: a side with a projection (po >= 0) or without.  idx: the index of t in the consensus read (t itself, or L - 1 - t on the ligation side).
__device__ static inline void gap_observe(const uint8_t* __restrict__ proj, int64_t po, const uint8_t* __restrict__ seq, const uint8_t* __restrict__ qual, int64_t o, int n, int idx,
                                          int t, int L, bool lig, int min_q, uint32_t& cls, bool& covers, uint32_t& ins_len)
{
    if (po >= 0) {
        const uint8_t* __restrict__ P = proj + po;
        const int tt = min(t, L - 1);
        const uint32_t b = P[tt], qv = P[L + tt], il = P[2 * (size_t)L + tt];
        const uint32_t c = reads_base_code(b);
        cls = b == '-' ? GAP_CLASS_DEL : c < 4u && (int)qv - 33 >= min_q ? c : GAP_CLASS_NONE;
        covers = il != GAP_NOT_COVERED; ins_len = il;
    } else {
        const bool present = idx >= 0 && idx < n;
        const int64_t at = o + max(min(idx, n - 1), 0);                                     // clamped: see the head of kernels_pileup.hip
        const uint32_t b = seq[at], qv = qual[at];
        uint32_t c = reads_base_code(b);
        if (lig) c = c < 4u ? 3u - c : 4u;
        cls = present && c < 4u && (int)qv - 33 >= min_q ? c : GAP_CLASS_NONE;
        covers = present && (lig ? idx >= 1 : (t + 1 < n && t + 1 < L));                   // the ungapped path consumes t and t + 1
        ins_len = 0u;
    }
}

struct GapPile {
    static constexpr int COLUMNS = GAPPED_COLUMNS;
    using Counters = GappedCounters;
    static constexpr ColumnSum<GappedCounters> SUMS[5] = {{0, 4, &GappedCounters::bases}, {4, 5, &GappedCounters::discordant}, {5, 6, &GappedCounters::deletions},
                                                          {6, 7, &GappedCounters::insertions}, {7, 8, &GappedCounters::ins_discordant}};
    int n[COLUMNS] = {0, 0, 0, 0, 0, 0, 0, 0};                                              // A, C, G, T, discordant, del, ins, ins_discordant
    // the vote of one molecule at one position and at the anchor behind it: ce / cl - each side's usable observation (0..3, del, none), ve / vl -
    // the side covers the anchor (t, t + 1), ne / nl - its insertion length there
    __device__ inline void add(bool ok, uint32_t ce, uint32_t cl, bool ve, bool vl, uint32_t ne, uint32_t nl)
    {
        const bool ue = ok && ce < GAP_CLASS_NONE, ul = ok && cl < GAP_CLASS_NONE;
        const uint32_t col = ue && ul && ce != cl ? GAP_CLASS_DISC : ue ? ce : ul ? cl : GAP_CLASS_NONE;
        n[0] += col == 0u; n[1] += col == 1u; n[2] += col == 2u; n[3] += col == 3u; n[5] += col == GAP_CLASS_DEL; n[4] += col == GAP_CLASS_DISC;
        const bool xe = ok && ve, xl = ok && vl;
        n[6] += xe && xl ? (ne == nl && ne > 0u) : xe ? ne > 0u : xl ? nl > 0u : false;
        n[7] += xe && xl && ne != nl;
    }
    __device__ static inline void groups(GapPile& S, const ConsensusView& I, const PileRow& R, uint32_t g0, uint32_t g1, uint32_t stride, int t, int L, const GapProj& P)
    {
        for (uint32_t g = g0; g < g1; g += stride) {
            const int64_t eo = I.ext_off[g], lo = I.lig_off[g];
            const int el = (int)(I.ext_off[g + 1] - eo), ll = (int)(I.lig_off[g + 1] - lo);
            const int64_t pe = P.off[2 * (size_t)(g - P.g_first)], pl = P.off[2 * (size_t)(g - P.g_first) + 1];
            uint32_t ce, cl, ne, nl;
            bool ve, vl;
            gap_observe(P.bytes, pe, I.ext_seq, I.ext_qual, eo, el, t, t, L, false, R.min_quality, ce, ve, ne);
            gap_observe(P.bytes, pl, I.lig_seq, I.lig_qual, lo, ll, L - 1 - t, t, L, true, R.min_quality, cl, vl, nl);
            S.add(I.family[g] >= R.min_family, ce, cl, ve, vl, ne, nl);
        }
    }
    __device__ inline void store(int32_t* __restrict__ o) const
    {
        int4* __restrict__ v = reinterpret_cast<int4*>(o);                                  // (32 bytes per position, the table 256-byte aligned)
        v[0] = make_int4(n[0], n[1], n[2], n[3]);
        v[1] = make_int4(n[4], n[5], n[6], n[7]);
    }
};

// ---- insertion alleles ------------------------------------------------------------------------------------------------------------------------
// where the events go: keys[0, cap), the slots reserved through ctr->events
struct InsEmit { uint64_t* __restrict__ keys; unsigned long long cap; InsCounters* __restrict__ ctr; };

// one side at the anchor (t, t + 1): does it cover it, with which insertion length, and (a side with a run) where the run starts in its read.  A side without a
// projection has the ungapped path: gap_observe's cover rule, length 0.
__device__ static inline void ins_side(const uint8_t* __restrict__ proj, int64_t po, int n, int idx, int t, int L, bool lig, bool& covers, uint32_t& len, int& at)
{
    at = 0;
    if (po >= 0) {
        const uint8_t* __restrict__ P = proj + po;
        const int tt = min(t, L - 1);
        const uint32_t il = P[2 * (size_t)L + tt];
        covers = il != GAP_NOT_COVERED; len = il;
        if (covers && il > 0u) at = (int)P[3 * (size_t)L + tt] | ((int)P[4 * (size_t)L + tt] << 8);
    } else {
        const bool present = idx >= 0 && idx < n;
        covers = present && (lig ? idx >= 1 : (t + 1 < n && t + 1 < L));
        len = 0u;
    }
}

struct InsPile {
    static constexpr int COLUMNS = INSERTION_COLUMNS;
    using Counters = InsCounters;
    static constexpr ColumnSum<InsCounters> SUMS[4] = {{0, 1, &InsCounters::span}, {1, 2, &InsCounters::insertions}, {2, 3, &InsCounters::ins_discordant},
                                                       {3, 4, &InsCounters::ambiguous}};
    int n[COLUMNS] = {0, 0, 0, 0};                                                          // span, ins, ins_discordant, ambiguous
    __device__ static inline void groups(InsPile& S, const ConsensusView& I, const PileRow& R, uint32_t g0, uint32_t g1, uint32_t stride, int t, int L, const GapProj& P,
                                         const InsEmit& E)
    {
        const int lane = threadIdx.x & 63;
        for (uint32_t g = g0; g < g1; g += stride) {                                        // (wave-uniform: every lane of the wavefront is here)
            const int64_t eo = I.ext_off[g], lo = I.lig_off[g];
            const int el = (int)(I.ext_off[g + 1] - eo), ll = (int)(I.lig_off[g + 1] - lo);
            const int64_t pe = P.off[2 * (size_t)(g - P.g_first)], pl = P.off[2 * (size_t)(g - P.g_first) + 1];
            const bool ok = I.family[g] >= R.min_family;
            bool ve, vl;
            uint32_t ne, nl;
            int ae, al;
            ins_side(P.bytes, pe, el, t, t, L, false, ve, ne, ae);
            ins_side(P.bytes, pl, ll, L - 1 - t, t, L, true, vl, nl, al);
            const bool xe = ok && ve, xl = ok && vl;
            const bool disc = xe && xl && ne != nl, spans = (xe || xl) && !disc;
            const int l = (int)(xe ? ne : nl);                                              // the agreed length of a molecule that spans
            const bool event = spans && l > 0 && t < L - 1;                                 // (a lane clamped beyond the template emits nothing)
            S.n[0] += spans; S.n[1] += spans && l > 0; S.n[2] += disc;
            const unsigned long long events = __ballot(event);
            if (events == 0ull) continue;                                                   // (the wavefront's)
            uint32_t bases = 0u;
            bool amb = l > GAP_ALLELE_MAX_LEN;
            if (event && !amb) {
                for (int j = 0; j < l; j++) {
                    int be = 0, bl = 0;
                    bool ue = false, ul = false;
                    if (xe) {                                                               // (el >= 1: the side has a projection)
                        const int64_t at = eo + max(min(gap_run_index(GAP_EXT, ae, l, j), el - 1), 0);
                        be = I.ext_seq[at];
                        ue = gap_base_code(be) < 4 && (int)I.ext_qual[at] - 33 >= R.min_quality;
                    }
                    if (xl) {
                        const int64_t at = lo + max(min(gap_run_index(GAP_LIG, al, l, j), ll - 1), 0);
                        bl = gap_complement(I.lig_seq[at]);
                        ul = gap_base_code(bl) < 4 && (int)I.lig_qual[at] - 33 >= R.min_quality;
                    }
                    const int c = gap_allele_base(be, ue, bl, ul);
                    amb = amb || c > 3;
                    bases = (bases << 2) | (uint32_t)(c & 3);
                }
            }
            S.n[3] += event && amb;
            unsigned long long first = 0;
            if (lane == 0) first = atomicAdd(&E.ctr->events, (unsigned long long)__popcll(events));
            first = __shfl(first, 0);
            if (event) {
                const unsigned long long slot = first + (unsigned long long)__popcll(events & ((1ull << lane) - 1ull));
                const uint32_t p = (uint32_t)(I.keys[g] >> 32) - R.cell0;
                if (slot < E.cap) E.keys[slot] = gap_allele_key(R.pos_off[p] + t, l, amb, bases);
            }
        }
    }
    __device__ inline void store(int32_t* __restrict__ o) const { *reinterpret_cast<int4*>(o) = make_int4(n[0], n[1], n[2], n[3]); }      // (16 bytes per anchor, the table 256-byte aligned)
};

// a lane per run of the sorted keys
__global__ __launch_bounds__(256) void k_ins_records(const uint64_t* __restrict__ run_keys, const int32_t* __restrict__ run_counts, const unsigned long long* __restrict__ n_runs,
                                                     int64_t cap, mipgen_insertion_record* __restrict__ records)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || (unsigned long long)i >= *n_runs) return;
    const uint64_t key = run_keys[i];
    mipgen_insertion_record r;
    r.pos = gap_allele_pos(key); r.length = gap_allele_length(key); r.count = run_counts[i]; r.bases = gap_allele_bases(key); r.ambiguous = gap_allele_ambiguous(key) ? 1 : 0;
    records[i] = r;
}

// ---- deletion alleles -------------------------------------------------------------------------------------------------------------------------
// where the events go: keys[0, cap), the slots reserved through ctr->events
struct DelEmit { uint64_t* __restrict__ keys; unsigned long long cap; DelCounters* __restrict__ ctr; };

// one group's reads and projections, as the observations of a position need them
struct DelMolecule { int64_t eo, lo, pe, pl; int el, ll; bool ok; };

// The class of the molecule at template position t (t <= L; L itself for a clamped lane, whose value is discarded) and whether a run of deletions that borders on
// t is ragged there.  A molecule that is not used has no class.
__device__ static inline uint32_t del_class(const ConsensusView& I, const PileRow& R, const GapProj& P, const DelMolecule& m, int t, int L, uint32_t& ce, uint32_t& cl)
{
    uint32_t ne, nl;
    bool ve, vl;
    gap_observe(P.bytes, m.pe, I.ext_seq, I.ext_qual, m.eo, m.el, t, t, L, false, R.min_quality, ce, ve, ne);
    gap_observe(P.bytes, m.pl, I.lig_seq, I.lig_qual, m.lo, m.ll, L - 1 - t, t, L, true, R.min_quality, cl, vl, nl);
    if (!m.ok) ce = cl = GAP_CLASS_NONE;
    return gap_molecule_class(ce, cl);
}

// A third policy of the count frame, k_del_wave / k_del_wg: four counters per position (depth, starts, ragged, del; one 16-byte store) and THE EVENTS as a side
// effect.  A lane whose molecule votes del while the lane below does not is the start of a maximal run; its length is the consecutive set bits of the ballot of the
// del lanes from its own position and, only where that run reaches lane 63 and the template goes on, the positions of the rounds behind observed directly.  The
// next round's wavefront sees that tail as "not a start" by the same rule.  Everything the wavefront decides on - the ballots, lane 0's neighbour, the
// continuation - is wave-uniform, so no lane waits for another.
struct DelPile {
    static constexpr int COLUMNS = DELETION_COLUMNS;
    using Counters = DelCounters;
    static constexpr ColumnSum<DelCounters> SUMS[4] = {{0, 1, &DelCounters::depth}, {1, 2, &DelCounters::starts}, {2, 3, &DelCounters::ragged}, {3, 4, &DelCounters::deleted}};
    int n[COLUMNS] = {0, 0, 0, 0};                                                          // depth, starts, ragged, del
    __device__ static inline void groups(DelPile& S, const ConsensusView& I, const PileRow& R, uint32_t g0, uint32_t g1, uint32_t stride, int t, int L, const GapProj& P,
                                         const DelEmit& E)
    {
        const int lane = threadIdx.x & 63;
        const int t0 = __builtin_amdgcn_readfirstlane(t);                                   // the round's first position (lane 0 is never clamped)
        const bool live = t < L;
        for (uint32_t g = g0; g < g1; g += stride) {                                        // (wave-uniform: every lane of the wavefront is here)
            DelMolecule m;
            m.eo = I.ext_off[g]; m.lo = I.lig_off[g];
            m.el = (int)(I.ext_off[g + 1] - m.eo); m.ll = (int)(I.lig_off[g + 1] - m.lo);
            m.pe = P.off[2 * (size_t)(g - P.g_first)]; m.pl = P.off[2 * (size_t)(g - P.g_first) + 1];
            m.ok = I.family[g] >= R.min_family;
            uint32_t ce, cl;
            const uint32_t c = del_class(I, R, P, m, t, L, ce, cl);
            const bool del = live && c == GAP_CLASS_DEL;                                    // (a lane clamped at or beyond the template's end is no part of any run)
            const bool rag = live && gap_ragged_flank(ce, cl);
            S.n[0] += c < GAP_CLASS_NONE; S.n[3] += c == GAP_CLASS_DEL;
            const unsigned long long dels = __ballot(del);
            if (dels == 0ull) continue;                                                     // (the wavefront's: the common case ends here)
            // the class of the position below: the lane below, or for lane 0 of a later round one more observation; nothing at t = 0
            bool below_del = __shfl_up((int)del, 1) != 0, below_rag = __shfl_up((int)rag, 1) != 0;
            if ((dels & 1ull) && t0 > 0) {                                                  // (wave-uniform)
                uint32_t be, bl;
                const uint32_t b = del_class(I, R, P, m, t0 - 1, L, be, bl);
                if (lane == 0) { below_del = b == GAP_CLASS_DEL; below_rag = gap_ragged_flank(be, bl); }
            } else if (lane == 0) {
                below_del = false; below_rag = false;
            }
            const bool start = del && !below_del;
            const unsigned long long starts = __ballot(start);
            if (starts == 0ull) continue;                                                   // (the wavefront's: every del lane continues a run of the round before)
            const unsigned long long rags = __ballot(rag);
            int l = start ? gap_mask_run(dels, lane) : 0;
            const int after = lane + l;                                                     // the lane behind the run, 64 if the run reaches the round's end
            bool above_rag = start && after < 64 && ((rags >> (after & 63)) & 1ull);
            // the one run that reaches lane 63, where the template goes on: wave-uniform direct observations behind the round
            const bool reaches = start && after == 64;
            if (__ballot(reaches) != 0ull && t0 + 64 < L) {
                int more = 0;
                bool end_rag = false;
                for (int tt = t0 + 64; tt < L; tt++) {
                    uint32_t xe, xl;
                    if (del_class(I, R, P, m, tt, L, xe, xl) != GAP_CLASS_DEL) { end_rag = gap_ragged_flank(xe, xl); break; }
                    more++;
                }
                if (reaches) { l += more; above_rag = end_rag; }
            }
            const bool ragged = start && (below_rag || above_rag);
            S.n[1] += start; S.n[2] += ragged;
            const long long sum = wave_sum_i64((long long)l);
            unsigned long long first = 0;
            if (lane == 0) {
                first = atomicAdd(&E.ctr->events, (unsigned long long)__popcll(starts));
                atomicAdd(&E.ctr->length_sum, (unsigned long long)sum);
            }
            first = __shfl(first, 0);
            if (start) {
                const unsigned long long slot = first + (unsigned long long)__popcll(starts & ((1ull << lane) - 1ull));
                const uint32_t p = (uint32_t)(I.keys[g] >> 32) - R.cell0;
                if (slot < E.cap) E.keys[slot] = gap_deletion_key(R.pos_off[p] + t, l, ragged);
            }
        }
    }
    __device__ inline void store(int32_t* __restrict__ o) const { *reinterpret_cast<int4*>(o) = make_int4(n[0], n[1], n[2], n[3]); }      // (16 bytes per position, the table 256-byte aligned)
};

// a lane per run of the sorted keys: the record's depth is the sites table's at the run's first base
__global__ __launch_bounds__(256) void k_del_records(const uint64_t* __restrict__ run_keys, const int32_t* __restrict__ run_counts, const unsigned long long* __restrict__ n_runs,
                                                     int64_t cap, const int32_t* __restrict__ sites, int64_t n_pos, mipgen_deletion_record* __restrict__ records)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || (unsigned long long)i >= *n_runs) return;
    const uint64_t key = run_keys[i];
    mipgen_deletion_record r;
    r.pos = gap_deletion_pos(key); r.length = gap_deletion_length(key); r.count = run_counts[i]; r.ragged = gap_deletion_ragged(key) ? 1 : 0;
    r.depth = r.pos < n_pos ? sites[r.pos * DELETION_COLUMNS] : 0;                          // (a key is a position of the table: the guard costs nothing)
    records[i] = r;
}

extern "C" {

size_t mipgen_gap_align_lds_bytes(int max_len, int W) { return (size_t)2 * (size_t)(max_len + W) * 2 * sizeof(uint32_t); }

// the sides of the row's groups [g_first, g_first + n_row_groups) that need the dynamic program: list[0, ctr->n_sides), proj_off[2 n_row_groups] (-1: no
// projection), ctr->proj_bytes; ctr is zero on entry
hipError_t mipgen_launch_gap_list(hipStream_t st, const ConsensusView& C, const PileRow& R, const uint8_t* mol_seq, uint32_t g_first, int64_t n_row_groups, int max_indel,
                                  int planes, uint8_t* need, uint32_t* list, int64_t* proj_off, GappedCounters* ctr)
{
    if (n_row_groups < 1 || n_row_groups > 0x3fffffff || max_indel < 1 || max_indel > GAP_MAX_INDEL || (planes != 3 && planes != 5)) return hipErrorInvalidValue;
    const GapIn I{C, R, mol_seq, g_first, max_indel};
    hipLaunchKernelGGL(k_gap_screen, dim3((unsigned)((n_row_groups + 3) / 4)), dim3(256), 0, st, I, n_row_groups, need);
    const dim3 grid((unsigned)((2 * n_row_groups + 255) / 256));
    if (planes == 5) hipLaunchKernelGGL(k_gap_list<5>, grid, dim3(256), 0, st, I, 2 * n_row_groups, need, list, proj_off, ctr);
    else hipLaunchKernelGGL(k_gap_list<3>, grid, dim3(256), 0, st, I, 2 * n_row_groups, need, list, proj_off, ctr);
    return hipGetLastError();
}

// the alignment of the n_sides listed sides into proj (planes: as the list was made), then counts[R.n_pos][8] written whole and summed into ctr
hipError_t mipgen_launch_gapped(hipStream_t st, const ConsensusView& C, const PileRow& R, int64_t n_units, const uint8_t* mol_seq, uint32_t g_first, int max_indel, int max_len,
                                int planes,
                                const uint32_t* list, int64_t n_sides, const int64_t* proj_off, uint8_t* proj, int32_t* counts, GappedCounters* ctr)
{
    if (R.n_small < 0 || R.n_big < 0 || R.n_small + R.n_big != n_units || n_units > 0x7fffffff || R.n_pos < 1 || n_sides < 0 || n_sides > 0x7fffffff || max_indel < 1 ||
        max_indel > GAP_MAX_INDEL || max_len < 1 || max_len > GAP_MAX_MOL || (planes != 3 && planes != 5))
        return hipErrorInvalidValue;
    const GapIn I{C, R, mol_seq, g_first, max_indel};
    const dim3 grid((unsigned)((n_sides + 1) / 2));
    const size_t lds = mipgen_gap_align_lds_bytes(max_len, max_indel);
    if (n_sides > 0 && planes == 5) hipLaunchKernelGGL(k_gap_align<true>, grid, dim3(64), lds, st, list, n_sides, proj_off, proj, I, max_len + max_indel, ctr);
    else if (n_sides > 0) hipLaunchKernelGGL(k_gap_align<false>, grid, dim3(64), lds, st, list, n_sides, proj_off, proj, I, max_len + max_indel, ctr);
    return pile_launch<GapPile>(st, C, R, counts, ctr, GapProj{g_first, proj_off, proj});
}

// anchors[R.n_pos][4] written whole and summed into ctr, the events of the row into keys[0, cap) in no defined order, ctr->events their number (ctr zero on entry);
// proj_off / proj: the five-plane projections of the row
hipError_t mipgen_launch_insertions(hipStream_t st, const ConsensusView& C, const PileRow& R, int64_t n_units, uint32_t g_first, const int64_t* proj_off, const uint8_t* proj,
                                    int32_t* anchors, uint64_t* keys, int64_t cap, InsCounters* ctr)
{
    if (R.n_small < 0 || R.n_big < 0 || R.n_small + R.n_big != n_units || n_units > 0x7fffffff || R.n_pos < 1 || R.n_pos > MIPGEN_CALL_MAX_POSITIONS || cap < 0 || cap > 0x7fffffff)
        return hipErrorInvalidValue;
    return pile_launch<InsPile>(st, C, R, anchors, ctr, GapProj{g_first, proj_off, proj}, InsEmit{keys, (unsigned long long)cap, ctr});
}

// the first min(*n_runs, cap) runs decoded into records
hipError_t mipgen_launch_insertion_records(hipStream_t st, const uint64_t* run_keys, const int32_t* run_counts, const unsigned long long* n_runs, int64_t cap,
                                           mipgen_insertion_record* records)
{
    if (cap < 1 || cap > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ins_records, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, st, run_keys, run_counts, n_runs, cap, records);
    return hipGetLastError();
}

// sites[R.n_pos][4] written whole and summed into ctr, the deletion events of the row into keys[0, cap) in no defined order, ctr->events their number and
// ctr->length_sum the sum of their lengths (ctr zero on entry); proj_off / proj: the three-plane projections of the row
hipError_t mipgen_launch_deletions(hipStream_t st, const ConsensusView& C, const PileRow& R, int64_t n_units, uint32_t g_first, const int64_t* proj_off, const uint8_t* proj,
                                   int32_t* sites, uint64_t* keys, int64_t cap, DelCounters* ctr)
{
    if (R.n_small < 0 || R.n_big < 0 || R.n_small + R.n_big != n_units || n_units > 0x7fffffff || R.n_pos < 1 || R.n_pos > MIPGEN_CALL_MAX_POSITIONS || cap < 0 || cap > 0x7fffffff)
        return hipErrorInvalidValue;
    return pile_launch<DelPile>(st, C, R, sites, ctr, GapProj{g_first, proj_off, proj}, DelEmit{keys, (unsigned long long)cap, ctr});
}

// the first min(*n_runs, cap) runs decoded into records, their depth read from sites[n_pos][4]
hipError_t mipgen_launch_deletion_records(hipStream_t st, const uint64_t* run_keys, const int32_t* run_counts, const unsigned long long* n_runs, int64_t cap, const int32_t* sites,
                                          int64_t n_pos, mipgen_deletion_record* records)
{
    if (cap < 1 || cap > 0x7fffffff || n_pos < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_del_records, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, st, run_keys, run_counts, n_runs, cap, sites, n_pos, records);
    return hipGetLastError();
}

}
