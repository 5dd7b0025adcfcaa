// kernels_pileup.hip — allele counts per template position of every probe from the consensus reads the handle holds.
//
//  k_pileup_cells      a lane per probe p of the requested row (and one more): start[p] = the first group whose cell is >= row * n + p, a lower bound in the
//                      ascending group keys.  The groups of cell p are [start[p], start[p + 1]): a contiguous run, because the keys are sorted by (row, probe, tag).
//  k_pileup_partition  a lane per probe: its rounds of 64 template positions, as (probe, round) units, go to the front of units[] (a cell of at most PILEUP_WG_CELL
//                      groups; an empty cell too: its zeros are written like any other count) or to its back; slots by a wavefront scan + one atomic per wavefront
//                      and class, as k_consensus_partition reserves its.
//  k_pileup_used       a lane per group: the row's groups of at least min_family pairs, counted by ballot.
//  Pile                the vote of the ungapped table, plugged into the count frame of pileup_frame.h: k_pileup_wave = k_pile_wave<Pile>, k_pileup_wg = k_pile_wg<Pile>,
//                      k_pileup_sum = k_pile_sum<Pile>.  A loop over the cell's groups: per group the two offsets of each side and the family come through scalar
//                      loads; each lane then loads four bytes - extension base and quality at t, ligation base and quality at len - 1 - t - so every load of the
//                      wavefront is 64 consecutive bytes of one consensus read (the ligation run descending).  Five 32-bit counters in registers, the group loop
//                      unrolled by four (16 byte loads in flight per lane), five dword stores per lane and round - the 20 bytes of its position.
//                      Out-of-range lanes: the index is CLAMPED and the value discarded - a lane at or beyond a side's length reads that side's last byte, a
//                      lane beyond len_p reads ligation byte 0, a side of length 0 reads index 0, which lies inside the allocation because consensus_finish
//                      reserves one byte more than the reads of a side.  No load is predicated, so the unrolled loop keeps its loads in flight.
//                      32-bit counters: a counter is at most the groups of a cell, a session holds at most 2^31 - 1 pairs and a group has at least one.
//                      Column sums: bases (columns 0..3) and discordant (column 4).
// Bound: the consensus bases and qualities of both sides once + 36 bytes of offsets and family per group and round + 20 bytes written per template position.
#include "pileup_frame.h"

__global__ __launch_bounds__(256) void k_pileup_cells(const uint64_t* __restrict__ keys, int64_t n_groups, uint32_t cell0, int32_t n, uint32_t* __restrict__ start)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n) return;
    const uint64_t want = ((uint64_t)cell0 + (uint64_t)p) << 32;                            // (at most 2^31 cells: the shift keeps every bit)
    int64_t lo = 0, hi = n_groups;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    start[p] = (uint32_t)lo;
}

// units[0, n_small): the rounds of the cells of at most PILEUP_WG_CELL groups; units[n_units - n_big, n_units): of the others.  n_units = the rounds of all probes
// (the host's sum, below 2^31); neither list is in probe order: a unit writes to its own positions whoever counts it.
__global__ __launch_bounds__(256) void k_pileup_partition(const uint32_t* __restrict__ start, const int32_t* __restrict__ mol_len, int32_t n, int64_t n_units,
                                                          uint2* __restrict__ units, PileupCounters* __restrict__ ctr)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = p < n;
    const int lane = threadIdx.x & 63;
    const uint32_t rounds = active ? ((uint32_t)mol_len[p] + 63u) >> 6 : 0u;
    const bool big = active && start[p + 1] - start[p] > (uint32_t)PILEUP_WG_CELL;
    const uint32_t rs = big ? 0u : rounds, rb = big ? rounds : 0u;
    const uint32_t is = wave_inclusive_sum_u32(rs, lane), ib = wave_inclusive_sum_u32(rb, lane);
    const uint32_t ts = __shfl(is, 63), tb = __shfl(ib, 63);
    unsigned long long bs = 0, bb = 0;
    if (lane == 0) {
        if (ts) bs = atomicAdd(&ctr->n_small, (unsigned long long)ts);
        if (tb) bb = atomicAdd(&ctr->n_big, (unsigned long long)tb);
    }
    bs = __shfl(bs, 0); bb = __shfl(bb, 0);
    for (uint32_t r = 0; r < rs; r++) units[bs + (is - rs) + r] = make_uint2((uint32_t)p, r);
    for (uint32_t r = 0; r < rb; r++) units[(unsigned long long)n_units - 1ull - (bb + (ib - rb) + r)] = make_uint2((uint32_t)p, r);
}

__global__ __launch_bounds__(256) void k_pileup_used(const uint32_t* __restrict__ start, int32_t n, const int32_t* __restrict__ family, int64_t n_groups, int min_family,
                                                     PileupCounters* __restrict__ ctr)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool used = g < n_groups && g >= (int64_t)start[0] && g < (int64_t)start[n] && family[g] >= min_family;
    const int c = __popcll(__ballot(used));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&ctr->used, (unsigned long long)c);
}

// ---- the count ---------------------------------------------------------------------------------------------------------------------------------------
struct Pile {
    static constexpr int COLUMNS = PILEUP_COLUMNS;
    using Counters = PileupCounters;
    static constexpr ColumnSum<PileupCounters> SUMS[2] = {{0, 4, &PileupCounters::bases}, {4, 5, &PileupCounters::discordant}};
    int n[COLUMNS] = {0, 0, 0, 0, 0};                                                       // A, C, G, T, discordant
    // the vote of one molecule at one position: pe / pl - the side covers the position; the ligation base is complemented into M's orientation
    __device__ inline void add(bool ok, bool pe, bool pl, uint32_t eb, uint32_t eq, uint32_t lb, uint32_t lq, int min_q)
    {
        const uint32_t ce = reads_base_code(eb), cr = reads_base_code(lb);
        const uint32_t cl = cr < 4u ? 3u - cr : 4u;                                         // A <-> T, C <-> G; anything else stays unusable
        const bool ue = ok && pe && ce < 4u && (int)eq - 33 >= min_q;
        const bool ul = ok && pl && cl < 4u && (int)lq - 33 >= min_q;
        const uint32_t col = ue && ul && ce != cl ? 4u : ue ? ce : ul ? cl : 5u;            // both usable and different: discordant, and no base
        n[0] += col == 0u; n[1] += col == 1u; n[2] += col == 2u; n[3] += col == 3u; n[4] += col == 4u;
    }
    // groups g0, g0 + stride, ... below g1 into S, for the lane whose extension index is t and whose ligation index is j = len - 1 - t (j < 0: a lane beyond
    // len_p).  g0, g1 and stride are the wavefront's: the five words of a group come through scalar loads.
    __device__ static inline void groups(Pile& S, const ConsensusView& I, const PileRow& R, uint32_t g0, uint32_t g1, uint32_t stride, int t, int len)
    {
        const int j = len - 1 - t;
        uint32_t g = g0;
        for (; g + 3u * stride < g1; g += 4u * stride) {                                    // (g1 < 2^31: no wrap)
            uint32_t eb[4], eq[4], lb[4], lq[4];
            bool ok[4], pe[4], pl[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t gu = g + (uint32_t)u * stride;
                const int64_t eo = I.ext_off[gu], lo = I.lig_off[gu];
                const int el = (int)(I.ext_off[gu + 1] - eo), ll = (int)(I.lig_off[gu + 1] - lo);
                ok[u] = I.family[gu] >= R.min_family;
                pe[u] = t < el; pl[u] = j >= 0 && j < ll;
                const int64_t ie = eo + max(min(t, el - 1), 0), il = lo + max(min(j, ll - 1), 0);  // clamped: see the head of the file
                eb[u] = I.ext_seq[ie]; eq[u] = I.ext_qual[ie]; lb[u] = I.lig_seq[il]; lq[u] = I.lig_qual[il];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) S.add(ok[u], pe[u], pl[u], eb[u], eq[u], lb[u], lq[u], R.min_quality);
        }
        for (; g < g1; g += stride) {
            const int64_t eo = I.ext_off[g], lo = I.lig_off[g];
            const int el = (int)(I.ext_off[g + 1] - eo), ll = (int)(I.lig_off[g + 1] - lo);
            const int64_t ie = eo + max(min(t, el - 1), 0), il = lo + max(min(j, ll - 1), 0);
            S.add(I.family[g] >= R.min_family, t < el, j >= 0 && j < ll, I.ext_seq[ie], I.ext_qual[ie], I.lig_seq[il], I.lig_qual[il], R.min_quality);
        }
    }
    __device__ inline void store(int32_t* __restrict__ o) const { o[0] = n[0]; o[1] = n[1]; o[2] = n[2]; o[3] = n[3]; o[4] = n[4]; }
};

extern "C" {

// start[0, R.n] of the row whose first cell is R.cell0, the (cell, round) units of its R.n probes (n_units: the rounds of all probes) and ctr->used; ctr is zero on entry
hipError_t mipgen_launch_pileup_prepare(hipStream_t st, const ConsensusView& C, const PileRow& R, int64_t n_units, uint32_t* start, uint2* units, PileupCounters* ctr)
{
    const int32_t n = R.n;
    if (n < 1 || C.n_groups < 1 || C.n_groups > 0x7fffffff || n_units < 1 || n_units > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pileup_cells, dim3((unsigned)(((int64_t)n + 1 + 255) / 256)), dim3(256), 0, st, C.keys, C.n_groups, R.cell0, n, start);
    hipLaunchKernelGGL(k_pileup_partition, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, st, start, R.mol_len, n, n_units, units, ctr);
    hipLaunchKernelGGL(k_pileup_used, dim3((unsigned)((C.n_groups + 255) / 256)), dim3(256), 0, st, start, n, C.family, C.n_groups, R.min_family, ctr);
    return hipGetLastError();
}

// R.units: k_pileup_partition's (the n_big workgroup units at its end); counts[R.n_pos][5] is written whole, then summed into ctr->bases / ctr->discordant
hipError_t mipgen_launch_pileup(hipStream_t st, const ConsensusView& C, const PileRow& R, int64_t n_units, int32_t* counts, PileupCounters* ctr)
{
    if (R.n_small < 0 || R.n_big < 0 || R.n_small + R.n_big != n_units || n_units > 0x7fffffff || R.n_pos < 1) return hipErrorInvalidValue;
    return pile_launch<Pile>(st, C, R, counts, ctr);
}

}
