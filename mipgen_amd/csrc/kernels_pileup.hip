// kernels_pileup.hip — allele counts per template position of every probe from the consensus reads the handle holds.
//
//  k_pileup_cells      a lane per probe p of the requested row (and one more): start[p] = the first group whose cell is >= row * n + p, a lower bound in the
//                      ascending group keys.  The groups of cell p are [start[p], start[p + 1]): a contiguous run, because the keys are sorted by (row, probe, tag).
//  k_pileup_partition  a lane per probe: its rounds of 64 template positions, as (probe, round) units, go to the front of units[] (a cell of at most PILEUP_WG_CELL
//                      groups; an empty cell too: its zeros are written like any other count) or to its back; slots by a wavefront scan + one atomic per wavefront
//                      and class, as k_consensus_partition reserves its.
//  k_pileup_used       a lane per group: the row's groups of at least min_family pairs, counted by ballot.
//  k_pileup_wave       a WAVEFRONT per (cell, round) unit, LANES OVER TEMPLATE POSITIONS, a loop over the cell's groups: lane l owns t = 64 r + l.  Per group the
//  k_pileup_wg         two offsets of each side and the family come through scalar loads; each lane then loads four bytes - extension base and quality at t,
//                      ligation base and quality at len - 1 - t - so every load of the wavefront is 64 consecutive bytes of one consensus read (the ligation run
//                      descending).  Five 32-bit counters in registers, the group loop unrolled by four (16 byte loads in flight per lane), five dword stores per
//                      lane and round - the 20 bytes of its position - and no atomic.  _wg: a 256-thread workgroup per unit of a cell above PILEUP_WG_CELL; its
//                      four wavefronts stride over the groups and add through LDS.
//                      Out-of-range lanes: the index is CLAMPED and the value discarded - a lane at or beyond a side's length reads that side's last byte, a
//                      lane beyond len_p reads ligation byte 0, a side of length 0 reads index 0, which lies inside the allocation because consensus_finish
//                      reserves one byte more than the reads of a side.  No load is predicated, so the unrolled loop keeps its loads in flight.
//                      32-bit counters: a counter is at most the groups of a cell, a session holds at most 2^31 - 1 pairs and a group has at least one.
//  k_pileup_sum        the sums of the columns of the finished table (bases, discordant): a grid-stride pass, one atomic pair per wavefront.
// Bound: the consensus bases and qualities of both sides once + 36 bytes of offsets and family per group and round + 20 bytes written per template position.
#include "kernels.h"

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

__device__ static inline uint32_t wave_inclusive_sum(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
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
    const uint32_t is = wave_inclusive_sum(rs, lane), ib = wave_inclusive_sum(rb, lane);
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
struct PileupIn {
    const int32_t* __restrict__ family;
    const int64_t* __restrict__ ext_off;
    const int64_t* __restrict__ lig_off;
    const uint8_t* __restrict__ ext_seq;
    const uint8_t* __restrict__ ext_qual;
    const uint8_t* __restrict__ lig_seq;
    const uint8_t* __restrict__ lig_qual;
    int min_family, min_quality;
};

struct Pile {
    int a = 0, c = 0, g = 0, t = 0, d = 0;
    // the vote of one molecule at one position: pe / pl - the side covers the position; the ligation base is complemented into M's orientation
    __device__ inline void add(bool ok, bool pe, bool pl, uint32_t eb, uint32_t eq, uint32_t lb, uint32_t lq, int min_q)
    {
        const uint32_t ce = reads_base_code(eb), cr = reads_base_code(lb);
        const uint32_t cl = cr < 4u ? 3u - cr : 4u;                                         // A <-> T, C <-> G; anything else stays unusable
        const bool ue = ok && pe && ce < 4u && (int)eq - 33 >= min_q;
        const bool ul = ok && pl && cl < 4u && (int)lq - 33 >= min_q;
        const uint32_t col = ue && ul && ce != cl ? 4u : ue ? ce : ul ? cl : 5u;            // both usable and different: discordant, and no base
        a += col == 0u; c += col == 1u; g += col == 2u; t += col == 3u; d += col == 4u;
    }
};

// groups g0, g0 + stride, ... below g1 into S, for the lane whose extension index is t and whose ligation index is j (j < 0: a lane beyond len_p).  g0, g1 and
// stride are the wavefront's: the five words of a group come through scalar loads.
__device__ static inline void pile_groups(Pile& S, const PileupIn& I, uint32_t g0, uint32_t g1, uint32_t stride, int t, int j)
{
    uint32_t g = g0;
    for (; g + 3u * stride < g1; g += 4u * stride) {                                        // (g1 < 2^31: no wrap)
        uint32_t eb[4], eq[4], lb[4], lq[4];
        bool ok[4], pe[4], pl[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t gu = g + (uint32_t)u * stride;
            const int64_t eo = I.ext_off[gu], lo = I.lig_off[gu];
            const int el = (int)(I.ext_off[gu + 1] - eo), ll = (int)(I.lig_off[gu + 1] - lo);
            ok[u] = I.family[gu] >= I.min_family;
            pe[u] = t < el; pl[u] = j >= 0 && j < ll;
            const int64_t ie = eo + max(min(t, el - 1), 0), il = lo + max(min(j, ll - 1), 0);      // clamped: see the head of the file
            eb[u] = I.ext_seq[ie]; eq[u] = I.ext_qual[ie]; lb[u] = I.lig_seq[il]; lq[u] = I.lig_qual[il];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) S.add(ok[u], pe[u], pl[u], eb[u], eq[u], lb[u], lq[u], I.min_quality);
    }
    for (; g < g1; g += stride) {
        const int64_t eo = I.ext_off[g], lo = I.lig_off[g];
        const int el = (int)(I.ext_off[g + 1] - eo), ll = (int)(I.lig_off[g + 1] - lo);
        const int64_t ie = eo + max(min(t, el - 1), 0), il = lo + max(min(j, ll - 1), 0);
        S.add(I.family[g] >= I.min_family, t < el, j >= 0 && j < ll, I.ext_seq[ie], I.ext_qual[ie], I.lig_seq[il], I.lig_qual[il], I.min_quality);
    }
}

// the lane's template position of round r (len for a lane at or beyond the end: it counts nothing that is stored)
__device__ static inline int pileup_position(uint32_t r, int lane, int len) { return (int)min((int64_t)r * 64 + lane, (int64_t)len); }

__global__ __launch_bounds__(256) void k_pileup_wave(const uint2* __restrict__ units, int64_t n_units, const int32_t* __restrict__ mol_len, const int64_t* __restrict__ pos_off,
                                                     const uint32_t* __restrict__ start, PileupIn I, int32_t* __restrict__ counts)
{
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_units) return;                                                               // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const uint2 unit = units[k];
    const uint32_t p = __builtin_amdgcn_readfirstlane(unit.x), r = __builtin_amdgcn_readfirstlane(unit.y);      // (the unit is the wavefront's: scalar loads from here on)
    const int len = mol_len[p];
    const int t = pileup_position(r, lane, len);
    Pile S;
    pile_groups(S, I, start[p], start[p + 1], 1u, t, len - 1 - t);
    if (t < len) {
        int32_t* __restrict__ o = counts + (pos_off[p] + t) * PILEUP_COLUMNS;
        o[0] = S.a; o[1] = S.c; o[2] = S.g; o[3] = S.t; o[4] = S.d;
    }
}

// a workgroup per unit of the back list.  One round per workgroup, so ONE barrier: nothing overwrites `part` afterwards (k_consensus_vote_wg, which loops over
// rounds, needs its second one).
__global__ __launch_bounds__(256) void k_pileup_wg(const uint2* __restrict__ units, const int32_t* __restrict__ mol_len, const int64_t* __restrict__ pos_off,
                                                   const uint32_t* __restrict__ start, PileupIn I, int32_t* __restrict__ counts)
{
    __shared__ int part[3][PILEUP_COLUMNS][64];                                             // the counters of wavefronts 1..3: [wavefront - 1][column][lane], 3,840 bytes
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint2 unit = units[blockIdx.x];
    const uint32_t p = unit.x, r = unit.y;
    const int len = mol_len[p];
    const int t = pileup_position(r, lane, len);
    Pile S;
    pile_groups(S, I, start[p] + wave, start[p + 1], 4u, t, len - 1 - t);
    if (wave) { part[wave - 1][0][lane] = S.a; part[wave - 1][1][lane] = S.c; part[wave - 1][2][lane] = S.g; part[wave - 1][3][lane] = S.t; part[wave - 1][4][lane] = S.d; }
    __syncthreads();
    if (wave == 0 && t < len) {
#pragma unroll
        for (int w = 0; w < 3; w++) { S.a += part[w][0][lane]; S.c += part[w][1][lane]; S.g += part[w][2][lane]; S.t += part[w][3][lane]; S.d += part[w][4][lane]; }
        int32_t* __restrict__ o = counts + (pos_off[p] + t) * PILEUP_COLUMNS;
        o[0] = S.a; o[1] = S.c; o[2] = S.g; o[3] = S.t; o[4] = S.d;
    }
}

__device__ static inline long long wave_sum_i64(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(256) void k_pileup_sum(const int32_t* __restrict__ counts, int64_t n_pos, PileupCounters* __restrict__ ctr)
{
    long long bases = 0, disc = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pos; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t* __restrict__ c = counts + i * PILEUP_COLUMNS;
        bases += (long long)c[0] + c[1] + c[2] + c[3]; disc += c[4];
    }
    bases = wave_sum_i64(bases); disc = wave_sum_i64(disc);
    if ((threadIdx.x & 63) == 0) {
        if (bases) atomicAdd(&ctr->bases, (unsigned long long)bases);
        if (disc) atomicAdd(&ctr->discordant, (unsigned long long)disc);
    }
}

extern "C" {

// start[0, n] of the row whose first cell is cell0, the (cell, round) units of its n probes (n_units: the rounds of all probes) and ctr->used; ctr is zero on entry
hipError_t mipgen_launch_pileup_prepare(hipStream_t st, const uint64_t* keys, const int32_t* family, int64_t n_groups, uint32_t cell0, int32_t n, const int32_t* mol_len,
                                        int min_family, int64_t n_units, uint32_t* start, uint2* units, PileupCounters* ctr)
{
    if (n < 1 || n_groups < 1 || n_groups > 0x7fffffff || n_units < 1 || n_units > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pileup_cells, dim3((unsigned)(((int64_t)n + 1 + 255) / 256)), dim3(256), 0, st, keys, n_groups, cell0, n, start);
    hipLaunchKernelGGL(k_pileup_partition, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, st, start, mol_len, n, n_units, units, ctr);
    hipLaunchKernelGGL(k_pileup_used, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, start, n, family, n_groups, min_family, ctr);
    return hipGetLastError();
}

// units: k_pileup_partition's (the n_big workgroup units at its end); counts[n_pos][5] is written whole, then summed into ctr->bases / ctr->discordant
hipError_t mipgen_launch_pileup(hipStream_t st, const uint2* units, int64_t n_units, int64_t n_small, int64_t n_big, const int32_t* mol_len, const int64_t* pos_off,
                                const uint32_t* start, const int32_t* family, const int64_t* ext_off, const int64_t* lig_off, const uint8_t* ext_seq, const uint8_t* ext_qual,
                                const uint8_t* lig_seq, const uint8_t* lig_qual, int min_family, int min_quality, int64_t n_pos, int32_t* counts, PileupCounters* ctr)
{
    if (n_small < 0 || n_big < 0 || n_small + n_big != n_units || n_units > 0x7fffffff || n_pos < 1) return hipErrorInvalidValue;
    const PileupIn I{family, ext_off, lig_off, ext_seq, ext_qual, lig_seq, lig_qual, min_family, min_quality};
    if (n_small > 0) hipLaunchKernelGGL(k_pileup_wave, dim3((unsigned)((n_small + 3) / 4)), dim3(256), 0, st, units, n_small, mol_len, pos_off, start, I, counts);
    if (n_big > 0) hipLaunchKernelGGL(k_pileup_wg, dim3((unsigned)n_big), dim3(256), 0, st, units + n_small, mol_len, pos_off, start, I, counts);
    hipLaunchKernelGGL(k_pileup_sum, dim3((unsigned)std::min<int64_t>((n_pos + 255) / 256, 2048)), dim3(256), 0, st, counts, n_pos, ctr);
    return hipGetLastError();
}

}
