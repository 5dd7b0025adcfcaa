// pileup_frame.h — the count frame of both pileup tables: kernels_pileup.hip instantiates it for Pile (5 columns), kernels_gapped.hip for GapPile
// (8 columns).  A policy V is the accumulator of one lane: int n[V::COLUMNS]; V::groups(S, C, R, g0, g1, stride, t, len, extra...) - the groups
// g0, g0 + stride, ... below g1 voted into S for the lane at template position t; S.store(o) - the lane's position written; V::Counters and V::SUMS - which
// column ranges k_pile_sum adds into which counter.
//
//  k_pile_wave  a WAVEFRONT per (cell, round) unit of the front list, LANES OVER TEMPLATE POSITIONS: lane l owns t = 64 r + l, CLAMPED to len for a lane at or
//               beyond the end (it counts nothing that is stored).  The unit is the wavefront's, so everything the group loop reads per group is a scalar load.
//  k_pile_wg    a 256-thread workgroup per unit of the back list (a cell above PILEUP_WG_CELL): its four wavefronts stride over the groups and add through LDS,
//               part[3][COLUMNS][64].  One round per workgroup, so ONE barrier: nothing overwrites `part` afterwards (k_consensus_vote_wg, which loops over
//               rounds, needs its second one).  No atomic in either.
//  k_pile_sum   the sums of column ranges of the finished table: a grid-stride pass, one atomic per wavefront and counter.
#pragma once
#include "kernels.h"
#include "device_utils.h"

template <class Ctr>
struct ColumnSum { int first, end; unsigned long long Ctr::*counter; };          // columns [first, end) of the table add up to this counter

// the lane's template position of round r
__device__ static inline int pile_position(uint32_t r, int lane, int len) { return (int)min((int64_t)r * 64 + lane, (int64_t)len); }

template <class V, class... X>
__global__ __launch_bounds__(256) void k_pile_wave(ConsensusView C, PileRow R, int32_t* __restrict__ counts, X... extra)
{
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= R.n_small) return;                                                             // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const uint2 unit = R.units[k];
    const uint32_t p = __builtin_amdgcn_readfirstlane(unit.x), r = __builtin_amdgcn_readfirstlane(unit.y);      // (the unit is the wavefront's: scalar loads from here on)
    const int len = R.mol_len[p];
    const int t = pile_position(r, lane, len);
    V S;
    V::groups(S, C, R, R.start[p], R.start[p + 1], 1u, t, len, extra...);
    if (t < len) S.store(counts + (R.pos_off[p] + t) * V::COLUMNS);
}

template <class V, class... X>
__global__ __launch_bounds__(256) void k_pile_wg(ConsensusView C, PileRow R, int32_t* __restrict__ counts, X... extra)
{
    __shared__ int part[3][V::COLUMNS][64];                                                 // the counters of wavefronts 1..3: [wavefront - 1][column][lane]
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint2 unit = R.units[R.n_small + blockIdx.x];
    const uint32_t p = unit.x, r = unit.y;
    const int len = R.mol_len[p];
    const int t = pile_position(r, lane, len);
    V S;
    V::groups(S, C, R, R.start[p] + wave, R.start[p + 1], 4u, t, len, extra...);
    if (wave) {
#pragma unroll
        for (int c = 0; c < V::COLUMNS; c++) part[wave - 1][c][lane] = S.n[c];
    }
    __syncthreads();
    if (wave == 0 && t < len) {
#pragma unroll
        for (int w = 0; w < 3; w++) {
#pragma unroll
            for (int c = 0; c < V::COLUMNS; c++) S.n[c] += part[w][c][lane];
        }
        S.store(counts + (R.pos_off[p] + t) * V::COLUMNS);
    }
}

template <class V>
__global__ __launch_bounds__(256) void k_pile_sum(const int32_t* __restrict__ counts, int64_t n_pos, typename V::Counters* __restrict__ ctr)
{
    constexpr int N = (int)(sizeof(V::SUMS) / sizeof(V::SUMS[0]));
    long long s[N] = {};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pos; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t* __restrict__ row = counts + i * V::COLUMNS;
#pragma unroll
        for (int k = 0; k < N; k++) {
#pragma unroll
            for (int c = V::SUMS[k].first; c < V::SUMS[k].end; c++) s[k] += row[c];
        }
    }
#pragma unroll
    for (int k = 0; k < N; k++) {
        s[k] = wave_sum_i64(s[k]);
        if ((threadIdx.x & 63) == 0 && s[k]) atomicAdd(&(ctr->*V::SUMS[k].counter), (unsigned long long)s[k]);
    }
}

// the three launches of a table: counts[R.n_pos][V::COLUMNS] is written whole, then summed into ctr
template <class V, class... X>
static inline hipError_t pile_launch(hipStream_t st, const ConsensusView& C, const PileRow& R, int32_t* counts, typename V::Counters* ctr, X... extra)
{
    if (R.n_small > 0) hipLaunchKernelGGL((k_pile_wave<V, X...>), dim3((unsigned)((R.n_small + 3) / 4)), dim3(256), 0, st, C, R, counts, extra...);
    if (R.n_big > 0) hipLaunchKernelGGL((k_pile_wg<V, X...>), dim3((unsigned)R.n_big), dim3(256), 0, st, C, R, counts, extra...);
    hipLaunchKernelGGL((k_pile_sum<V>), dim3((unsigned)std::min<int64_t>((R.n_pos + 255) / 256, 2048)), dim3(256), 0, st, counts, R.n_pos, ctr);
    return hipGetLastError();
}
