// kernels_locus.hip — the fold from template positions to genome loci between the count and the call.  A plan gives every template position x of a
// table either no locus (-1) or locus * 4 + flags (bit 0: the probe is on the minus strand; bit 1: the insertion columns of this source are those of row x - 1).
//
//  The plan on the device, once per installed plan:
//  k_locus_keys     a lane per x: key = locus (n_loci for -1, the sentinel that sorts last), id = x.  The pairs go through the device radix sort the consensus path
//                   links (mipgen_consensus_sort); it is stable, so the sources of a locus stand in ascending x.
//  k_locus_sources  a lane per sorted element: src[i] = x << 2 | flags (x < 2^29: it fits 32 bits).
//  k_locus_first    a lane per locus and one more: first[l] = the lower bound of l in the sorted keys, the shape of k_pileup_cells.  The sources of locus l are
//                   src[first[l], first[l + 1]); a locus without a source has an empty run and needs no special case; the excluded positions lie behind first[n_loci].
//  The fold, once per table:
//  k_locus_merge    a lane per locus, a loop over its sources.  A source row comes through call_load_row's wide loads (count_row.h); a minus source adds A <-> T and
//                   C <-> G swapped, discordant and del as they are; the insertion columns are the row's own on a plus source, 0 on a minus one, and those of row
//                   x - 1 (one more 8-byte load) under bit 1 on either strand.  The merged row is stored once with the same wide stores: a lane owns its locus, so
//                   there is no atomic and no zeroing pass (the reason of 4.12).  Consecutive loci of a plus probe read consecutive rows, of a minus probe
//                   descending ones.  32-bit counters: a merged counter is at most the groups of the session - a molecule belongs to one probe and adds at most one
//                   to a column of one position of it, and the plan builders give a locus at most one position per probe - and a session holds fewer than 2^31.
//  k_locus_sum      the totals of a merged table: loci with any non-zero counter by ballot, the sums of A + C + G + T, discordant and (8 columns) del, ins,
//                   ins_discordant: wave-uniform grid-stride rounds, wave_sum_i64 and one atomic per wavefront and counter, as k_pile_sum.
// Bound: 4 bytes of src per source + its row (20 or 32 bytes, 8 more under bit 1) + the merged row written, streaming.  No LDS, no scratch, vector stores only.
#include "kernels.h"
#include "device_utils.h"
#include "count_row.h"

__global__ __launch_bounds__(256) void k_locus_keys(const int64_t* __restrict__ plan, int64_t n_pos, int64_t n_loci, uint64_t* __restrict__ keys, uint32_t* __restrict__ ids)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_pos) return;
    const int64_t e = plan[x];
    keys[x] = e < 0 ? (uint64_t)n_loci : (uint64_t)(e >> 2);
    ids[x] = (uint32_t)x;
}

__global__ __launch_bounds__(256) void k_locus_sources(const uint32_t* __restrict__ ids_sorted, const int64_t* __restrict__ plan, int64_t n_pos, uint32_t* __restrict__ src)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pos) return;
    const uint32_t x = ids_sorted[i];
    const int64_t e = plan[x];
    src[i] = x << 2 | (e < 0 ? 0u : (uint32_t)(e & 3));                                     // (an excluded position lies behind first[n_loci]: never read)
}

__global__ __launch_bounds__(256) void k_locus_first(const uint64_t* __restrict__ keys_sorted, int64_t n_pos, int64_t n_loci, uint32_t* __restrict__ first)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l > n_loci) return;
    int64_t lo = 0, hi = n_pos;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys_sorted[mid] < (uint64_t)l) lo = mid + 1; else hi = mid;
    }
    first[l] = (uint32_t)lo;
}

template <int COLUMNS>
__global__ __launch_bounds__(256) void k_locus_merge(const int32_t* __restrict__ counts, const uint32_t* __restrict__ src, const uint32_t* __restrict__ first, int64_t n_loci,
                                                     int32_t* __restrict__ merged)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_loci) return;
    int32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t i1 = first[l + 1];
    for (uint32_t i = first[l]; i < i1; i++) {
        const uint32_t s = src[i];
        const int64_t x = (int64_t)(s >> 2);
        int32_t c[8];
        call_load_row(counts, COLUMNS, x, c);
        if (s & 1u) { m[0] += c[3]; m[1] += c[2]; m[2] += c[1]; m[3] += c[0]; }
        else { m[0] += c[0]; m[1] += c[1]; m[2] += c[2]; m[3] += c[3]; }
        m[4] += c[4];
        if (COLUMNS == 8) {
            m[5] += c[5];
            if (s & 2u) {                                                                   // (x >= 1: the host refuses bit 1 at x = 0)
                const int2 a = *(const int2*)(counts + (x - 1) * 8 + 6);
                m[6] += a.x; m[7] += a.y;
            } else if (!(s & 1u)) { m[6] += c[6]; m[7] += c[7]; }
        }
    }
    call_store_row(merged, COLUMNS, l, m);
}

template <int COLUMNS>
__global__ __launch_bounds__(256) void k_locus_sum(const int32_t* __restrict__ merged, int64_t n_loci, LocusCounters* __restrict__ ctr)
{
    long long s[5] = {0, 0, 0, 0, 0}, covered = 0;                                          // bases, discordant, del, ins, ins_discordant
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) - lane, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = wave0; i0 < n_loci; i0 += step) {                                     // (wave-uniform rounds: every lane runs the ballot)
        const int64_t l = i0 + lane;
        int32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (l < n_loci) call_load_row(merged, COLUMNS, l, c);
        covered += __popcll(__ballot((c[0] | c[1] | c[2] | c[3] | c[4] | c[5] | c[6] | c[7]) != 0)) * (lane == 0);
        s[0] += (long long)c[0] + c[1] + c[2] + c[3]; s[1] += c[4]; s[2] += c[5]; s[3] += c[6]; s[4] += c[7];
    }
    unsigned long long* const out[5] = {&ctr->bases, &ctr->discordant, &ctr->deletions, &ctr->insertions, &ctr->ins_discordant};
#pragma unroll
    for (int k = 0; k < (COLUMNS == 8 ? 5 : 2); k++) {
        const long long t = wave_sum_i64(s[k]);
        if (lane == 0 && t) atomicAdd(out[k], (unsigned long long)t);
    }
    if (lane == 0 && covered) atomicAdd(&ctr->covered, (unsigned long long)covered);
}

extern "C" {

static inline bool locus_shape_ok(int64_t n_pos, int64_t n_loci) { return n_pos >= 1 && n_pos <= MIPGEN_CALL_MAX_POSITIONS && n_loci >= 1 && n_loci <= MIPGEN_CALL_MAX_POSITIONS; }
static inline unsigned locus_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

hipError_t mipgen_launch_locus_keys(hipStream_t st, const int64_t* plan, int64_t n_pos, int64_t n_loci, uint64_t* keys, uint32_t* ids)
{
    if (!locus_shape_ok(n_pos, n_loci)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_locus_keys, dim3(locus_blocks(n_pos)), dim3(256), 0, st, plan, n_pos, n_loci, keys, ids);
    return hipGetLastError();
}

// src[n_pos] and first[n_loci + 1] from the sorted pairs
hipError_t mipgen_launch_locus_index(hipStream_t st, const uint64_t* keys_sorted, const uint32_t* ids_sorted, const int64_t* plan, int64_t n_pos, int64_t n_loci, uint32_t* src,
                                     uint32_t* first)
{
    if (!locus_shape_ok(n_pos, n_loci)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_locus_sources, dim3(locus_blocks(n_pos)), dim3(256), 0, st, ids_sorted, plan, n_pos, src);
    hipLaunchKernelGGL(k_locus_first, dim3(locus_blocks(n_loci + 1)), dim3(256), 0, st, keys_sorted, n_pos, n_loci, first);
    return hipGetLastError();
}

// merged[n_loci][columns] is written whole, then summed into ctr (zero on entry)
hipError_t mipgen_launch_locus_merge(hipStream_t st, const int32_t* counts, int columns, const uint32_t* src, const uint32_t* first, int64_t n_pos, int64_t n_loci,
                                     int32_t* merged, LocusCounters* ctr)
{
    if (!locus_shape_ok(n_pos, n_loci) || (columns != 5 && columns != 8)) return hipErrorInvalidValue;
    const unsigned sum_blocks = (unsigned)std::min<int64_t>((n_loci + 255) / 256, 2048);
    if (columns == 8) {
        hipLaunchKernelGGL(k_locus_merge<8>, dim3(locus_blocks(n_loci)), dim3(256), 0, st, counts, src, first, n_loci, merged);
        hipLaunchKernelGGL(k_locus_sum<8>, dim3(sum_blocks), dim3(256), 0, st, merged, n_loci, ctr);
    } else {
        hipLaunchKernelGGL(k_locus_merge<5>, dim3(locus_blocks(n_loci)), dim3(256), 0, st, counts, src, first, n_loci, merged);
        hipLaunchKernelGGL(k_locus_sum<5>, dim3(sum_blocks), dim3(256), 0, st, merged, n_loci, ctr);
    }
    return hipGetLastError();
}

}
