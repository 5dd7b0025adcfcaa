// kernels_consensus.hip — single-molecule consensus reads per (row, probe, tag) group.
//
//  k_member_keys          a lane per pair of the chunk just assigned: (key, global pair id) and where its reads lie in the arena; a pair that joins no group
//                         gets the sentinel key, which sorts behind every group.
//  sort + run boundaries  hipCUB (rocPRIM): one radix sort of (key, pair id) over the key bits that can be set, run-length encode of the member keys (group key,
//                         family size), exclusive sums (group_start, output offsets).
//  k_consensus_partition  a lane per group: its index into the one-wavefront list (from the front) or the workgroup list (from the back).
//  k_consensus_len[_big]  per group the minimum member length of each side behind its tag: a lane per small group, a wavefront per large one.
//  k_consensus_vote_wave  a WAVEFRONT per group, LANES OVER POSITIONS, a loop over the members: lane l of round r owns position 64 r + l, so what a wavefront
//  k_consensus_vote_wg    loads of one member is 64 consecutive base bytes and 64 consecutive quality bytes of one read - the opposite of k_read_assign's lane
//                         per pair (64 lanes, 64 cache lines).  Four sums per lane in registers, the member loop unrolled by four (8 byte loads in flight per
//                         lane), coalesced byte stores.  _wg: a family above CONSENSUS_WG_FAMILY takes a 256-thread workgroup; its four wavefronts stride over
//                         the members and add their sums through LDS.  Bound: the retained read bytes behind the tags once (base + quality) and the record of
//                         every member (32 bytes, wave-uniform); 2 bytes written per consensus position.
#include <hipcub/hipcub.hpp>

#include "kernels.h"

__device__ static inline int wave_count(bool pred) { return __popcll(__ballot(pred)); }

__global__ __launch_bounds__(256) void k_member_keys(ReadsParams P, int64_t n_pairs, uint32_t pair0, const int32_t* __restrict__ assign, const int32_t* __restrict__ row,
                                                     const uint8_t* __restrict__ ext_bytes, const int64_t* __restrict__ ext_off, int64_t ext_base,
                                                     const uint8_t* __restrict__ lig_bytes, const int64_t* __restrict__ lig_off, int64_t lig_base, int64_t qdelta,
                                                     uint64_t sentinel, uint64_t* __restrict__ keys, uint32_t* __restrict__ ids, ConsensusPair* __restrict__ recs,
                                                     ConsensusCounters* __restrict__ cctr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n_pairs;
    bool member = false;
    if (active) {
        const int64_t eb = ext_off[i] - ext_base, ee = ext_off[i + 1] - ext_base;
        const int64_t lb = lig_off[i] - lig_base, le = lig_off[i + 1] - lig_base;
        const int result = assign[i];
        uint64_t key = sentinel;
        if (result >= 0) {
            uint32_t tag = 0;
            bool clean = pack_tag(ext_bytes, eb, P.te, &tag);                              // (an assigned pair's reads hold their tags, as in k_read_assign)
            clean = pack_tag(lig_bytes, lb, P.tl, &tag) && clean;
            const uint32_t cell = row ? (uint32_t)row[i] * (uint32_t)P.n_probes + (uint32_t)result : (uint32_t)result;
            if (clean) { key = ((uint64_t)cell << 32) | tag; member = true; }
        }
        keys[i] = key;
        ids[i] = pair0 + (uint32_t)i;
        ConsensusPair r;
        r.ext = ext_bytes + eb; r.lig = lig_bytes + lb; r.qdelta = qdelta;
        r.ext_len = (int32_t)min(ee - eb, (int64_t)0x7fffffff); r.lig_len = (int32_t)min(le - lb, (int64_t)0x7fffffff);
        recs[i] = r;
    }
    const int n_mem = wave_count(member);
    if ((threadIdx.x & 63) == 0 && n_mem) atomicAdd(&cctr->members, (unsigned long long)n_mem);
}

// order[0, n_small): the groups of at most CONSENSUS_WG_FAMILY members; order[n_groups - n_big, n_groups): the others (neither list is in group order: a group
// writes to its own output offsets whoever votes it)
__global__ __launch_bounds__(256) void k_consensus_partition(const int32_t* __restrict__ family, int64_t n_groups, uint32_t* __restrict__ order,
                                                             ConsensusCounters* __restrict__ cctr)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = g < n_groups;
    const bool big = active && family[g] > CONSENSUS_WG_FAMILY, small = active && !big;
    const unsigned long long ms = __ballot(small), mb = __ballot(big);
    const int lane = threadIdx.x & 63;
    unsigned long long bs = 0, bb = 0;
    if (lane == 0) {
        if (ms) bs = atomicAdd(&cctr->n_small, (unsigned long long)__popcll(ms));
        if (mb) bb = atomicAdd(&cctr->n_big, (unsigned long long)__popcll(mb));
    }
    bs = __shfl(bs, 0); bb = __shfl(bb, 0);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (small) order[bs + (unsigned long long)__popcll(ms & below)] = (uint32_t)g;
    if (big) order[(unsigned long long)n_groups - 1ull - (bb + (unsigned long long)__popcll(mb & below))] = (uint32_t)g;
}

// a lane per group of at most CONSENSUS_WG_FAMILY members (the larger ones: k_consensus_len_big)
__global__ __launch_bounds__(256) void k_consensus_len(int te, int tl, int64_t n_groups, const uint32_t* __restrict__ group_start, const int32_t* __restrict__ family,
                                                       const uint32_t* __restrict__ ids, const ConsensusPair* __restrict__ recs, int64_t* __restrict__ ext_len,
                                                       int64_t* __restrict__ lig_len)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const int f = family[g];
    if (f > CONSENSUS_WG_FAMILY) return;
    const uint32_t s = group_start[g];
    int me = 0x7fffffff, ml = 0x7fffffff;
    for (int m = 0; m < f; m++) {
        const ConsensusPair r = recs[ids[s + (uint32_t)m]];
        me = min(me, r.ext_len); ml = min(ml, r.lig_len);
    }
    ext_len[g] = max(me - te, 0); lig_len[g] = max(ml - tl, 0);
}

__device__ static inline int wave_min(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}

// a wavefront per group of the workgroup list: the lanes stride over the members
__global__ __launch_bounds__(256) void k_consensus_len_big(int te, int tl, const uint32_t* __restrict__ big, int64_t n_big, const uint32_t* __restrict__ group_start,
                                                           const int32_t* __restrict__ family, const uint32_t* __restrict__ ids, const ConsensusPair* __restrict__ recs,
                                                           int64_t* __restrict__ ext_len, int64_t* __restrict__ lig_len)
{
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_big) return;                                                                 // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const uint32_t g = big[k], s = group_start[g];
    const int f = family[g];
    int me = 0x7fffffff, ml = 0x7fffffff;
    for (int m = lane; m < f; m += 64) {
        const ConsensusPair r = recs[ids[s + (uint32_t)m]];
        me = min(me, r.ext_len); ml = min(ml, r.lig_len);
    }
    me = wave_min(me); ml = wave_min(ml);
    if (lane == 0) { ext_len[g] = max(me - te, 0); lig_len[g] = max(ml - tl, 0); }
}

// ---- the vote ----------------------------------------------------------------------------------------------------------------------------------------
// the four sums of a position; T is uint32_t where the number of members is bounded (the bound is next to the instantiation), uint64_t otherwise
template <typename T>
struct Votes {
    T a = 0, c = 0, g = 0, t = 0;
    __device__ inline void add(uint32_t base, uint32_t qual)
    {
        const int qi = (int)qual - 33;
        const T q = (T)min(max(qi, 0), CONSENSUS_MAX_Q);
        a += base == 'A' ? q : (T)0; c += base == 'C' ? q : (T)0; g += base == 'G' ? q : (T)0; t += base == 'T' ? q : (T)0;      // any other byte casts no vote
    }
};

// consensus base and quality of one position from its four sums: the strictly largest sum wins, v = S[best] - sum of the others; a shared
// largest sum, or no vote at all, is N with v = -sum; v > 40 prints 'I', v < 2 '#', else chr(v + 33)
template <typename T>
__device__ static inline void call_base(const Votes<T>& S, uint8_t* base, uint8_t* qual)
{
    const T mx = max(max(S.a, S.c), max(S.g, S.t));
    const int at_max = (int)(S.a == mx) + (int)(S.c == mx) + (int)(S.g == mx) + (int)(S.t == mx);
    const bool called = mx > 0 && at_max == 1;
    const T total = S.a + S.c + S.g + S.t;
    *base = !called ? 'N' : S.a == mx ? 'A' : S.c == mx ? 'C' : S.g == mx ? 'G' : 'T';
    // v = 2 mx - total when called (>= 1), <= 0 otherwise: only the range 2..40 is printed as a number
    const T others = total - mx;
    const bool low = !called || mx < others + 2;
    const bool high = called && mx > others + 40;
    *qual = low ? '#' : high ? 'I' : (uint8_t)((uint32_t)(mx - others) + 33u);
}

// members [m0, f) of the group in steps of `stride` into S, for the position whose byte lies `at` bytes into every member's read (the tag included)
template <typename T>
__device__ static inline void vote_members(Votes<T>& S, const uint32_t* __restrict__ ids, const ConsensusPair* __restrict__ recs, uint32_t s, int m0, int f, int stride,
                                           bool lig, int64_t at)
{
    int m = m0;
    for (; m + 3 * stride < f; m += 4 * stride) {
        uint32_t b[4], q[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t id = __builtin_amdgcn_readfirstlane(ids[s + (uint32_t)(m + u * stride)]);      // (the member is the wavefront's: scalar loads)
            const ConsensusPair r = recs[id];
            const uint8_t* __restrict__ p = (lig ? r.lig : r.ext) + at;
            b[u] = p[0]; q[u] = p[r.qdelta];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) S.add(b[u], q[u]);
    }
    for (; m < f; m += stride) {
        const uint32_t id = __builtin_amdgcn_readfirstlane(ids[s + (uint32_t)m]);
        const ConsensusPair r = recs[id];
        const uint8_t* __restrict__ p = (lig ? r.lig : r.ext) + at;
        S.add(p[0], p[r.qdelta]);
    }
}

// 32-bit sums: a group of this kernel has at most CONSENSUS_WG_FAMILY members of at most CONSENSUS_MAX_Q each
static_assert((long long)CONSENSUS_WG_FAMILY * CONSENSUS_MAX_Q < (1ll << 31), "k_consensus_vote_wave keeps 32-bit sums");

__global__ __launch_bounds__(256) void k_consensus_vote_wave(int te, int tl, const uint32_t* __restrict__ small, int64_t n_small, const uint32_t* __restrict__ group_start,
                                                             const int32_t* __restrict__ family, const uint32_t* __restrict__ ids, const ConsensusPair* __restrict__ recs,
                                                             const int64_t* __restrict__ ext_off, const int64_t* __restrict__ lig_off, uint8_t* __restrict__ ext_seq,
                                                             uint8_t* __restrict__ ext_qual, uint8_t* __restrict__ lig_seq, uint8_t* __restrict__ lig_qual)
{
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_small) return;                                                               // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const uint32_t g = small[k], s = group_start[g];
    const int f = family[g];
    for (int side = 0; side < 2; side++) {
        const int64_t o = side ? lig_off[g] : ext_off[g];
        const int64_t L = (side ? lig_off[g + 1] : ext_off[g + 1]) - o;                     // <= the length of every member behind its tag
        const int skip = side ? tl : te;
        uint8_t* __restrict__ seq = (side ? lig_seq : ext_seq) + o;
        uint8_t* __restrict__ qual = (side ? lig_qual : ext_qual) + o;
        for (int64_t p0 = 0; p0 < L; p0 += 64) {
            const int64_t p = p0 + lane;
            Votes<uint32_t> S;
            vote_members(S, ids, recs, s, 0, f, 1, side != 0, skip + min(p, L - 1));        // (a lane beyond the end reads the last position and stores nothing)
            uint8_t cb, cq;
            call_base(S, &cb, &cq);
            if (p < L) { seq[p] = cb; qual[p] = cq; }
        }
    }
}

// a workgroup per group of more than CONSENSUS_WG_FAMILY members; 64-bit sums (a family has up to 2^31 - 1 members: 93 * 2^31 does not fit 32 bits)
__global__ __launch_bounds__(256) void k_consensus_vote_wg(int te, int tl, const uint32_t* __restrict__ big, const uint32_t* __restrict__ group_start,
                                                           const int32_t* __restrict__ family, const uint32_t* __restrict__ ids, const ConsensusPair* __restrict__ recs,
                                                           const int64_t* __restrict__ ext_off, const int64_t* __restrict__ lig_off, uint8_t* __restrict__ ext_seq,
                                                           uint8_t* __restrict__ ext_qual, uint8_t* __restrict__ lig_seq, uint8_t* __restrict__ lig_qual)
{
    __shared__ unsigned long long part[3][4][64];                                           // the sums of wavefronts 1..3: [wavefront - 1][base][lane], 6 KiB
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t g = big[blockIdx.x], s = group_start[g];
    const int f = family[g];
    for (int side = 0; side < 2; side++) {
        const int64_t o = side ? lig_off[g] : ext_off[g];
        const int64_t L = (side ? lig_off[g + 1] : ext_off[g + 1]) - o;
        const int skip = side ? tl : te;
        uint8_t* __restrict__ seq = (side ? lig_seq : ext_seq) + o;
        uint8_t* __restrict__ qual = (side ? lig_qual : ext_qual) + o;
        for (int64_t p0 = 0; p0 < L; p0 += 64) {                                            // (L is the workgroup's: every thread runs the same rounds)
            const int64_t p = p0 + lane;
            Votes<unsigned long long> S;
            vote_members(S, ids, recs, s, wave, f, 4, side != 0, skip + min(p, L - 1));
            if (wave) { part[wave - 1][0][lane] = S.a; part[wave - 1][1][lane] = S.c; part[wave - 1][2][lane] = S.g; part[wave - 1][3][lane] = S.t; }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int w = 0; w < 3; w++) { S.a += part[w][0][lane]; S.c += part[w][1][lane]; S.g += part[w][2][lane]; S.t += part[w][3][lane]; }
                uint8_t cb, cq;
                call_base(S, &cb, &cq);
                if (p < L) { seq[p] = cb; qual[p] = cq; }
            }
            __syncthreads();                                                                // (the next round overwrites `part`)
        }
    }
}

extern "C" {

hipError_t mipgen_launch_member_keys(hipStream_t st, const ReadsParams* P, int64_t n_pairs, uint32_t pair0, const int32_t* assign, const int32_t* row, const uint8_t* ext_bytes,
                                     const int64_t* ext_off, int64_t ext_base, const uint8_t* lig_bytes, const int64_t* lig_off, int64_t lig_base, int64_t qdelta,
                                     uint64_t sentinel, uint64_t* keys, uint32_t* ids, ConsensusPair* recs, ConsensusCounters* cctr)
{
    if (n_pairs <= 0) return hipSuccess;
    const int64_t blocks = (n_pairs + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_member_keys, dim3((unsigned)blocks), dim3(256), 0, st, *P, n_pairs, pair0, assign, row, ext_bytes, ext_off, ext_base, lig_bytes, lig_off, lig_base,
                       qdelta, sentinel, keys, ids, recs, cctr);
    return hipGetLastError();
}

// (keys_in, ids_in)[0, n) -> sorted by the low `end_bit` key bits in (keys_out, ids_out); temp == nullptr: the scratch size
hipError_t mipgen_consensus_sort(hipStream_t st, void* temp, size_t* temp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* ids_in, uint32_t* ids_out,
                                 int64_t n, int end_bit)
{
    if (n > 0x7fffffff) return hipErrorInvalidValue;
    size_t need = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, need, keys_in, keys_out, ids_in, ids_out, (int)n, 0, end_bit, st);
    if (e != hipSuccess) return e;
    if (!temp) { *temp_bytes = need; return hipSuccess; }
    if (*temp_bytes < need) return hipErrorInvalidValue;
    size_t t = *temp_bytes;
    return hipcub::DeviceRadixSort::SortPairs(temp, t, keys_in, keys_out, ids_in, ids_out, (int)n, 0, end_bit, st);
}

// the runs of keys[0, n) (sorted): group_keys, family and their number; temp == nullptr: the scratch size
hipError_t mipgen_consensus_runs(hipStream_t st, void* temp, size_t* temp_bytes, const uint64_t* keys, int64_t n, uint64_t* group_keys, int32_t* family,
                                 unsigned long long* n_groups)
{
    if (n > 0x7fffffff) return hipErrorInvalidValue;
    size_t need = 0;
    hipError_t e = hipcub::DeviceRunLengthEncode::Encode(nullptr, need, keys, group_keys, family, n_groups, (int)n, st);
    if (e != hipSuccess) return e;
    if (!temp) { *temp_bytes = need; return hipSuccess; }
    if (*temp_bytes < need) return hipErrorInvalidValue;
    size_t t = *temp_bytes;
    return hipcub::DeviceRunLengthEncode::Encode(temp, t, keys, group_keys, family, n_groups, (int)n, st);
}

// family[0, n) -> group_start[0, n) (their sum is below 2^31: a session holds at most 2^31 - 1 pairs); temp == nullptr: the scratch size
hipError_t mipgen_consensus_scan_u32(hipStream_t st, void* temp, size_t* temp_bytes, const int32_t* family, uint32_t* group_start, int64_t n)
{
    if (n > 0x7fffffff) return hipErrorInvalidValue;
    size_t need = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, reinterpret_cast<const uint32_t*>(family), group_start, (int)n, st);
    if (e != hipSuccess) return e;
    if (!temp) { *temp_bytes = need; return hipSuccess; }
    if (*temp_bytes < need) return hipErrorInvalidValue;
    size_t t = *temp_bytes;
    return hipcub::DeviceScan::ExclusiveSum(temp, t, reinterpret_cast<const uint32_t*>(family), group_start, (int)n, st);
}

// len[0, n) -> off[0, n), 64-bit; temp == nullptr: the scratch size
hipError_t mipgen_consensus_scan_i64(hipStream_t st, void* temp, size_t* temp_bytes, const int64_t* len, int64_t* off, int64_t n)
{
    if (n > 0x7fffffff) return hipErrorInvalidValue;
    size_t need = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, len, off, (int)n, st);
    if (e != hipSuccess) return e;
    if (!temp) { *temp_bytes = need; return hipSuccess; }
    if (*temp_bytes < need) return hipErrorInvalidValue;
    size_t t = *temp_bytes;
    return hipcub::DeviceScan::ExclusiveSum(temp, t, len, off, (int)n, st);
}

hipError_t mipgen_launch_consensus_partition(hipStream_t st, const int32_t* family, int64_t n_groups, uint32_t* order, ConsensusCounters* cctr)
{
    if (n_groups <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_consensus_partition, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, family, n_groups, order, cctr);
    return hipGetLastError();
}

// order: k_consensus_partition's (the n_big large groups at its end)
hipError_t mipgen_launch_consensus_len(hipStream_t st, int te, int tl, int64_t n_groups, const uint32_t* order, int64_t n_big, const uint32_t* group_start,
                                       const int32_t* family, const uint32_t* ids, const ConsensusPair* recs, int64_t* ext_len, int64_t* lig_len)
{
    if (n_groups <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_consensus_len, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, te, tl, n_groups, group_start, family, ids, recs, ext_len, lig_len);
    if (n_big > 0)
        hipLaunchKernelGGL(k_consensus_len_big, dim3((unsigned)((n_big + 3) / 4)), dim3(256), 0, st, te, tl, order + (n_groups - n_big), n_big, group_start, family, ids, recs,
                           ext_len, lig_len);
    return hipGetLastError();
}

hipError_t mipgen_launch_consensus_vote(hipStream_t st, int te, int tl, int64_t n_groups, const uint32_t* order, int64_t n_small, int64_t n_big, const uint32_t* group_start,
                                        const int32_t* family, const uint32_t* ids, const ConsensusPair* recs, const int64_t* ext_off, const int64_t* lig_off,
                                        uint8_t* ext_seq, uint8_t* ext_qual, uint8_t* lig_seq, uint8_t* lig_qual)
{
    if (n_small + n_big != n_groups) return hipErrorInvalidValue;
    if (n_small > 0)
        hipLaunchKernelGGL(k_consensus_vote_wave, dim3((unsigned)((n_small + 3) / 4)), dim3(256), 0, st, te, tl, order, n_small, group_start, family, ids, recs, ext_off,
                           lig_off, ext_seq, ext_qual, lig_seq, lig_qual);
    if (n_big > 0)
        hipLaunchKernelGGL(k_consensus_vote_wg, dim3((unsigned)n_big), dim3(256), 0, st, te, tl, order + n_small, group_start, family, ids, recs, ext_off, lig_off, ext_seq,
                           ext_qual, lig_seq, lig_qual);
    return hipGetLastError();
}

}
