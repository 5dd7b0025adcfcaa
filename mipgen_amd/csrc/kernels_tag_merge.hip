// kernels_tag_merge.hip — molecular tags one substitution apart merged by the count rule before the consensus.  The rule itself is tag_merge.h's;
// these are its lanes.
//
//  k_tag_parent    a lane per raw group: up to 3 L neighbour keys looked up in the sorted, duplicate-free group keys through the nested windows of tag_parent
//                  (two searches of the whole array for the cell's range, then five searches per tag position in a window that shrinks by a factor of four per
//                  position and ends the walk once it holds the lane's own key alone); the best eligible parent's group index, or -1.
//  k_tag_root      a lane per raw group: parents followed to the root under the bound of TAG_MERGE_MAX_LINKS; absorbed groups counted by ballot and popcount, moved
//                  pairs and the deepest chain by a wavefront reduction, one atomic each per wavefront.
//  k_tag_rewrite   a lane per PAIR of the sorted (key, pair id) list: a member finds its raw group by a search of its key in the group keys - no lane loops over a
//                  family, so a family of 5,000 costs what 5,000 singletons cost - and takes its root's key; a sentinel key (a pair in no group) is copied as it is
//                  and still sorts last.  The pairs go back to the unsorted arrays, where the second sort reads them.
#include "kernels.h"
#include "tag_merge.h"

__global__ __launch_bounds__(256) void k_tag_parent(const uint64_t* __restrict__ keys, const int32_t* __restrict__ family, int64_t n_groups, int L, int32_t* __restrict__ parent)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    parent[g] = (int32_t)tag_parent(keys, family, n_groups, g, L);
}

__device__ static inline unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ static inline int wave_max_i32(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

__global__ __launch_bounds__(256) void k_tag_root(const int32_t* __restrict__ parent, const int32_t* __restrict__ family, int64_t n_groups, int32_t* __restrict__ root,
                                                  TagMergeCounters* __restrict__ ctr)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = g < n_groups;
    int64_t r = g;
    int depth = 0;
    bool ended = true;
    if (active) {
        ended = tag_root(parent, n_groups, g, &r, &depth);
        root[g] = (int32_t)r;
    }
    const bool absorbed = active && ended && depth > 0;
    const int n_absorbed = __popcll(__ballot(absorbed));
    const int n_unended = __popcll(__ballot(!ended));
    const unsigned long long moved = wave_sum_u64(absorbed ? (unsigned long long)family[g] : 0ull);
    const int deepest = wave_max_i32(ended ? depth : 0);
    if ((threadIdx.x & 63) == 0) {
        if (n_absorbed) { atomicAdd(&ctr->absorbed, (unsigned long long)n_absorbed); atomicAdd(&ctr->moved_pairs, moved); }
        if (deepest) atomicMax(&ctr->max_depth, (unsigned long long)deepest);
        if (n_unended) atomicAdd(&ctr->unended, (unsigned long long)n_unended);
    }
}

// keys_sorted / ids_sorted [0, n_pairs): the sorted pairs, the n_members member keys in front; group_keys [0, n_groups): their runs
__global__ __launch_bounds__(256) void k_tag_rewrite(const uint64_t* __restrict__ keys_sorted, const uint32_t* __restrict__ ids_sorted, int64_t n_pairs, int64_t n_members,
                                                     const uint64_t* __restrict__ group_keys, int64_t n_groups, const int32_t* __restrict__ root,
                                                     uint64_t* __restrict__ keys, uint32_t* __restrict__ ids)
{
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_pairs) return;
    uint64_t key = keys_sorted[m];
    if (m < n_members) {
        const int64_t g = tag_lower_bound(group_keys, 0, n_groups, key);
        if (g < n_groups && group_keys[g] == key) key = group_keys[root[g]];            // (every member key is a group key: the test keeps a bad list inside the arrays)
    }
    keys[m] = key;
    ids[m] = ids_sorted[m];
}

extern "C" {

hipError_t mipgen_launch_tag_parent(hipStream_t st, const uint64_t* keys, const int32_t* family, int64_t n_groups, int tag_bases, int32_t* parent)
{
    if (n_groups <= 0) return hipSuccess;
    if (n_groups > 0x7fffffff || tag_bases < 1 || tag_bases > READS_MAX_TAG) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tag_parent, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, keys, family, n_groups, tag_bases, parent);
    return hipGetLastError();
}

// ctr: zero on entry
hipError_t mipgen_launch_tag_root(hipStream_t st, const int32_t* parent, const int32_t* family, int64_t n_groups, int32_t* root, TagMergeCounters* ctr)
{
    if (n_groups <= 0) return hipSuccess;
    if (n_groups > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tag_root, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, parent, family, n_groups, root, ctr);
    return hipGetLastError();
}

hipError_t mipgen_launch_tag_rewrite(hipStream_t st, const uint64_t* keys_sorted, const uint32_t* ids_sorted, int64_t n_pairs, int64_t n_members, const uint64_t* group_keys,
                                     int64_t n_groups, const int32_t* root, uint64_t* keys, uint32_t* ids)
{
    if (n_pairs <= 0) return hipSuccess;
    if (n_pairs > 0x7fffffff || n_members > n_pairs || n_groups > n_members) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tag_rewrite, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, keys_sorted, ids_sorted, n_pairs, n_members, group_keys, n_groups, root, keys, ids);
    return hipGetLastError();
}

}
