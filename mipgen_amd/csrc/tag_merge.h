// tag_merge.h — the one-substitution merge of molecular tags as __host__ __device__ functions: kernels_tag_merge.hip runs them a lane per raw
// group, tests/tag_merge_host.cpp runs them as a plain C++ program under the sanitizers.  The rule, on the sorted, duplicate-free keys (cell << 32 | tag code)
// of the raw groups and their family sizes:
//   neighbour of b        a key of the same cell whose tag code differs from b's in exactly one 2-bit field
//   eligible parent of b  a neighbour a with c_a >= 2 c_b - 1 and c_a > c_b
//   parent of b           the eligible parent of the largest count, of the smaller key among equals; none: b is a root
// Counts rise strictly along parent links, so the links form a forest and a chain has at most 31 links (c >= 2^(k-1) + 1 after k links, families below 2^31).
// Every function reads nothing but its arguments, so a plain C++ program can include this file without HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TAG_HD __host__ __device__ static inline
#define TAG_RESTRICT __restrict__
#else
#define TAG_HD static inline
#define TAG_RESTRICT
#endif

#define TAG_MERGE_MAX_LINKS 31       // links of the longest chain the rule can build; a walk that has not ended after them is reported, never continued
#define TAG_MERGE_ROOT (-1)          // parent of a root

// what the three kernels count: groups with a parent, the pairs of those groups, the links of the deepest chain, walks that did not end
struct TagMergeCounters { unsigned long long absorbed, moved_pairs, max_depth, unended; };

// the first index in [lo, hi) whose key is not below `key` (hi when there is none)
TAG_HD int64_t tag_lower_bound(const uint64_t* TAG_RESTRICT keys, int64_t lo, int64_t hi, uint64_t key)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

TAG_HD bool tag_eligible(int32_t c_parent, int32_t c_child)
{
    return (int64_t)c_parent >= 2 * (int64_t)c_child - 1 && c_parent > c_child;
}

// a beats the best so far (best < 0: there is none yet).  The keys are of one cell, so the smaller key is the smaller tag code.
TAG_HD bool tag_better(int32_t c_a, uint64_t key_a, int32_t c_best, uint64_t key_best, int64_t best)
{
    return best < 0 || c_a > c_best || (c_a == c_best && key_a < key_best);
}

// The parent of raw group g (TAG_MERGE_ROOT: none) among keys[0, n), L = tag bases (1..16).  The sort order does the look-up: the keys that share g's bits from
// 2i + 2 up are one run, the neighbours at tag position i lie inside it, and the runs nest - so the window starts as the cell's range (two searches of the whole
// array) and is narrowed position by position from the highest one down; a window that holds g alone ends the walk.  Whole 64-bit keys are compared: a code that
// exists in another cell only is not found, because the window never leaves the cell.
TAG_HD int64_t tag_parent(const uint64_t* TAG_RESTRICT keys, const int32_t* TAG_RESTRICT family, int64_t n, int64_t g, int L)
{
    const uint64_t k = keys[g];
    const int32_t c = family[g];
    const uint64_t cell_base = (k >> (2 * L)) << (2 * L);                      // (L = 16: the cell bits alone)
    int64_t lo = tag_lower_bound(keys, 0, g, cell_base);                       // (g itself is in the cell)
    int64_t hi = tag_lower_bound(keys, g + 1, n, cell_base + (1ull << (2 * L)));
    int64_t best = TAG_MERGE_ROOT;
    int32_t c_best = 0;
    uint64_t key_best = 0;
    for (int i = L - 1; i >= 0 && hi - lo > 1; i--) {
        for (uint64_t d = 1; d < 4; d++) {
            const uint64_t nb = k ^ (d << (2 * i));
            const int64_t j = tag_lower_bound(keys, lo, hi, nb);
            if (j < hi && keys[j] == nb) {
                const int32_t c_a = family[j];
                if (tag_eligible(c_a, c) && tag_better(c_a, nb, c_best, key_best, best)) { best = j; c_best = c_a; key_best = nb; }
            }
        }
        if (i) {                                                               // the keys that share g's field i too: the window of position i - 1
            const uint64_t base = (k >> (2 * i)) << (2 * i);
            lo = tag_lower_bound(keys, lo, g, base);
            hi = tag_lower_bound(keys, g + 1, hi, base + (1ull << (2 * i)));
        }
    }
    return best;
}

// The root of raw group g along parent[] and the links walked to it in *depth; false when the walk has not ended after TAG_MERGE_MAX_LINKS links (a state the
// rule cannot build: reported, never continued).  An index outside [0, n) ends the walk the same way.
TAG_HD bool tag_root(const int32_t* TAG_RESTRICT parent, int64_t n, int64_t g, int64_t* root, int* depth)
{
    int64_t at = g;
    int links = 0;
    for (;;) {
        const int64_t p = parent[at];
        if (p == TAG_MERGE_ROOT) { *root = at; *depth = links; return true; }
        if (p < 0 || p >= n || links == TAG_MERGE_MAX_LINKS) { *root = g; *depth = links; return false; }
        at = p; links++;
    }
}
