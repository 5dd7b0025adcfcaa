// insertion_call_model.h — the sparse background pool of DESIGN 4.17 as the pieces the kernels of kernels_insertion_call.hip are made of.  An insertion allele is
// the 64-bit key of gapped_align.h (position, length, bases); the pool holds one int32 S per position - the span of the anchor summed over ALL sample rows - and one
// entry {key, K, X} per distinct non-ambiguous allele of any sample row, keys strictly ascending: K the counts of the rows whose record of the allele qualifies, X the
// spans of the rows whose record does NOT.  Only a row that has the record can fail the qualification, so N = S - X; an allele no sample row carries has K = 0, N = S.
// The rules themselves - qualification, leave-one-out, the filters, the tail - are call_model.h's and are called, not restated.  Every piece is __host__ __device__
// and reads nothing but its arguments, so a plain C++ program can include this file without HIP (tests/insertion_call_host.cpp does, under the sanitizers).
//
// Integers.  k <= n <= the groups of a cell; K, X and S add one cell over the sample rows, so each is below 2^31 as the dense pool's sums are (call_model.h).
#pragma once
#include "call_model.h"
#include "gapped_align.h"

// one entry's sums beside its key: the pool keeps keys and sums in two arrays, so that the search strides over 8 bytes
struct InsPoolSums { int32_t K, X; };

// the key a non-ambiguous allele record is pooled and looked up under
CALL_HD uint64_t ins_call_key(int64_t pos, int length, uint32_t bases) { return gap_allele_key(pos, length, false, bases); }

// the first index whose key is not below `key` (n: none); keys[0, n) ascending
CALL_HD int64_t ins_pool_lower_bound(const uint64_t* keys, int64_t n, uint64_t key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the index of `key` in the pool, or -1: absent
CALL_HD int64_t ins_pool_find(const uint64_t* keys, int64_t n, uint64_t key)
{
    const int64_t at = ins_pool_lower_bound(keys, n, key);
    return at < n && keys[at] == key ? at : -1;
}

// entry -> (K, N) given S, the span of the key's position over all sample rows; at < 0: the allele is absent
CALL_HD void ins_pool_sums(const InsPoolSums* sums, int64_t at, int64_t S, int64_t* K, int64_t* N)
{
    *K = at < 0 ? 0 : sums[at].K;
    *N = at < 0 ? S : S - sums[at].X;
}

// what one sample row's record (k of n) adds to its allele's entry: k to K when the row qualifies there, else n to X
CALL_HD InsPoolSums ins_pool_contribution(int64_t k, int64_t n, int32_t bg_max_ppm)
{
    const bool q = call_qualifies(k, n, bg_max_ppm);
    return {q ? (int32_t)k : 0, q ? 0 : (int32_t)n};
}

// One tested record (k of n at `key`, S the pooled span of its position) against the pool: the background without the row being called, and whether the cell is a
// candidate.
CALL_HD bool ins_call_cell(const uint64_t* keys, const InsPoolSums* sums, int64_t n_pool, uint64_t key, int64_t k, int64_t n, int64_t S, bool own_row_is_sample,
                           const CallModel& P, int64_t* K_o, int64_t* N_o)
{
    int64_t K, N;
    ins_pool_sums(sums, ins_pool_find(keys, n_pool, key), S, &K, &N);
    call_leave_one_out(K, N, k, n, own_row_is_sample, P.bg_max_ppm, K_o, N_o);
    return call_candidate(k, n, *K_o, *N_o, P);
}
