// kernels_call.hip — variant calls from a finished count table against a background pooled over the sample rows.  The arithmetic is call_model.h's;
// its accuracy argument stands at the head of that file.
//
//  k_call_pool   a lane per position: one row's finished table added into the pool, K[5] and N[5] int32 per position (40 bytes), per allele class under the
//                qualification rule.  One launch per sample row; a lane owns its position, so there is no atomic.  int32 suffices: a count is at most the groups of
//                a cell, the pool adds one cell's counts over the rows, and the groups of a session are fewer than 2^31.
//  k_call_flag   a lane per position: the row's counts (two 16-byte loads of a 32-byte gapped row; a 16-byte and a 4-byte load of a 20-byte ungapped row, which is
//                only 4-byte aligned), the 40 bytes of the pool and the ref byte; leave-one-out and the four integer filters per alt class.  Candidate slots: a
//                wavefront scan of the lanes' candidate counts and one atomic per wavefront, as k_pileup_partition reserves its; `tested` and `too_deep` by ballot.
//                A candidate is written as its record with q = -1.  The list holds 4 candidates per position at most.
//  k_call_tail   a QUARTER WAVEFRONT per candidate, lanes over the terms i = k + lane + 16 j.  Each term is exp(lt_i - lt_k), computed on its own.  Rounds run until
//                the SMALLEST term of the round - its last one, because the terms fall from k on (call_model.h), and an upper bound of every term still to come -
//                is below 2^-60 of the running sum, or the next round would start beyond n; the four xor steps 8, 4, 2, 1 stay inside the group of 16.  (Testing
//                the round's largest term instead would cost every candidate a second round: the first round holds term k = 1.)  The common candidate (k small, e about 1e-3) takes one round, the rare deep one near its mean
//                hundreds of terms in tens of rounds: no lane walks a sequential loop the others wait for.  The leader writes q, the sort key
//                (pos << 3 | allele for a call, the sentinel n_pos << 3 otherwise) and the slot; calls are counted by ballot.
//  k_call_gather the j-th smallest key's record to records[j], for j below the calls counted by k_call_tail.
// The order: slots come from atomics, so the list is in no fixed order; the (key, slot) pairs of ALL candidates go through the device radix sort the consensus path
// links (mipgen_consensus_sort), calls first in ascending (pos, allele), and the first `calls` records are gathered.  Keys of calls are distinct, so the bytes are the
// same from call to call.  No LDS, no scratch, vector stores only.
#include "kernels.h"
#include "device_utils.h"
#include "call_model.h"
#include "count_row.h"

__global__ __launch_bounds__(256) void k_call_pool(const int32_t* __restrict__ counts, int columns, int64_t n_pos, int32_t bg_max_ppm, int32_t* __restrict__ pool)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_pos) return;
    int32_t c[8];
    call_load_row(counts, columns, x, c);
    const int64_t n = call_depth(c, columns);
    int32_t* __restrict__ o = pool + x * 10;
#pragma unroll
    for (int a = 0; a < CALL_ALLELES; a++) {
        const int32_t k = call_allele_count(c, columns, a);
        if (call_qualifies(k, n, bg_max_ppm)) { o[a] += k; o[5 + a] += (int32_t)n; }
    }
}

__global__ __launch_bounds__(256) void k_call_flag(const int32_t* __restrict__ counts, int columns, const int32_t* __restrict__ pool, const uint8_t* __restrict__ ref,
                                                   int64_t n_pos, int own_row_is_sample, CallModel P, mipgen_call_record* __restrict__ cand, CallCounters* __restrict__ ctr)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = x < n_pos;
    int32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int r = -1;
    if (active) { call_load_row(counts, columns, x, c); r = call_ref_class(ref[x]); }
    const int64_t n = call_depth(c, columns);
    const bool deep = r >= 0 && n > MIPGEN_CALL_MAX_DEPTH, tested = r >= 0 && call_depth_tested(n, P);
    const int n_tested = __popcll(__ballot(tested)), n_deep = __popcll(__ballot(deep));
    if (lane == 0) {
        if (n_tested) atomicAdd(&ctr->tested, (unsigned long long)n_tested);
        if (n_deep) atomicAdd(&ctr->too_deep, (unsigned long long)n_deep);
    }
    uint32_t mask = 0;                                                   // the alt classes that are candidates
    int32_t Ko[CALL_ALLELES], No[CALL_ALLELES];
    if (tested) {
        const int alleles = call_alleles(columns);
#pragma unroll
        for (int a = 0; a < CALL_ALLELES; a++) {
            int64_t K_o, N_o;
            const int32_t k = call_allele_count(c, columns, a);
            call_leave_one_out(pool[x * 10 + a], pool[x * 10 + 5 + a], k, n, own_row_is_sample != 0, P.bg_max_ppm, &K_o, &N_o);
            Ko[a] = (int32_t)K_o; No[a] = (int32_t)N_o;
            if (a != r && a < alleles && call_candidate(k, n, K_o, N_o, P)) mask |= 1u << a;
        }
    }
    const uint32_t mine = (uint32_t)__popc(mask);
    const uint32_t incl = wave_inclusive_sum_u32(mine, lane), total = __shfl(incl, 63);
    if (total == 0) return;                                              // (wave-uniform)
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&ctr->candidates, (unsigned long long)total);
    base = __shfl(base, 0);
    unsigned long long slot = base + (incl - mine);
#pragma unroll
    for (int a = 0; a < CALL_ALLELES; a++)
        if (mask >> a & 1u) {
            mipgen_call_record rec;
            rec.pos = x; rec.allele = a; rec.depth = (int32_t)n; rec.alt = call_allele_count(c, columns, a); rec.bg_alt = Ko[a]; rec.bg_depth = No[a]; rec.q = -1;
            cand[slot++] = rec;
        }
}

__global__ __launch_bounds__(256) void k_call_tail(mipgen_call_record* __restrict__ cand, int64_t n_cand, int64_t n_pos, CallModel P, uint64_t* __restrict__ keys,
                                                   uint32_t* __restrict__ ids, CallCounters* __restrict__ ctr)
{
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int sub = threadIdx.x & 15;
    const bool active = g < n_cand;                                      // (uniform over the group of 16; the shuffles below are run by every lane of the wavefront)
    int64_t k = 1, n = 1, A = 1, B = 2;
    if (active) { const mipgen_call_record rec = cand[g]; k = rec.alt; n = rec.depth; A = (int64_t)rec.bg_alt + P.a0; B = (int64_t)rec.bg_depth + P.n0; }
    const CallTail T = call_tail_of(n, A, B);
    const double lt_k = call_log_term(T, k);
    double S = 0.0;
    bool more = active;
    for (int64_t i0 = k; __any(more); i0 += 16) {
        const int64_t i = i0 + sub;
        double t = more && i <= n ? exp(call_log_term(T, i) - lt_k) : 0.0;
        double least = t;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) { t += shfl_xor_f64(t, m); least = fmin(least, shfl_xor_f64(least, m)); }
        S += t;
        more = more && i0 + 16 <= n && !(least < S * 0x1p-60);
    }
    const int32_t q = active ? call_q_of(lt_k, S) : -1;
    const bool leader = active && sub == 0, call = leader && q >= P.min_q;
    if (leader) {
        cand[g].q = q;
        keys[g] = call ? ((uint64_t)cand[g].pos << 3 | (uint64_t)cand[g].allele) : (uint64_t)n_pos << 3;
        ids[g] = (uint32_t)g;
    }
    const int n_calls = __popcll(__ballot(call));
    if ((threadIdx.x & 63) == 0 && n_calls) atomicAdd(&ctr->calls, (unsigned long long)n_calls);
}

// lanes over the slots of the sorted list: the first ctr->calls of them are the calls (the count is read on the device: no host round trip between sort and gather)
__global__ __launch_bounds__(256) void k_call_gather(const mipgen_call_record* __restrict__ cand, const uint32_t* __restrict__ ids, int64_t n_cand,
                                                     const CallCounters* __restrict__ ctr, mipgen_call_record* __restrict__ records)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_cand && (unsigned long long)j < ctr->calls) records[j] = cand[ids[j]];
}

extern "C" {

static inline bool call_shape_ok(int columns, int64_t n_pos) { return (columns == 5 || columns == 8) && n_pos >= 1 && n_pos <= MIPGEN_CALL_MAX_POSITIONS; }

hipError_t mipgen_launch_call_pool(hipStream_t st, const int32_t* counts, int columns, int64_t n_pos, int32_t bg_max_ppm, int32_t* pool)
{
    if (!call_shape_ok(columns, n_pos)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_call_pool, dim3((unsigned)((n_pos + 255) / 256)), dim3(256), 0, st, counts, columns, n_pos, bg_max_ppm, pool);
    return hipGetLastError();
}

// cand: 4 n_pos records; ctr zero on entry
hipError_t mipgen_launch_call_flag(hipStream_t st, const int32_t* counts, int columns, const int32_t* pool, const uint8_t* ref, int64_t n_pos, int own_row_is_sample,
                                   const CallModel& P, mipgen_call_record* cand, CallCounters* ctr)
{
    if (!call_shape_ok(columns, n_pos)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_call_flag, dim3((unsigned)((n_pos + 255) / 256)), dim3(256), 0, st, counts, columns, pool, ref, n_pos, own_row_is_sample, P, cand, ctr);
    return hipGetLastError();
}

// q of cand[0, n_cand), keys / ids of the sort, ctr->calls
hipError_t mipgen_launch_call_tail(hipStream_t st, mipgen_call_record* cand, int64_t n_cand, int64_t n_pos, const CallModel& P, uint64_t* keys, uint32_t* ids, CallCounters* ctr)
{
    if (n_cand < 1 || n_cand > 4 * n_pos || n_pos > MIPGEN_CALL_MAX_POSITIONS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_call_tail, dim3((unsigned)((n_cand + 15) / 16)), dim3(256), 0, st, cand, n_cand, n_pos, P, keys, ids, ctr);
    return hipGetLastError();
}

hipError_t mipgen_launch_call_gather(hipStream_t st, const mipgen_call_record* cand, const uint32_t* ids, int64_t n_cand, const CallCounters* ctr, mipgen_call_record* records)
{
    if (n_cand < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_call_gather, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, st, cand, ids, n_cand, ctr, records);
    return hipGetLastError();
}

}
