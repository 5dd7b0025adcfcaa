// kernels_insertion_call.hip — insertion alleles called against a background pooled over the sample rows.  The pool is sparse: a cross-sample join
// on the 64-bit allele key, built and looked up on the device.  The arithmetic is insertion_call_model.h's (and, through it, call_model.h's).
//
//  k_ins_pool_append   one launch per sample row over its finished insertions result (anchor table and allele records, still on the device).  Lane i adds the span of
//                      position i into S[i] - a lane owns its position: no atomic - and, when record i is not ambiguous, appends the entry (key, k if the row qualifies
//                      at the allele, n if it does not) to the session's entry list.  Slots: the rank of the lane among the wavefront's non-ambiguous records (ballot)
//                      plus one atomic per wavefront on the running entry count, as k_call_flag reserves its candidates.  The order inside a row is that of the
//                      atomics, so undefined; the sort fixes it.
//  (pool reduce)       the (key, entry index) pairs go through mipgen_consensus_sort, the sorted keys through mipgen_consensus_runs - the run keys ARE the pool's
//                      key array, ascending and distinct - and the run lengths through an exclusive scan.
//  k_ins_pool_reduce   a lane per run: the K and X of its entries added up.  A row's keys are distinct, so a run is at most as long as there are sample rows; the
//                      loads of a run are gathers through the sorted indices, a handful per lane.
//  k_ins_call_flag     a lane per allele record of the row being called.  Ambiguous records are skipped.  The lane reads the span of its anchor (n) and of the pool
//                      (S), finds its key in the pool's keys by one lower-bound search - log2(alleles) dependent loads, the first levels shared by the whole wavefront
//                      and so served from cache -, applies leave-one-out and the filters, counts `tested` and `too_deep` by ballot and reserves its candidate slot
//                      as k_call_flag does.  The candidate is a mipgen_call_record whose pos is the INDEX of the record in the row's ascending record array and whose
//                      allele is 0: k_call_tail, the sort and k_call_gather of kernels_call.hip then run unchanged and return the calls in record order, which is
//                      allele-key order.
//  k_ins_call_records  a lane per call: the gathered record joined with the allele record at its pos into the 40-byte output record.
// Every shuffle and ballot is reached by all lanes of the wavefront: a lane without work carries a zero flag and no lane returns before the last of them.  No LDS, no
// scratch, vector stores only.
#include "kernels.h"
#include "device_utils.h"
#include "insertion_call_model.h"

__global__ __launch_bounds__(256) void k_ins_pool_append(const int32_t* __restrict__ anchors, int64_t n_pos, const mipgen_insertion_record* __restrict__ records,
                                                         int64_t n_records, int32_t bg_max_ppm, int32_t* __restrict__ S, uint64_t* __restrict__ keys,
                                                         InsPoolSums* __restrict__ sums, uint32_t* __restrict__ ids, unsigned long long cap, InsPoolCounters* __restrict__ ctr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (i < n_pos) S[i] += anchors[i * INSERTION_COLUMNS];
    mipgen_insertion_record rec;
    rec.pos = 0; rec.length = 1; rec.count = 0; rec.bases = 0; rec.ambiguous = 1;
    if (i < n_records) rec = records[i];
    const bool mine = i < n_records && !rec.ambiguous && rec.pos >= 0 && rec.pos < n_pos;
    const unsigned long long flags = __ballot(mine);
    if (flags == 0) return;                                              // (wave-uniform)
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&ctr->entries, (unsigned long long)__popcll(flags));
    base = __shfl(base, 0);
    const unsigned long long slot = base + (unsigned long long)__popcll(flags & ((1ull << lane) - 1ull));
    if (!mine || slot >= cap) return;
    keys[slot] = ins_call_key(rec.pos, rec.length, rec.bases);
    sums[slot] = ins_pool_contribution(rec.count, anchors[rec.pos * INSERTION_COLUMNS], bg_max_ppm);
    ids[slot] = (uint32_t)slot;
}

__global__ __launch_bounds__(256) void k_ins_pool_reduce(const int32_t* __restrict__ run_counts, const uint32_t* __restrict__ run_start, const unsigned long long* __restrict__ n_runs,
                                                         int64_t n_entries, const uint32_t* __restrict__ ids_sorted, const InsPoolSums* __restrict__ entry_sums,
                                                         InsPoolSums* __restrict__ pool_sums)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_entries || (unsigned long long)r >= *n_runs) return;
    const int64_t a = run_start[r];
    int64_t b = a + run_counts[r];
    if (b > n_entries) b = n_entries;
    InsPoolSums s{0, 0};
    for (int64_t j = a; j < b; j++) {
        const InsPoolSums e = entry_sums[ids_sorted[j]];
        s.K += e.K; s.X += e.X;
    }
    pool_sums[r] = s;
}

// span[x * span_stride]: the span of anchor x of the row being called (stride 4: column 0 of its anchor table; 1: a plain array)
__global__ __launch_bounds__(256) void k_ins_call_flag(const mipgen_insertion_record* __restrict__ records, int64_t n_records, const int32_t* __restrict__ span, int span_stride,
                                                       int64_t n_pos, const uint64_t* __restrict__ pool_keys, const InsPoolSums* __restrict__ pool_sums, int64_t n_pool,
                                                       const int32_t* __restrict__ pool_span, int own_row_is_sample, CallModel P, mipgen_call_record* __restrict__ cand,
                                                       CallCounters* __restrict__ ctr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    mipgen_insertion_record rec;
    rec.pos = 0; rec.length = 1; rec.count = 0; rec.bases = 0; rec.ambiguous = 1;
    if (i < n_records) rec = records[i];
    const bool material = i < n_records && !rec.ambiguous && rec.pos >= 0 && rec.pos < n_pos;
    const int64_t k = rec.count, n = material ? span[rec.pos * span_stride] : 0;
    const bool deep = material && n > MIPGEN_CALL_MAX_DEPTH, tested = material && call_depth_tested(n, P);
    const int n_tested = __popcll(__ballot(tested)), n_deep = __popcll(__ballot(deep));
    if (lane == 0) {
        if (n_tested) atomicAdd(&ctr->tested, (unsigned long long)n_tested);
        if (n_deep) atomicAdd(&ctr->too_deep, (unsigned long long)n_deep);
    }
    int64_t K_o = 0, N_o = 0;
    bool is_cand = false;
    if (tested)
        is_cand = ins_call_cell(pool_keys, pool_sums, n_pool, ins_call_key(rec.pos, rec.length, rec.bases), k, n, pool_span[rec.pos], own_row_is_sample != 0, P, &K_o, &N_o);
    const unsigned long long flags = __ballot(is_cand);
    if (flags == 0) return;                                              // (wave-uniform)
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&ctr->candidates, (unsigned long long)__popcll(flags));
    base = __shfl(base, 0);
    if (!is_cand) return;
    const unsigned long long slot = base + (unsigned long long)__popcll(flags & ((1ull << lane) - 1ull));
    mipgen_call_record out;
    out.pos = i; out.allele = 0; out.depth = (int32_t)n; out.alt = (int32_t)k; out.bg_alt = (int32_t)K_o; out.bg_depth = (int32_t)N_o; out.q = -1;
    cand[slot] = out;                                                    // (slot < n_records: a record is one candidate at most)
}

__global__ __launch_bounds__(256) void k_ins_call_records(const mipgen_call_record* __restrict__ calls, int64_t n_calls, const mipgen_insertion_record* __restrict__ records,
                                                          int64_t n_records, mipgen_insertion_call_record* __restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_calls) return;
    const mipgen_call_record c = calls[j];
    if (c.pos < 0 || c.pos >= n_records) return;
    const mipgen_insertion_record a = records[c.pos];
    mipgen_insertion_call_record r;
    r.pos = a.pos; r.length = a.length; r.bases = a.bases; r.depth = c.depth; r.alt = c.alt; r.bg_alt = c.bg_alt; r.bg_depth = c.bg_depth; r.q = c.q; r.reserved = 0;
    out[j] = r;
}

extern "C" {

static inline unsigned ins_call_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

// one sample row into the pool: S[n_pos] += its spans; its non-ambiguous records appended to (keys, sums, ids)[ctr->entries ...), at most cap entries in all
hipError_t mipgen_launch_ins_pool_append(hipStream_t st, const int32_t* anchors, int64_t n_pos, const mipgen_insertion_record* records, int64_t n_records, int32_t bg_max_ppm,
                                         int32_t* S, uint64_t* keys, InsPoolSums* sums, uint32_t* ids, int64_t cap, InsPoolCounters* ctr)
{
    if (n_pos < 1 || n_pos > MIPGEN_CALL_MAX_POSITIONS || n_records < 0 || n_records > 0x7fffffff || cap < 0 || cap > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ins_pool_append, dim3(ins_call_grid(std::max(n_pos, n_records))), dim3(256), 0, st, anchors, n_pos, records, n_records, bg_max_ppm, S, keys, sums, ids,
                       (unsigned long long)cap, ctr);
    return hipGetLastError();
}

// the sums of the first min(*n_runs, n_entries) runs of the sorted entries
hipError_t mipgen_launch_ins_pool_reduce(hipStream_t st, const int32_t* run_counts, const uint32_t* run_start, const unsigned long long* n_runs, int64_t n_entries,
                                         const uint32_t* ids_sorted, const InsPoolSums* entry_sums, InsPoolSums* pool_sums)
{
    if (n_entries < 1 || n_entries > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ins_pool_reduce, dim3(ins_call_grid(n_entries)), dim3(256), 0, st, run_counts, run_start, n_runs, n_entries, ids_sorted, entry_sums, pool_sums);
    return hipGetLastError();
}

// cand: n_records records; ctr zero on entry
hipError_t mipgen_launch_ins_call_flag(hipStream_t st, const mipgen_insertion_record* records, int64_t n_records, const int32_t* span, int span_stride, int64_t n_pos,
                                       const uint64_t* pool_keys, const InsPoolSums* pool_sums, int64_t n_pool, const int32_t* pool_span, int own_row_is_sample,
                                       const CallModel& P, mipgen_call_record* cand, CallCounters* ctr)
{
    if (n_records < 1 || n_records > MIPGEN_CALL_MAX_POSITIONS || n_pos < 1 || n_pos > MIPGEN_CALL_MAX_POSITIONS || n_pool < 0 || (span_stride != 1 && span_stride != 4))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ins_call_flag, dim3(ins_call_grid(n_records)), dim3(256), 0, st, records, n_records, span, span_stride, n_pos, pool_keys, pool_sums, n_pool, pool_span,
                       own_row_is_sample, P, cand, ctr);
    return hipGetLastError();
}

hipError_t mipgen_launch_ins_call_records(hipStream_t st, const mipgen_call_record* calls, int64_t n_calls, const mipgen_insertion_record* records, int64_t n_records,
                                          mipgen_insertion_call_record* out)
{
    if (n_calls < 1 || n_calls > n_records) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ins_call_records, dim3(ins_call_grid(n_calls)), dim3(256), 0, st, calls, n_calls, records, n_records, out);
    return hipGetLastError();
}

}
