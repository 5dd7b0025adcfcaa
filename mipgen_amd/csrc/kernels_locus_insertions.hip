// kernels_locus_insertions.hip — the fold of a row's insertion alleles from template positions to genome loci, between the insertions call and the sparse pool or
// the insertion call.  The plan is the installed one of 4.15 (src, first); the anchor row a source pulls is the row k_locus_merge<8> takes columns 6
// and 7 from: row x - 1 under bit 1, row x with flags 0, none on a minus source without bit 1.
//
//  Once per installed plan:
//  k_locus_anchor_map    a lane per locus, a loop over its sources: own[a] = l << 2 | flags of the flags-0 source x = a, prev[a] = that of the bit-1 source x = a + 1
//                        (both GAP_LOCUS_NONE before the launch).  A plan holds each x once, so no two lanes write one element.
//  Once per row:
//  k_locus_ins_fold      a lane per allele record: own[pos] and prev[pos] looked up; for each hit the locus key (gap_locus_allele_key: the reverse complement under
//                        bit 0) and the record's index are appended.  Slots: the ranks of the lane among the wavefront's own-hits and prev-hits (two ballots) plus one
//                        atomic per wavefront on the running pair count, as k_ins_pool_append reserves its slots; 2 n_records pairs at most, so no count pass.  The
//                        order of the pairs is that of the atomics, so undefined; the sort fixes it.  Records no source pulls are counted by ballot.
//  (sort, runs, scan)    mipgen_consensus_sort over the 64 key bits, mipgen_consensus_runs - the run keys are the locus records' keys, ascending and distinct -, an
//                        exclusive scan of the run lengths.
//  k_locus_ins_reduce    a lane per run: the counts of its entries added through the sorted indices (two entries of one key are a handful at most: the sources of a
//                        locus) and the record written from the key's fields.  The shape of k_ins_pool_reduce.
//  k_locus_anchor_merge  a lane per locus, a loop over its sources: one 16-byte load per pulled anchor row, one 16-byte store; a lane owns its row, so no atomic and
//                        no zeroing pass.  The totals - loci with a non-zero row by ballot, the four column sums by wave_sum_i64 - are taken in the same pass: wave-uniform
//                        grid-stride rounds over at most 2,048 workgroups, as k_locus_sum, so that they cost one atomic per wavefront and counter of THOSE (a wavefront per
//                        64 loci would queue a million atomics on five addresses); a lane past n_loci carries a zero row and reaches every ballot and shuffle.
// Every ballot and shuffle is reached by all 64 lanes: a lane without work carries a zero flag.  No LDS, no scratch, vector stores only.
#include "kernels.h"
#include "device_utils.h"
#include "gapped_align.h"

__global__ __launch_bounds__(256) void k_locus_anchor_map(const uint32_t* __restrict__ src, const uint32_t* __restrict__ first, int64_t n_pos, int64_t n_loci,
                                                          uint32_t* __restrict__ own, uint32_t* __restrict__ prev)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_loci) return;
    uint32_t i1 = first[l + 1];
    if ((int64_t)i1 > n_pos) i1 = (uint32_t)n_pos;
    for (uint32_t i = first[l]; i < i1; i++) {
        const uint32_t s = src[i], flags = s & 3u, word = (uint32_t)l << 2 | flags;
        const int64_t x = (int64_t)(s >> 2);
        if (x >= n_pos) continue;
        if (flags & 2u) { if (x >= 1) prev[x - 1] = word; }                                  // (x >= 1: the host refuses bit 1 at x = 0)
        else if (flags == 0u) own[x] = word;
    }
}

__global__ __launch_bounds__(256) void k_locus_ins_fold(const mipgen_insertion_record* __restrict__ records, int64_t n_records, const uint32_t* __restrict__ own,
                                                        const uint32_t* __restrict__ prev, int64_t n_pos, uint64_t* __restrict__ keys, uint32_t* __restrict__ ids,
                                                        unsigned long long cap, LocusInsCounters* __restrict__ ctr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    mipgen_insertion_record rec;
    rec.pos = 0; rec.length = 1; rec.count = 0; rec.bases = 0; rec.ambiguous = 1;
    if (i < n_records) rec = records[i];
    const bool real = i < n_records && rec.pos >= 0 && rec.pos < n_pos;
    const uint32_t w_own = real ? own[rec.pos] : GAP_LOCUS_NONE, w_prev = real ? prev[rec.pos] : GAP_LOCUS_NONE;
    const bool hit_own = w_own != GAP_LOCUS_NONE, hit_prev = w_prev != GAP_LOCUS_NONE;
    const unsigned long long f_own = __ballot(hit_own), f_prev = __ballot(hit_prev), f_none = __ballot(real && !hit_own && !hit_prev);
    const unsigned long long n_own = (unsigned long long)__popcll(f_own), n_new = n_own + (unsigned long long)__popcll(f_prev);
    unsigned long long base = 0;
    if (lane == 0) {
        if (n_new) base = atomicAdd(&ctr->folded, n_new);
        if (f_none) atomicAdd(&ctr->dropped, (unsigned long long)__popcll(f_none));
    }
    base = __shfl(base, 0);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (hit_own) {
        const unsigned long long slot = base + (unsigned long long)__popcll(f_own & below);
        if (slot < cap) { keys[slot] = gap_locus_allele_key(w_own, rec.length, rec.ambiguous != 0, rec.bases); ids[slot] = (uint32_t)i; }
    }
    if (hit_prev) {
        const unsigned long long slot = base + n_own + (unsigned long long)__popcll(f_prev & below);
        if (slot < cap) { keys[slot] = gap_locus_allele_key(w_prev, rec.length, rec.ambiguous != 0, rec.bases); ids[slot] = (uint32_t)i; }
    }
}

__global__ __launch_bounds__(256) void k_locus_ins_reduce(const uint64_t* __restrict__ run_keys, const int32_t* __restrict__ run_counts, const uint32_t* __restrict__ run_start,
                                                          const unsigned long long* __restrict__ n_runs, int64_t n_pairs, const uint32_t* __restrict__ ids_sorted,
                                                          const mipgen_insertion_record* __restrict__ records, int64_t n_records, mipgen_insertion_record* __restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_pairs || (unsigned long long)r >= *n_runs) return;
    const int64_t a = run_start[r];
    int64_t b = a + run_counts[r];
    if (b > n_pairs) b = n_pairs;
    long long count = 0;
    for (int64_t j = a; j < b; j++) {
        const uint32_t id = ids_sorted[j];
        if ((int64_t)id < n_records) count += records[id].count;
    }
    const uint64_t key = run_keys[r];
    mipgen_insertion_record rec;
    rec.pos = gap_allele_pos(key); rec.length = gap_allele_length(key); rec.count = (int32_t)count; rec.bases = gap_allele_bases(key);
    rec.ambiguous = gap_allele_ambiguous(key) ? 1 : 0;
    out[r] = rec;
}

__global__ __launch_bounds__(256) void k_locus_anchor_merge(const int32_t* __restrict__ anchors, const uint32_t* __restrict__ src, const uint32_t* __restrict__ first,
                                                            int64_t n_pos, int64_t n_loci, int32_t* __restrict__ locus_anchors, LocusInsCounters* __restrict__ ctr)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) - lane, step = (int64_t)gridDim.x * blockDim.x;
    long long s0 = 0, s1 = 0, s2 = 0, s3 = 0, covered = 0;
    for (int64_t i0 = wave0; i0 < n_loci; i0 += step) {                                     // (wave-uniform rounds: every lane runs the ballot)
        const int64_t l = i0 + lane;
        int4 m = make_int4(0, 0, 0, 0);
        if (l < n_loci) {
            uint32_t i1 = first[l + 1];
            if ((int64_t)i1 > n_pos) i1 = (uint32_t)n_pos;
            for (uint32_t i = first[l]; i < i1; i++) {
                const uint32_t s = src[i], flags = s & 3u;
                const int64_t x = (int64_t)(s >> 2), row = (flags & 2u) ? x - 1 : flags == 0u ? x : -1;
                if (row < 0 || row >= n_pos) continue;
                const int4 a = *(const int4*)(anchors + row * INSERTION_COLUMNS);
                m.x += a.x; m.y += a.y; m.z += a.z; m.w += a.w;
            }
            *(int4*)(locus_anchors + l * INSERTION_COLUMNS) = m;
        }
        covered += __popcll(__ballot((m.x | m.y | m.z | m.w) != 0)) * (lane == 0);
        s0 += m.x; s1 += m.y; s2 += m.z; s3 += m.w;
    }
    s0 = wave_sum_i64(s0); s1 = wave_sum_i64(s1); s2 = wave_sum_i64(s2); s3 = wave_sum_i64(s3);
    if (lane == 0) {
        if (covered) atomicAdd(&ctr->loci, (unsigned long long)covered);
        if (s0) atomicAdd(&ctr->span, (unsigned long long)s0);
        if (s1) atomicAdd(&ctr->insertions, (unsigned long long)s1);
        if (s2) atomicAdd(&ctr->ins_discordant, (unsigned long long)s2);
        if (s3) atomicAdd(&ctr->ambiguous, (unsigned long long)s3);
    }
}

extern "C" {

static inline bool locus_ins_shape_ok(int64_t n_pos, int64_t n_loci) { return n_pos >= 1 && n_pos <= MIPGEN_CALL_MAX_POSITIONS && n_loci >= 1 && n_loci <= MIPGEN_CALL_MAX_POSITIONS; }
static inline unsigned locus_ins_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

// own[n_pos] and prev[n_pos] (both filled with GAP_LOCUS_NONE on entry) from the sources of an installed plan
hipError_t mipgen_launch_locus_anchor_map(hipStream_t st, const uint32_t* src, const uint32_t* first, int64_t n_pos, int64_t n_loci, uint32_t* own, uint32_t* prev)
{
    if (!locus_ins_shape_ok(n_pos, n_loci)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_locus_anchor_map, dim3(locus_ins_blocks(n_loci)), dim3(256), 0, st, src, first, n_pos, n_loci, own, prev);
    return hipGetLastError();
}

// the (locus key, record index) pairs of a row's records into (keys, ids)[ctr->folded ...), at most cap = 2 n_records; ctr zero on entry
hipError_t mipgen_launch_locus_ins_fold(hipStream_t st, const mipgen_insertion_record* records, int64_t n_records, const uint32_t* own, const uint32_t* prev, int64_t n_pos,
                                        uint64_t* keys, uint32_t* ids, int64_t cap, LocusInsCounters* ctr)
{
    if (n_records < 1 || n_records > 0x7fffffff || n_pos < 1 || n_pos > MIPGEN_CALL_MAX_POSITIONS || cap < 0 || cap > 2 * n_records) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_locus_ins_fold, dim3(locus_ins_blocks(n_records)), dim3(256), 0, st, records, n_records, own, prev, n_pos, keys, ids, (unsigned long long)cap, ctr);
    return hipGetLastError();
}

// the locus records of the first min(*n_runs, n_pairs) runs of the sorted pairs
hipError_t mipgen_launch_locus_ins_reduce(hipStream_t st, const uint64_t* run_keys, const int32_t* run_counts, const uint32_t* run_start, const unsigned long long* n_runs,
                                          int64_t n_pairs, const uint32_t* ids_sorted, const mipgen_insertion_record* records, int64_t n_records, mipgen_insertion_record* out)
{
    if (n_pairs < 1 || n_pairs > 0x7fffffff || n_records < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_locus_ins_reduce, dim3(locus_ins_blocks(n_pairs)), dim3(256), 0, st, run_keys, run_counts, run_start, n_runs, n_pairs, ids_sorted, records, n_records, out);
    return hipGetLastError();
}

// locus_anchors[n_loci][4] is written whole and summed into ctr (its five totals zero on entry)
hipError_t mipgen_launch_locus_anchor_merge(hipStream_t st, const int32_t* anchors, const uint32_t* src, const uint32_t* first, int64_t n_pos, int64_t n_loci,
                                            int32_t* locus_anchors, LocusInsCounters* ctr)
{
    if (!locus_ins_shape_ok(n_pos, n_loci)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_locus_anchor_merge, dim3(std::min(locus_ins_blocks(n_loci), 2048u)), dim3(256), 0, st, anchors, src, first, n_pos, n_loci, locus_anchors, ctr);
    return hipGetLastError();
}

}
