// kernels_reads.hip — reads and unique tags per probe from smMIP read pairs.
//
//  k_read_assign      a LANE per read pair.  Bound: the read bytes streamed from HBM once (a pair touches the cache lines of its first tag + arm
//                     bases only; the lines are fetched whole) plus two dependent hash probes and one 64-byte probe record per candidate, all of
//                     which sit in L2 / Infinity Cache for tables of 10^4-10^5 probes; 4 + 8 bytes written per pair.  A pair's work is two lookups
//                     and a handful of popcounts with nothing to share between lanes: a wavefront per pair would leave 62 lanes idle through the
//                     lookups and spend cross-lane reductions on a 16-30 base compare that one lane does in three instructions on bit planes.
//                     With `row` (the sample row of every pair) a count goes to the cell row * n_probes + probe instead of the probe.
//  k_sample_assign    a LANE per pair: the first J bases of the index read packed as a key, one lookup in the barcode hash (four at an index with
//                     one byte that is not A C G T), the pairs of every row counted in LDS and flushed once per workgroup.
//  k_reads_histogram  a lane per key of the sorted, duplicate-free key list: unique tags per probe (one atomic per distinct key).
//  sort + unique      hipCUB (rocPRIM) radix sort and run-length unique on the accumulated 64-bit keys (probe << 32 | tag).
#include <hipcub/hipcub.hpp>

#include "kernels.h"

// up to 64 bases of `b` from byte `from`, n of them (n <= 64), as bit planes; the bytes are fetched as aligned 32-bit words (the buffer is padded
// to a multiple of 4 bytes beyond its end, accel_reads.hip).  Positions >= n are marked bad.
__device__ static inline void pack_bases(const uint8_t* __restrict__ b, int64_t from, int n, uint64_t& p0, uint64_t& p1, uint64_t& bad)
{
    p0 = 0; p1 = 0; bad = ~reads_len_mask(n);
    if (n <= 0) return;
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(b) + (from >> 2);
    const int sh = (int)(from & 3);
    const int nw = (sh + n + 3) >> 2;                                    // <= 17 words
    int i = -sh;
    for (int k = 0; k < nw; k++, i += 4) {
        const uint32_t v = w[k];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int idx = i + j;
            if (idx < 0 || idx >= n) continue;
            const uint32_t c = reads_base_code((v >> (8 * j)) & 255u);
            p0 |= (uint64_t)(c & 1u) << idx;
            p1 |= (uint64_t)((c >> 1) & 1u) << idx;
            bad |= (uint64_t)(c >> 2) << idx;
        }
    }
}

// the probes whose seed is `key`: [*a, *b) of T.probes (empty when the key is in no probe)
__device__ static inline void seed_lookup(const SeedTable& T, uint64_t key, uint32_t* a, uint32_t* b)
{
    *a = 0; *b = 0;
    uint32_t s = reads_hash(key) & T.mask;
    for (uint32_t step = 0; step <= T.mask; step++, s = (s + 1) & T.mask) {
        const uint32_t slot = T.slots[s];
        if (slot == 0u) return;
        if (T.keys[slot - 1] == key) { *a = T.start[slot - 1]; *b = T.start[slot]; return; }
    }
}

__device__ static inline int wave_count(bool pred) { return __popcll(__ballot(pred)); }

__global__ __launch_bounds__(256) void k_read_assign(ReadsParams P, const ReadProbe* __restrict__ probes, SeedTable TE, SeedTable TL, int64_t pair0, int64_t n_pairs,
                                                     const uint8_t* __restrict__ ext_bytes, const int64_t* __restrict__ ext_off, int64_t ext_base,
                                                     const uint8_t* __restrict__ lig_bytes, const int64_t* __restrict__ lig_off, int64_t lig_base,
                                                     int32_t* __restrict__ assign, unsigned long long* __restrict__ reads, uint64_t* __restrict__ keys,
                                                     unsigned long long key_cap, ReadsCounters* __restrict__ ctr, const int32_t* __restrict__ row)
{
    const int64_t i = pair0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < pair0 + n_pairs;
    int result = READS_UNASSIGNED;
    bool tag_clean = false;
    uint32_t tag = 0, cell = 0;
    if (active) {
        const int64_t eb = ext_off[i] - ext_base, ee = ext_off[i + 1] - ext_base;
        const int64_t lb = lig_off[i] - lig_base, le = lig_off[i + 1] - lig_base;
        const int avail_e = (int)min((int64_t)64, max((int64_t)0, ee - eb - P.te));        // bases after the tag, as far as an arm can reach
        const int avail_l = (int)min((int64_t)64, max((int64_t)0, le - lb - P.tl));
        uint64_t x0, x1, xbad, y0, y1, ybad;
        pack_bases(ext_bytes, eb + P.te, avail_e, x0, x1, xbad);
        pack_bases(lig_bytes, lb + P.tl, avail_l, y0, y1, ybad);
        // the two seed lookups
        const bool e_seed = avail_e >= P.S && (xbad & P.seed_mask) == 0;
        const bool l_seed = avail_l >= P.S && (ybad & P.seed_mask) == 0;
        const uint64_t ekey = reads_seed_key(x0, x1, P.seed_mask), lkey = reads_seed_key(y0, y1, P.seed_mask);
        uint32_t ea = 0, eb_ = 0, la = 0, lb_ = 0;
        if (e_seed) seed_lookup(TE, ekey, &ea, &eb_);
        if (l_seed) seed_lookup(TL, lkey, &la, &lb_);
        if ((eb_ - ea) + (lb_ - la) > (uint32_t)READS_MAX_CAND) result = READS_OVERFLOW;
        else {
            int best = 1 << 30, best_p = -1, ties = 0;
            for (int side = 0; side < 2; side++) {
                const uint32_t a = side ? la : ea, b = side ? lb_ : eb_;
                const int32_t* __restrict__ list = side ? TL.probes : TE.probes;
                for (uint32_t c = a; c < b; c++) {
                    const int p = list[c];
                    const ReadProbe q = probes[p];
                    // the union of the two ranges: a probe of the ligation range whose extension seed is the read's was met in the extension range
                    if (side && eb_ > ea && (q.ebad & P.seed_mask) == 0 && reads_seed_key(q.e0, q.e1, P.seed_mask) == ekey) continue;
                    if (avail_e < q.e_len || avail_l < q.l_len) continue;                  // a read shorter than tag + arm fails
                    const int me = __popcll(((x0 ^ q.e0) | (x1 ^ q.e1) | xbad | q.ebad) & reads_len_mask(q.e_len));
                    const int ml = __popcll(((y0 ^ q.l0) | (y1 ^ q.l1) | ybad | q.lbad) & reads_len_mask(q.l_len));
                    if (me > P.m || ml > P.m) continue;
                    const int tot = me + ml;
                    if (tot < best) { best = tot; best_p = p; ties = 1; }
                    else if (tot == best) ties++;
                }
            }
            if (ties == 1) result = best_p;
            else if (ties > 1) result = READS_AMBIGUOUS;
        }
        if (result >= 0) {
            tag_clean = pack_tag(ext_bytes, eb, P.te, &tag);                               // (an assigned pair's reads hold their tags: avail >= arm >= 1)
            tag_clean = pack_tag(lig_bytes, lb, P.tl, &tag) && tag_clean;
            cell = row ? (uint32_t)row[i] * (uint32_t)P.n_probes + (uint32_t)result : (uint32_t)result;       // (rows * probes <= 2^32: accel_reads.hip)
            atomicAdd(&reads[cell], 1ull);
        }
        assign[i] = result;
    }
    // totals: one atomic per wavefront and counter
    const int lane = threadIdx.x & 63;
    const int n_act = wave_count(active), n_asg = wave_count(active && result >= 0), n_amb = wave_count(active && result == READS_AMBIGUOUS);
    const int n_un = wave_count(active && result == READS_UNASSIGNED), n_ov = wave_count(active && result == READS_OVERFLOW);
    const int n_tn = wave_count(active && result >= 0 && !tag_clean);
    // keys of the assigned pairs with a clean tag, appended: one atomic per wavefront reserves the slots (with no tag bases there is one key per
    // probe and nothing to count: unique_tags is `reads` then, and no key is written)
    const bool has_key = active && result >= 0 && tag_clean && (P.te + P.tl) > 0;
    const unsigned long long mask = __ballot(has_key);
    unsigned long long base = 0;
    if (lane == 0) {
        if (n_act) atomicAdd(&ctr->pairs, (unsigned long long)n_act);
        if (n_asg) atomicAdd(&ctr->assigned, (unsigned long long)n_asg);
        if (n_amb) atomicAdd(&ctr->ambiguous, (unsigned long long)n_amb);
        if (n_un) atomicAdd(&ctr->unassigned, (unsigned long long)n_un);
        if (n_ov) atomicAdd(&ctr->overflow, (unsigned long long)n_ov);
        if (n_tn) atomicAdd(&ctr->tag_n, (unsigned long long)n_tn);
        if (mask) base = atomicAdd(&ctr->n_keys, (unsigned long long)__popcll(mask));
    }
    base = __shfl(base, 0);
    if (has_key) {
        const unsigned long long pos = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
        if (pos < key_cap) keys[pos] = ((uint64_t)cell << 32) | tag;
        else atomicAdd(&ctr->keys_lost, 1ull);              // (the host sizes the buffer for every pair of the launch: never taken, and reported if it is)
    }
}

// the sample of `key` in the barcode hash: the slot's kind (SAMPLE_SLOT_EMPTY: not there) and its sample
__device__ static inline uint32_t sample_lookup(const SampleTable& T, uint64_t key, int32_t* sample)
{
    uint32_t s = reads_hash(key) & T.mask;
    for (uint32_t step = 0; step <= T.mask; step++, s = (s + 1) & T.mask) {
        const SampleSlot e = T.slots[s];                                    // one 16-byte load
        if (e.kind == SAMPLE_SLOT_EMPTY) return SAMPLE_SLOT_EMPTY;
        if (e.key == key) { *sample = e.sample; return e.kind; }
    }
    return SAMPLE_SLOT_EMPTY;
}

// DESIGN 4.10.  Pairs [0, n_pairs) of the uploaded chunk, grid-stride: row[i] (sample, or n_samples = undetermined) and sample_index[i] (>= 0, -1 none,
// -2 ambiguous).  The pairs of a sample row are counted in LDS when `lds_rows` > 0 (= rows, the dynamic LDS of the launch) and flushed with one atomic per
// row the workgroup met; none / ambiguous (and so the undetermined row) by ballot, one atomic per wavefront and counter.
__global__ __launch_bounds__(256) void k_sample_assign(SampleTable T, int64_t n_pairs, const uint8_t* __restrict__ idx_bytes, const int64_t* __restrict__ idx_off,
                                                       int64_t idx_base, int32_t* __restrict__ row, int32_t* __restrict__ sample_index,
                                                       unsigned long long* __restrict__ row_pairs, SampleCounters* __restrict__ sctr, int lds_rows)
{
    extern __shared__ uint32_t row_count[];
    for (int r = threadIdx.x; r < lds_rows; r += blockDim.x) row_count[r] = 0u;
    __syncthreads();
    const uint64_t jmask = reads_len_mask(T.J);
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // (every lane of a wavefront runs the same number of rounds: the ballots below are whole)
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n_pairs; i0 += stride) {
        const int64_t i = i0 + threadIdx.x;
        const bool active = i < n_pairs;
        int32_t sample = SAMPLE_NONE;
        if (active) {
            const int64_t b = idx_off[i] - idx_base, e = idx_off[i + 1] - idx_base;
            if (e - b >= T.J) {
                uint64_t p0, p1, bad;
                pack_bases(idx_bytes, b, T.J, p0, p1, bad);
                bad &= jmask;
                if (bad == 0) {
                    int32_t v = 0;
                    if (sample_lookup(T, reads_seed_key(p0, p1, jmask), &v) != SAMPLE_SLOT_EMPTY) sample = v;
                } else if (T.d == 1 && (bad & (bad - 1)) == 0) {
                    // one byte that is not A C G T: every barcode is at distance >= 1, and one at distance 1 equals the index with one of the four
                    // bases in that place
                    const uint64_t bit = bad;
                    int hits = 0;
                    for (uint32_t c = 0; c < 4; c++) {
                        const uint64_t q0 = (p0 & ~bit) | ((c & 1u) ? bit : 0ull), q1 = (p1 & ~bit) | ((c & 2u) ? bit : 0ull);
                        int32_t v = 0;
                        if (sample_lookup(T, reads_seed_key(q0, q1, jmask), &v) == SAMPLE_SLOT_EXACT) { hits++; sample = v; }
                    }
                    if (hits > 1) sample = SAMPLE_AMBIGUOUS;
                }
            }
            row[i] = sample >= 0 ? sample : T.n_samples;
            sample_index[i] = sample;
            if (sample >= 0) {
                if (lds_rows > 0) atomicAdd(&row_count[sample], 1u);
                else atomicAdd(&row_pairs[sample], 1ull);
            }
        }
        const int n_none = wave_count(active && sample == SAMPLE_NONE), n_amb = wave_count(active && sample == SAMPLE_AMBIGUOUS);
        if (lane == 0) {
            if (n_none) atomicAdd(&sctr->none, (unsigned long long)n_none);
            if (n_amb) atomicAdd(&sctr->ambiguous, (unsigned long long)n_amb);
            if (n_none + n_amb) atomicAdd(&row_pairs[T.n_samples], (unsigned long long)(n_none + n_amb));
        }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < lds_rows; r += blockDim.x) {
        const uint32_t c = row_count[r];
        if (c) atomicAdd(&row_pairs[r], (unsigned long long)c);
    }
}

// keys[0, n): sorted and duplicate-free - one count per key into its probe (its cell, with sample rows)
__global__ __launch_bounds__(256) void k_reads_histogram(const uint64_t* __restrict__ keys, int64_t n, unsigned long long* __restrict__ unique)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) atomicAdd(&unique[keys[i] >> 32], 1ull);
}

extern "C" {

hipError_t mipgen_launch_read_assign(hipStream_t s, const ReadsParams* P, const ReadProbe* probes, const SeedTable* TE, const SeedTable* TL, int64_t pair0, int64_t n_pairs,
                                     const uint8_t* ext_bytes, const int64_t* ext_off, int64_t ext_base, const uint8_t* lig_bytes, const int64_t* lig_off, int64_t lig_base,
                                     int32_t* assign, unsigned long long* reads, uint64_t* keys, int64_t key_cap, ReadsCounters* ctr, const int32_t* row)
{
    if (n_pairs <= 0) return hipSuccess;
    const int64_t blocks = (n_pairs + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_read_assign, dim3((unsigned)blocks), dim3(256), 0, s, *P, probes, *TE, *TL, pair0, n_pairs, ext_bytes, ext_off, ext_base, lig_bytes, lig_off,
                       lig_base, assign, reads, keys, (unsigned long long)key_cap, ctr, row);
    return hipGetLastError();
}

hipError_t mipgen_launch_sample_assign(hipStream_t s, const SampleTable* T, int64_t n_pairs, const uint8_t* idx_bytes, const int64_t* idx_off, int64_t idx_base, int32_t* row,
                                       int32_t* sample_index, unsigned long long* row_pairs, SampleCounters* sctr)
{
    if (n_pairs <= 0) return hipSuccess;
    // at most 2,048 workgroups (8 per CU), each with pairs enough to be worth the clearing and the flush of its LDS counters
    const int64_t blocks = std::min<int64_t>((n_pairs + 255) / 256, 2048);
    const int lds_rows = T->n_samples <= SAMPLES_LDS_ROWS ? T->n_samples : 0;
    hipLaunchKernelGGL(k_sample_assign, dim3((unsigned)blocks), dim3(256), (size_t)lds_rows * sizeof(uint32_t), s, *T, n_pairs, idx_bytes, idx_off, idx_base, row, sample_index,
                       row_pairs, sctr, lds_rows);
    return hipGetLastError();
}

hipError_t mipgen_launch_reads_histogram(hipStream_t s, const uint64_t* keys, int64_t n, unsigned long long* unique)
{
    if (n <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(k_reads_histogram, dim3((unsigned)blocks), dim3(256), 0, s, keys, n, unique);
    return hipGetLastError();
}

// keys[0, n) -> sorted and duplicate-free in keys[0, *n_out), through `alt` (n entries); temp == nullptr: the scratch size of both steps
hipError_t mipgen_reads_sort_unique(hipStream_t s, void* temp, size_t* temp_bytes, uint64_t* keys, uint64_t* alt, int64_t n, int end_bit, unsigned long long* n_out)
{
    if (n > 0x7fffffff) return hipErrorInvalidValue;
    size_t a = 0, b = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, a, keys, alt, (int)n, 0, end_bit, s);
    if (e != hipSuccess) return e;
    e = hipcub::DeviceSelect::Unique(nullptr, b, alt, keys, n_out, (int)n, s);
    if (e != hipSuccess) return e;
    const size_t need = std::max(a, b);
    if (!temp) { *temp_bytes = need; return hipSuccess; }
    if (*temp_bytes < need) return hipErrorInvalidValue;
    size_t t = *temp_bytes;
    e = hipcub::DeviceRadixSort::SortKeys(temp, t, keys, alt, (int)n, 0, end_bit, s);
    if (e != hipSuccess) return e;
    t = *temp_bytes;
    return hipcub::DeviceSelect::Unique(temp, t, alt, keys, n_out, (int)n, s);
}

}
