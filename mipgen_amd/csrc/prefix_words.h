// prefix_words.h — the front of the two dense logistic kernels (k_records_logistic: kernels_logistic.hip, k_logistic_dense: kernels_logistic_dense.hip):
// the bases a tile can touch staged in LDS and turned into packed 16-bit prefix counts, three u64 words per base, so that every window statistic of a
// candidate - base counts, guard, masked N, SNP counts, GC/AT class switches - is two ds_read_b64 and a subtract.  The two kernels must produce
// bit-identical records: both take the words, their fill and the window counts from here.
//
//  W0: A | C<<16 | G<<32 | bad (N or '-')<<48
//  W1: masked N | snp_any<<16 | snp_bad<<32 | snp_ok<<48
//  W2: GC/AT class switch against the base before | not ACGT<<16
// A field holds the count over the tile's bases: the tiles stay far below 65,536 of them.
#pragma once
#include <hip/hip_runtime.h>
#include "device_utils.h"
#include "logistic_device.h"
#include "mip_record.h"

#define PW_SCRATCH 48                // u64 words of scan scratch (block_exclusive_scan3_u64)

// the arrays in LDS: span + 1 words each (slot span holds the totals), the scratch behind them; sb (span base bytes) is placed by the kernel
struct PrefixWords {
    uint64_t *W0, *W1, *W2, *scratch;
    uint8_t* sb;
};

// u64 words of W0..W2 and the scratch for span bases (host and device: the kernels' LDS sizing)
__host__ __device__ constexpr size_t prefix_words_u64(int span) { return (size_t)3 * (span + 1) + PW_SCRATCH; }

__device__ __forceinline__ PrefixWords prefix_words_carve(unsigned char* smem, int span)
{
    PrefixWords W;
    W.W0 = (uint64_t*)smem; W.W1 = W.W0 + (span + 1); W.W2 = W.W1 + (span + 1); W.scratch = W.W2 + (span + 1);
    W.sb = nullptr;
    return W;
}

// the indicator words of one base from its byte b and the code cp of the base before it (its own code where there is none: no switch)
struct BaseWords { uint64_t w0, w1, w2; };
__device__ __forceinline__ BaseWords base_words(uint8_t b, int cp)
{
    const int c = b & BASE_CODE_MASK, snp = (b >> BASE_SNP_SHIFT) & 3;
    const int sw = ((c == BASE_G || c == BASE_C) != (cp == BASE_G || cp == BASE_C));
    BaseWords w;
    w.w0 = (uint64_t)(c == BASE_A) | ((uint64_t)(c == BASE_C) << 16) | ((uint64_t)(c == BASE_G) << 32) | ((uint64_t)(c == BASE_N || c == BASE_DASH) << 48);
    w.w1 = (uint64_t)((b & BASE_MASKED_BIT) != 0) | ((uint64_t)(snp != 0) << 16) | ((uint64_t)(snp == 2) << 32) | ((uint64_t)(snp == 1) << 48);
    w.w2 = (uint64_t)sw | ((uint64_t)(c >= 4) << 16);
    return w;
}

// Stages the bases [lo, lo + span) of the region (BASE_OTHER outside it), fills the words and scans them in place: W*[i] = the counts over the bases
// before i.  All NT threads of the workgroup call; whatever they wrote to LDS before the call is visible to all of them after it.
template <int NT>
__device__ __forceinline__ void prefix_words_build(const PrefixWords& W, const DevRegion& R, const uint8_t* __restrict__ bases, int lo, int span)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < span; i += NT) W.sb[i] = region_base(R, bases, lo + i);
    __syncthreads();
    for (int i = tid; i < span; i += NT) {
        const uint8_t b = W.sb[i];
        const BaseWords w = base_words(b, (i > 0 ? W.sb[i - 1] : b) & BASE_CODE_MASK);
        W.W0[i] = w.w0; W.W1[i] = w.w1; W.W2[i] = w.w2;
    }
    __syncthreads();
    block_exclusive_scan3_u64(W.W0, W.W1, W.W2, span, W.scratch);
}

// the counts of the arm window [s, s + len) (tile-local, genome order): T = len - A - C - G - (what is not ACGT, e.g. IUPAC codes, which count as nothing)
struct ArmCounts { uint32_t nA, nC, nG, nT, bad, other, masked, snp_any, snp_bad, snp_ok; };
__device__ __forceinline__ ArmCounts arm_window(const PrefixWords& W, int s, int len)
{
    const uint64_t d0 = W.W0[s + len] - W.W0[s], d1 = W.W1[s + len] - W.W1[s], d2 = W.W2[s + len] - W.W2[s];
    ArmCounts c;
    c.nA = f16(d0, 0); c.nC = f16(d0, 1); c.nG = f16(d0, 2); c.bad = f16(d0, 3); c.other = f16(d2, 1);
    c.nT = (uint32_t)len - c.nA - c.nC - c.nG - c.other;
    c.masked = f16(d1, 0); c.snp_any = f16(d1, 1); c.snp_bad = f16(d1, 2); c.snp_ok = f16(d1, 3);
    return c;
}

// the counts of the insert window [bi, bi + ss), ss > 0, and run = 1 + its GC/AT class switches on the strand-oriented insert (SVMipv4.cpp:118-142): from
// the switch prefix where every base is ACGT (a switch needs the base before it: those of bases bi + 1 .. bi + ss - 1), by the walk otherwise
struct InsertCounts { uint32_t nA, nC, nG, nT, other; int run; };
__device__ __forceinline__ InsertCounts insert_window(const PrefixWords& W, int bi, int ss, bool minus)
{
    const uint64_t t0 = W.W0[bi + ss] - W.W0[bi], t2 = W.W2[bi + ss] - W.W2[bi];
    InsertCounts t;
    t.nA = f16(t0, 0); t.nC = f16(t0, 1); t.nG = f16(t0, 2); t.other = f16(t2, 1);
    t.nT = (uint32_t)ss - t.nA - t.nC - t.nG - t.other;
    if (t.other == 0) t.run = 1 + (int)(f16(W.W2[bi + ss], 0) - f16(W.W2[bi + 1], 0));
    else t.run = run_count_slow(W.sb, bi, ss, minus);
    return t;
}
