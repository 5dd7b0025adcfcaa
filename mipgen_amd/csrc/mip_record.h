// mip_record.h — the integer record of design_mip and the bounds skips, as the device kernels restate them: one definition each.
//
// The record layout is the one the MIPGEN_REC_* accessors of include/mipgen_accel.h read; every builder packs it with pack_record, and every
// kernel that reads a region's base, looks an oligo's copy number up, tests the mapping flag, places a candidate's arms, orients the ligation
// junction, decides the bounds skips (mip_bounds.h: the rule and the forms the dense-grid kernels use) or applies the record's constant SVR
// scores does so through the functions below.  The one exception is k_svr_dense (kernels_svr.hip): its arm_entry keeps a copy lookup and a
// junction orientation of its own - the kernel sits at its register budget, and a call there changes its generated code.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include "device_utils.h"
#include "mip_bounds.h"

struct ArmStarts { int ext, lig; };

// arm starts of the candidate at scan start p with scan size ss: PlusSVMipv4.cpp:9-12 / MinusSVMipv4.cpp:32-35
__device__ __forceinline__ ArmStarts arm_starts(int p, int ss, int e, int l, bool minus)
{
    return minus ? ArmStarts{p + ss, p - l} : ArmStarts{p - e, p + ss};
}

// the bounds skips of mipgen.cpp:443-444, and a non-empty scan target: the candidate is constructed (MIPGEN_FLAG_VALID)
__device__ __forceinline__ bool constructed(const DevRegion& R, int p, int C, int e, int l) { return constructed(R.seq_stop, p, C, e, l); }

// the byte of the region's sequence at chromosome coordinate pos (common.h: code, masked bit, SNP class); BASE_OTHER outside it
__device__ __forceinline__ uint8_t region_base(const DevRegion& R, const uint8_t* bases, int pos)
{
    const int ri = pos - R.seq_start;
    return (ri >= 0 && ri < R.seq_len) ? bases[R.seq_off + ri] : (uint8_t)BASE_OTHER;
}

// copy number of the oligo [start, start + len), mipgen.cpp:612-613: absent key -> 0, no table -> 1
__device__ __forceinline__ int oligo_copy(const DevParams* P, const DevRegion& R, const int32_t* copy, int start, int len)
{
    if (R.copy_off < 0) return 1;
    const int slot = P->len_slot[len], ri = start - R.seq_start;
    return (slot >= 0 && ri >= 0 && ri < R.seq_len) ? copy[R.copy_off + (int64_t)slot * R.seq_len + ri] : 0;
}

// an arm's copy number from its record field: a 16-bit field saturates at 65535, where the reference keeps bwa's unbounded X0 count
// (mipgen.cpp:586-587): the true value comes from the copy table
__device__ __forceinline__ int true_arm_copy(const DevParams* P, const DevRegion& R, const int32_t* copy, int start, int len, uint32_t rec_field)
{
    if (rec_field != 65535u || R.copy_off < 0) return (int)rec_field;
    return oligo_copy(P, R, copy, start, len);
}

// mapping flag, mipgen.cpp:615-625: the unmappable-position table of capture size index k at the MIP's upstream arm.  mapping_tested: there is a
// table and the parameters consult it; unmapped_at: its entry for size index k at ms = start - seq_start, 0 <= ms < seq_len
__device__ __forceinline__ bool mapping_tested(const DevParams* P, const DevRegion& R) { return R.unmap_off >= 0 && P->check_copy_number; }
__device__ __forceinline__ bool unmapped_at(const DevRegion& R, const uint8_t* unmap, int k, int ms) { return unmap[R.unmap_off + (int64_t)k * R.seq_len + ms] != 0; }
__device__ __forceinline__ bool unmapped(const DevParams* P, const DevRegion& R, const uint8_t* unmap, int k, bool minus, int ext_start, int lig_start)
{
    if (!mapping_tested(P, R)) return false;
    const int ms = (minus ? lig_start : ext_start) - R.seq_start;
    return ms >= 0 && ms < R.seq_len && unmapped_at(R, unmap, k, ms);
}

// the record's flags, mipgen.cpp:610,626,690-693,759-760; snp_count is 0 where the mapping flag returns early (the masking and SNP fields keep
// their defaults)
__device__ __forceinline__ uint32_t record_flags(bool mapping, int masked_n, int arm_sum, double thr, int snp_any, int snp_bad, int snp_ok, bool guard,
                                                 int& snp_count)
{
    uint32_t flags = MIPGEN_FLAG_VALID | (guard ? MIPGEN_FLAG_GUARD : 0u);
    snp_count = 0;
    if (mapping) return flags | MIPGEN_FLAG_MAPPING;
    if ((double)masked_n / (double)arm_sum > thr) flags |= MIPGEN_FLAG_MASKING;
    snp_count = snp_any;
    if (snp_bad != 0 || snp_count > 1) flags |= MIPGEN_FLAG_SNP;
    if (snp_ok != 0) flags |= MIPGEN_FLAG_HAS_SNP_MIP;
    return flags;
}

// ligation junction = the first two bases of the oriented ligation arm, 4 * code + code (A < C < G < T); 255 if either is not ACGT
__device__ __forceinline__ uint32_t junction_code(int j0, int j1) { return (j0 < 4 && j1 < 4) ? (uint32_t)(4 * j0 + j1) : 255u; }

// ... of the ligation arm [start, start + len) of genome-order base bytes sb: on '-' the oriented arm is the reverse complement
__device__ __forceinline__ uint32_t lig_junction(const uint8_t* sb, int start, int len, bool minus)
{
    int j0, j1;
    if (!minus) { j0 = sb[start] & BASE_CODE_MASK; j1 = sb[start + 1] & BASE_CODE_MASK; }
    else { j0 = comp_code(sb[start + len - 1] & BASE_CODE_MASK); j1 = comp_code(sb[start + len - 2] & BASE_CODE_MASK); }
    return junction_code(j0, j1);
}

// the 64-bit record, fields as MIPGEN_REC_*: copy numbers saturate at 65535, the masked-base and SNP counts at 255
__device__ __forceinline__ uint64_t pack_record(int ext_copy, int lig_copy, int masked_n, int snp_count, uint32_t flags, uint32_t jc)
{
    const uint32_t ec = (uint32_t)min(max(ext_copy, 0), 65535), lc = (uint32_t)min(max(lig_copy, 0), 65535);
    return (uint64_t)ec | ((uint64_t)lc << 16) | ((uint64_t)min(masked_n, 255) << 32) | ((uint64_t)min(snp_count, 255) << 40) |
           ((uint64_t)flags << 48) | ((uint64_t)jc << 56);
}

// the record fixes the SVR score: the candidate is not constructed, an arm holds a guard base (the all-zero feature vector, SVMipv4.cpp:63-68)
// or an arm's copy number is 0 (log10(0) = -inf: every kernel value is 0)
__device__ __forceinline__ bool score_is_constant(uint64_t rec)
{
    const uint32_t flags = MIPGEN_REC_FLAGS(rec);
    return !(flags & MIPGEN_FLAG_VALID) || (flags & MIPGEN_FLAG_GUARD) || MIPGEN_REC_EXT_COPY(rec) == 0 || MIPGEN_REC_LIG_COPY(rec) == 0;
}

// ... and the score with those constants applied: 0, s_guard (the model at the all-zero vector), -rho; s where the record does not fix it
__device__ __forceinline__ double record_score(uint64_t rec, double s, double rho, double s_guard)
{
    const uint32_t flags = MIPGEN_REC_FLAGS(rec);
    if (!(flags & MIPGEN_FLAG_VALID)) return 0.0;
    if (flags & MIPGEN_FLAG_GUARD) return s_guard;
    if (MIPGEN_REC_EXT_COPY(rec) == 0 || MIPGEN_REC_LIG_COPY(rec) == 0) return -rho;
    return s;
}
