// list_stage.h — the front of the list scorers (k_features_batch, k_candidates: kernels_misc.hip): how an entry of a list becomes oriented base codes
// in LDS and the integers of its record, one definition per SOURCE of the entry.  There are two sources (common.h):
//   BatchSrc  a candidate addressed by coordinates in the resident batch: strand orientation (reverse_comp, MinusSVMipv4.cpp:6-29), masked / SNP bits,
//             copy numbers, the mapping flag and the long-range row come from the batch's tables (design_mip, mipgen.cpp:606-760);
//   ProbeSrc  a probe given by its oriented sequences as a MIP table prints them (mipgen.cpp:765-794): no strand, no tables - copies and long-range row
//             come with the probe, the flags are VALID | GUARD only.
// list_entry(S, i) reads entry i of a launch; its two staging functions are all a kernel needs:
//   stage_arms    ONE wavefront (arms are at most MIPGEN_MAX_OLIGO = 64 bases, lane i on base i) writes the oriented arms and returns the integers;
//   stage_insert  nt cooperating threads write one piece of the oriented insert.
// Everything behind the staged codes - mer histogram, features (mip_features.h), record, scores - is the kernels' own, shared code.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include "device_utils.h"
#include "mip_record.h"
#include "mip_features.h"

// LDS writes of a wavefront visible to its own lanes: nothing in the list front is wider than this
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// what stage_arms hands back, the same in every lane: the record's integers, the guard of SVMipv4.cpp:63 and the ligation junction
struct ArmInts { int ext_copy, lig_copy, masked_n, snp_count, flags, guard, jc; };

struct BatchEntry {
    BatchSrc S;
    const DevRegion* R;
    int p, e, l, ss;               // scan start, arm lengths, scan size
    int C;
    bool minus, valid;             // valid: a function of the candidate alone - every thread of a workgroup decides it alike
    int64_t out;                   // where the entry's results go
    const double* lrc;

    __device__ __forceinline__ uint8_t base_at(int pos) const { return region_base(*R, S.bases, pos); }
    // lane i holds byte i of each arm in genome order; oriented codes (complement + reverse on '-') go to LDS, the record's counts over the arms'
    // bytes come from wave ballots
    __device__ __forceinline__ ArmInts stage_arms(uint8_t* s_ext, uint8_t* s_lig, int lane) const
    {
        const ArmStarts st = arm_starts(p, ss, e, l, minus);
        const bool in_e = lane < e, in_l = lane < l;
        const uint8_t raw_e = in_e ? base_at(st.ext + lane) : (uint8_t)0, raw_l = in_l ? base_at(st.lig + lane) : (uint8_t)0;
        const int code_e = raw_e & BASE_CODE_MASK, code_l = raw_l & BASE_CODE_MASK;
        if (in_e) s_ext[minus ? e - 1 - lane : lane] = (uint8_t)(minus ? comp_code(code_e) : code_e);
        if (in_l) s_lig[minus ? l - 1 - lane : lane] = (uint8_t)(minus ? comp_code(code_l) : code_l);
        auto cnt2 = [&](bool pe, bool pl) -> int { return __builtin_popcountll(__ballot(in_e && pe)) + __builtin_popcountll(__ballot(in_l && pl)); };
        const int snp_e = (raw_e >> BASE_SNP_SHIFT) & 3, snp_l = (raw_l >> BASE_SNP_SHIFT) & 3;
        const int masked_n = cnt2((raw_e & BASE_MASKED_BIT) != 0, (raw_l & BASE_MASKED_BIT) != 0);
        const int snp_any = cnt2(snp_e != 0, snp_l != 0), snp_bad = cnt2(snp_e == 2, snp_l == 2), snp_ok = cnt2(snp_e == 1, snp_l == 1);
        const int bad = cnt2(code_e == BASE_N || code_e == BASE_DASH, code_l == BASE_N || code_l == BASE_DASH);
        const int ext_copy = oligo_copy(S.P, *R, S.copy, st.ext, e), lig_copy = oligo_copy(S.P, *R, S.copy, st.lig, l);
        const int k = (S.P->max_capture - C) / S.P->inc;
        const bool mapping = k >= 0 && k < S.P->n_sizes_all && unmapped(S.P, *R, S.unmap, k, minus, st.ext, st.lig);
        int snp_count;
        const uint32_t flags = record_flags(mapping, masked_n, l + e, S.P->masked_arm_threshold, snp_any, snp_bad, snp_ok, bad != 0, snp_count);
        wave_lds_sync();
        return {ext_copy, lig_copy, masked_n, snp_count, (int)flags, bad != 0, (int)junction_code(s_lig[0], s_lig[1])};
    }
    // bases [c0, c0 + lenx) of the oriented insert; BASE_OTHER outside the region's sequence
    __device__ __forceinline__ void stage_insert(uint8_t* s_ins, int c0, int lenx, int t, int nt) const
    {
        for (int i = t; i < lenx; i += nt) {
            const int b = base_at(minus ? p + ss - 1 - (c0 + i) : p + c0 + i) & BASE_CODE_MASK;
            s_ins[i] = (uint8_t)(minus ? comp_code(b) : b);
        }
    }
};

__device__ __forceinline__ BatchEntry list_entry(const BatchSrc& S, int64_t i)
{
    const mipgen_candidate c = S.cands[i];
    BatchEntry en;
    en.S = S; en.R = S.regions + c.region;
    en.p = c.scan_start; en.C = c.capture_size; en.e = c.ext_len; en.l = c.lig_len; en.ss = en.C - en.e - en.l;
    en.minus = c.strand != 0;
    en.valid = constructed(*en.R, en.p, en.C, en.e, en.l) && en.e <= MIPGEN_MAX_OLIGO && en.l <= MIPGEN_MAX_OLIGO && en.e >= 2 && en.l >= 2;
    en.out = i; en.lrc = en.R->lrc;
    return en;
}

struct ProbeEntry {
    const uint8_t* bytes;
    ProbeRec pr;
    int e, l, ss;                  // 1 <= e, l <= MIPGEN_MAX_OLIGO (checked by the host)
    static constexpr bool valid = true;
    int64_t out;
    const double* lrc;

    // the oriented arms as the file holds them: no strand, no masked / SNP bits, no table to look a copy number up in
    __device__ __forceinline__ ArmInts stage_arms(uint8_t* s_ext, uint8_t* s_lig, int lane) const
    {
        const uint8_t code_e = lane < e ? ascii_base_code(bytes[pr.ext_off + lane]) : (uint8_t)BASE_A;
        const uint8_t code_l = lane < l ? ascii_base_code(bytes[pr.lig_off + lane]) : (uint8_t)BASE_A;
        if (lane < e) s_ext[lane] = code_e;
        if (lane < l) s_lig[lane] = code_l;
        if (lane == 0 && l < 2) s_lig[1] = BASE_OTHER;                    // a one-base arm has no junction dimer (lig_probe_sequence.substr(0, 2), SVMipv4.cpp:103)
        // the guard of SVMipv4.cpp:63: N in an arm, '-' in mip_seq = ligation arm + middle + extension arm (the host looked at the middle: pr.guard)
        const bool bad_lane = (lane < e && (code_e == BASE_N || code_e == BASE_DASH)) || (lane < l && (code_l == BASE_N || code_l == BASE_DASH));
        const bool guard = pr.guard != 0 || __ballot(bad_lane) != 0ull;
        wave_lds_sync();
        return {pr.ext_copy, pr.lig_copy, 0, 0, (int)(MIPGEN_FLAG_VALID | (guard ? MIPGEN_FLAG_GUARD : 0u)), guard, (int)junction_code(s_lig[0], s_lig[1])};
    }
    __device__ __forceinline__ void stage_insert(uint8_t* s_ins, int c0, int lenx, int t, int nt) const
    {
        for (int i = t; i < lenx; i += nt) s_ins[i] = ascii_base_code(bytes[pr.ins_off + c0 + i]);
    }
};

__device__ __forceinline__ ProbeEntry list_entry(const ProbeSrc& S, int64_t i)
{
    const int64_t pi = S.sel ? S.sel[i] : (S.order ? (int64_t)S.order[i] : i);
    ProbeEntry en;
    en.bytes = S.bytes; en.pr = S.probes[pi];
    en.e = en.pr.ext_len; en.l = en.pr.lig_len; en.ss = en.pr.ins_len;
    en.out = S.sel ? i : pi;
    en.lrc = en.pr.lrc_index >= 0 ? S.lrc + (int64_t)en.pr.lrc_index * MIPGEN_N_LRC : nullptr;
    return en;
}
