// Table stage of k_svr_dense: the numbering of its batches and the integer side of an entry - from (batch, lane) to the LDS byte addresses the entry
// reads and the one it writes.  Host + device, no floating point: tests/svr_table_decode.cpp walks every batch of every tile shape lane by lane.
//
// A wavefront draws `base`, a multiple of 64, from the work counter; the index space is
//     [0, nU_pad)  upstream arm windows  |  [nU_pad, nU_pad + nD_pad)  downstream arm windows  |  [.., + n_ins)  inserts        (pads to 64)
// so the role of a batch is a scalar: whatever depends on it (2-mer array distance, per-length constants, copy-number feature row) is chosen once per
// batch on the scalar unit, and a lane adds its entry's fields to scalar bases.  The descriptors stay packed as they were stored, nU + nD pairs of words
// (e_a, e_b) and nothing for the pads: the entry of a lane is (scalar first) + lane, and the lanes past a range's count idle.
#pragma once
#include <stdint.h>
#include "common.h"

#define SVR_SLOT (SVR_GROUP * 8)             // bytes of one SV-interleaved slot
static_assert(SVR_SLOT == 24, "the reciprocal records {1/i, 1/(i-1), 1/(i-2)} have the pitch of a slot: one scaled length addresses both");

// ---- descriptor word e_b of an arm window: every field is a ready-made byte offset ---------------------------------------------------------------
//   len * SVR_SLOT (12 b: len <= 127)  |  byte offset of the junction term inside the TJ table (9 b: code 0 = not a ligation arm, 17 = junction not ACGT,
//   both -> a zero term) << 12  |  byte offset of log10(copy) (10 b: copy code 0..101) << 21
SVR_HD uint32_t svr_ent_b_pack(uint32_t len, uint32_t jcode, uint32_t cpc) { return len * SVR_SLOT | (jcode * SVR_SLOT) << 12 | (cpc * 8u) << 21; }

// ---- batch numbering -----------------------------------------------------------------------------------------------------------------------------
enum { SVR_BATCH_UP = 0, SVR_BATCH_DOWN = 1, SVR_BATCH_INSERT = 2 };
struct SvrBatch {
    int role;      // scalar: which of the three ranges the batch lies in
    int first;     // lane 0's entry: index of its descriptor pair (arm windows), insert number position * ssr + scan-size index (inserts)
    int live;      // lanes 0 .. live - 1 have an entry (may exceed 64: the whole batch)
};
SVR_HD int svr_batch_pad(int n) { return (n + 63) & ~63; }
SVR_HD int svr_table_work(int nU, int nD, int n_ins) { return svr_batch_pad(nU) + svr_batch_pad(nD) + n_ins; }      // the counter's range
SVR_HD SvrBatch svr_batch(int base, int nU, int nD, int n_ins)
{
    const int up_end = svr_batch_pad(nU), arm_end = up_end + svr_batch_pad(nD);
    SvrBatch b;
    if (base < up_end) { b.role = SVR_BATCH_UP; b.first = base; b.live = nU - base; }
    else if (base < arm_end) { b.role = SVR_BATCH_DOWN; b.first = nU + (base - up_end); b.live = nD - (base - up_end); }
    else { b.role = SVR_BATCH_INSERT; b.first = base - arm_end; b.live = n_ins - b.first; }
    return b;
}

// ---- what an arm batch takes from its role, in one word per role (two scalars stay alive across the SV loop, not seven) ----------------------------
//   dB (13 b): (slots of the role's prefix arrays - 1) * SLOT, 1-mer slot -> one slot before the same 2-mer slot
//   k  (16 b): (first per-length constant of the role - its shortest arm) * SLOT: + len * SLOT = the constant of a length; a PF byte offset like e_a's
//   copy-number feature row of the role's arm (1 b): the ligation arm's (F_LLC = F_LEC + 1) or the extension arm's
static_assert(F_LLC == F_LEC + 1, "one bit tells the two copy-number rows apart");
SVR_HD uint32_t svr_role_pack(uint32_t dB, uint32_t k, bool lig) { return dB | k << 13 | (lig ? 1u : 0u) << 31; }
SVR_HD uint32_t svr_role_dB(uint32_t rw) { return rw & 0x1FFFu; }
SVR_HD uint32_t svr_role_k(uint32_t rw) { return (rw >> 13) & 0xFFFFu; }
SVR_HD uint32_t svr_role_copy_row(uint32_t rw) { return (uint32_t)F_LEC * SVR_SLOT + (rw >> 31) * SVR_SLOT; }     // byte offset in an SV-interleaved model row

// a * b + c with a, b < 2^24: one v_mad_u32_u24 (left to itself the compiler widens such an address to a 64-bit multiply-add)
SVR_HD uint32_t svr_mad24(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
    return r;
#else
    return (a & 0xFFFFFFu) * (b & 0xFFFFFFu) + c;
#endif
}

// ---- arm window: exponent = per-length constant + junction term + copy term + (1/len) dF1 + (1/(len-1)) dF2 ----------------------------------------
struct SvrArmAddr {
    uint32_t A1, A0;       // 1-mer prefix slots: window start, window end
    uint32_t Bp, B0;       // 2-mer prefix array: one slot before the window start (read at + one slot), window end
    uint32_t Kp, Tj;       // per-length constant, junction term
    uint32_t rv, lc;       // reciprocal record of the length, log10(copy)
    uint32_t dst;          // the factor's slot in TB
};
// scalar bases: pf_a the PF block; dB = (slots of the role's prefix array - 1) * SLOT; k_a = pf_a + (the role's first per-length constant - its shortest
// arm) * SLOT; tj_a = pf_a + the TJ table; rv_a, lg_a, tb_a the reciprocal records, the log10 table and TB
SVR_HD SvrArmAddr svr_arm_decode(uint32_t ea, uint32_t eb, uint32_t pf_a, uint32_t dB, uint32_t k_a, uint32_t tj_a, uint32_t rv_a, uint32_t lg_a, uint32_t tb_a)
{
    SvrArmAddr A;
    const uint32_t lenS = eb & 0xFFFu;
    A.A1 = pf_a + (ea & 0xFFFFu);
    A.A0 = A.A1 + lenS;
    A.Bp = A.A1 + dB;
    A.B0 = A.Bp + lenS;
    A.Kp = k_a + lenS;
    A.Tj = tj_a + ((eb >> 12) & 0x1FFu);
    A.rv = rv_a + lenS;
    A.lc = lg_a + (eb >> 21);
    A.dst = tb_a + (ea >> 16);
    return A;
}

// ---- insert window (position pi, scan size ssmin + ssi) ------------------------------------------------------------------------------------------
// Entry first + lane with first = bq * ssr + br and lane = lane_q * ssr + lane_r: ssi = br + lane_r, pi = bq + lane_q, one wrap at ssr.  All four
// come in multiplied by SVR_SLOT (the batch's on the scalar unit, the lane's once per kernel), and so does ssr: every address is a sum.
struct SvrInsAddr {
    uint32_t F1, F2, F3;   // 1/2/3-mer prefix slots of the position
    uint32_t E1, E2, E3;   // ... and of position + scan size (- 1, - 2)
    uint32_t Ti;           // per-scan-size term
    uint32_t rv;           // reciprocal record of the scan size
    uint32_t dst;          // the factor's slot in IT
};
// scalar bases: ss0 = ssmin * SLOT; i1 = slots of an insert prefix array * SLOT; ti_a = pf_a + the per-scan-size terms; it_a = IT, it_p its position pitch
SVR_HD SvrInsAddr svr_ins_decode(uint32_t bqS, uint32_t brS, uint32_t lane_qS, uint32_t lane_rS, uint32_t ssrS, uint32_t pf_a, uint32_t ss0, uint32_t i1,
                                 uint32_t ti_a, uint32_t rv_a, uint32_t it_a, uint32_t it_p)
{
    SvrInsAddr I;
    uint32_t ssiS = brS + lane_rS, piS = bqS + lane_qS;
    if (ssiS >= ssrS) { ssiS -= ssrS; piS += SVR_SLOT; }
    I.F1 = pf_a + piS;
    I.E1 = I.F1 + ss0 + ssiS;                                  // prefix slot p + ss of the 1-mer array
    I.F2 = I.F1 + i1; I.F3 = I.F2 + i1;
    I.E2 = I.E1 + (i1 - SVR_SLOT); I.E3 = I.E1 + (2u * i1 - 2u * SVR_SLOT);   // p + ss - 1 of the 2-mer, p + ss - 2 of the 3-mer array
    I.Ti = ti_a + ssiS;
    I.rv = rv_a + ss0 + ssiS;
    I.dst = svr_mad24(ssiS, it_p, piS + it_a);                 // IT[ssi][it_p positions][group]
    return I;
}
