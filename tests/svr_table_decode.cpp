// Host check of the table stage's batch numbering and address arithmetic (mipgen_amd/csrc/svr_table_decode.h), compiled on its own by
// tests/test_svr_table_decode_cpu.py.  For every tile of 1..28 positions x 1..9 capture sizes and of 29..90 positions x 1 capture size (capture
// increment 5, largest capture 180), on both strands (the strands swap the arms' roles), with the default arm pairs (12 + 12 lengths) and with the pairs
// (16,24) (17,24) (18,24) (16,25) (3 extension, 2 ligation lengths), it walks the work counter's range batch by batch and lane by lane, as k_svr_dense
// does:  base -> svr_batch -> (role, first entry, live lanes);  a live lane of an arm batch decodes the packed descriptors of entry first + lane with
// svr_arm_decode and the role's packed constants, a live lane of an insert batch decodes (position, scan size) with svr_ins_decode from the scaled
// quotient / remainder of the batch and of the lane.
//   * every address, and the slot the factor is stored to, equals the formula the kernel used before the numbering was changed - restated below from
//     the entry's plain fields (role, window, length, junction code, copy code), for both PF buffers;
//   * every upstream, downstream and insert entry is produced exactly once; a lane past its range's count produces nothing; the role of a batch is the
//     role of each of its entries;
//   * the packed fields fit their bits (16-bit PF and TB offsets, 13 + 16 bits of a role word, 24-bit multiply operands);
//   * svr_layout().total_bytes is what the layout's restated sum gives: the tile shapes are sized from it.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#include "../mipgen_amd/csrc/svr_table_decode.h"

static int fails = 0;
static long checked_arm = 0, checked_ins = 0, idle_lanes = 0, tiles = 0;
#define CHECK(c, ...) do { if (!(c) && fails++ < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// the layout's footprint, restated (doubles first, then the byte-addressed tail)
static int ref_total_bytes(int np, int ssmin, int ssmax, int Lmax, int n_arm, int group, int n_up, int n_dn, int it_pitch)
{
    const int ssr = ssmax - ssmin + 1, nq = np + ssr - 1;
    const int ins_sl = svr_pad_slots(np + ssmax), up_sl = svr_pad_slots(Lmax + np), dn_sl = svr_pad_slots(nq + Lmax);
    const int rinv_len = (ssmax > Lmax ? ssmax : Lmax) + 2;
    long o = 3 * rinv_len + 102 + 44 + 2 * group * SV_ROW;
    const int pf_stride = 3 * ins_sl + 2 * up_sl + 2 * dn_sl + 2 * n_arm + 1 + 18 + ssr;
    int pf = 2 * group * pf_stride;
    const int scratch = (np * (80 * 4 + ssr * 16) + 7) / 8;
    if (pf < scratch) pf = scratch;
    o += pf;
    o += group * (np * n_arm + nq * n_arm);
    o += group * (it_pitch > 0 ? ssr * it_pitch : np * (ssr | 1));
    long bytes = o * 8;
    bytes += SVR_N_ARR * 16 * 4;
    bytes += 2 * (np * n_up + nq * n_dn) * 4;
    bytes += 2 * SVR_MAX_CHUNK * (SVR_MAX_THREADS / 64) + 16;
    bytes = (bytes + 15) & ~15L;
    bytes += 64;
    bytes += 4 * (3 * ins_sl + 2 * up_sl + 2 * dn_sl);
    bytes += np + ssmax + 2 * Lmax + 1 + 8;
    return (int)((bytes + 15) & ~15L);
}

struct Pairs { int e_min, e_max, l_min, l_max, min_sum, max_sum; };

static void walk_tile(const Pairs& Q, int np, int kc, bool minus)
{
    const int inc = 5, lanes = 256, group = SVR_GROUP, max_capture = 180, n_threads = 1024;
    const int n_e = Q.e_max - Q.e_min + 1, n_l = Q.l_max - Q.l_min + 1, Lmax = Q.l_max > Q.e_max ? Q.l_max : Q.e_max, n_arm = (n_e > n_l ? n_e : n_l) | 1;
    const int Cmax = max_capture, Cmin = Cmax - (kc - 1) * inc, ssmax = Cmax - Q.min_sum, ssmin = Cmin - Q.max_sum, ssr = ssmax - ssmin + 1;
    if (svr_layout(np, ssmin, ssmax, Lmax, n_arm, group, n_e, n_l, n_threads, 0).total_bytes > SVR_LDS_LIMIT || np * kc > lanes) return;   // no such tile
    const int pitch = svr_it_pitch(np, kc, inc, lanes, ssmin, ssmax, Lmax, n_arm, group, n_e, n_l, n_threads);
    const int up_min = minus ? Q.l_min : Q.e_min, dn_min = minus ? Q.e_min : Q.l_min, n_up = minus ? n_l : n_e, n_dn = minus ? n_e : n_l;
    const int up_cp_f = minus ? F_LLC : F_LEC, dn_cp_f = minus ? F_LEC : F_LLC;
    const SvrLayout L = svr_layout(np, ssmin, ssmax, Lmax, n_arm, group, n_up, n_dn, n_threads, pitch);
    tiles++;
    CHECK(L.total_bytes == ref_total_bytes(np, ssmin, ssmax, Lmax, n_arm, group, n_up, n_dn, pitch), "np %d kc %d: total_bytes %d, restated %d", np, kc,
          L.total_bytes, ref_total_bytes(np, ssmin, ssmax, Lmax, n_arm, group, n_up, n_dn, pitch));
    const uint32_t SLOT = SVR_SLOT;
    const int nq = L.nq, nU = np * n_up, nD = nq * n_dn, n_ent = nU + nD, n_ins = np * ssr;
    CHECK(n_ent == L.n_ent, "np %d kc %d: %d entries, the layout keeps %d", np, kc, n_ent, L.n_ent);
    const int S_ins = L.ins_sl, S_up = L.up_sl;
    // LDS byte addresses as the kernel takes them (the dynamic segment starts at 0)
    const uint32_t rows_a = L.rows * 8, pf_a0 = L.pf * 8, tb_a = L.tb * 8, it_a = L.it * 8, rv_a = L.rinv * 8, lg_a = L.lg10 * 8;
    const uint32_t pf_bytes = SVR_GROUP * L.pf_stride * 8;
    const uint32_t dBu = L.up_sl * SLOT - SLOT, dBd = L.dn_sl * SLOT - SLOT, kU = (L.ku - up_min) * SLOT, kD = (L.kd - dn_min) * SLOT;
    const uint32_t tj_off = L.tj * SLOT, ti_off = L.ti * SLOT, i1 = L.ins_sl * SLOT, ss0 = ssmin * SLOT;
    CHECK(dBu < (1u << 13) && dBd < (1u << 13) && kU < (1u << 16) && kD < (1u << 16), "np %d kc %d: role fields %u %u %u %u", np, kc, dBu, dBd, kU, kD);
    const uint32_t roleU = svr_role_pack(dBu, kU, up_cp_f == F_LLC), roleD = svr_role_pack(dBd, kD, dn_cp_f == F_LLC);
    CHECK((uint32_t)ssr * SLOT < (1u << 24) && (uint32_t)L.it_p < (1u << 24), "np %d kc %d: 24-bit operands", np, kc);

    // the descriptors, as phase 0b of the kernel stores them: entry w < nU upstream (position major, length minor), then downstream (q index major)
    struct Plain { bool up; int wl, li, len, s0; uint32_t jcode, cpc; };
    std::vector<Plain> plain(n_ent);
    std::vector<uint32_t> ent_a(n_ent), ent_b(n_ent);
    for (int w = 0; w < n_ent; w++) {
        Plain p;
        p.up = w < nU;
        int s;
        if (p.up) { p.wl = w / n_up; p.li = w - p.wl * n_up; p.len = up_min + p.li; s = Lmax + p.wl - p.len; }
        else { const int w2 = w - nU; p.wl = w2 / n_dn; p.li = w2 - p.wl * n_dn; p.len = dn_min + p.li; s = Lmax + ssmin + p.wl; }
        p.s0 = p.up ? s : p.wl;
        const bool is_lig = p.up ? minus : !minus;
        p.jcode = is_lig ? (uint32_t)(w * 7 % 17) + 1 : 0;               // any code 0..17 and any copy code 0..101: the decode must carry them through
        p.cpc = (uint32_t)(w * 13 % 102);
        plain[w] = p;
        const uint32_t lo = (uint32_t)((3 * S_ins + (p.up ? 0 : 2 * S_up) + p.s0) * (int)SLOT), hi = (uint32_t)(((p.up ? L.tu : L.td) + p.wl * n_arm + p.li) * (int)SLOT);
        CHECK(lo < 65536 && hi < 65536, "np %d kc %d entry %d: e_a halves %u %u", np, kc, w, lo, hi);
        ent_a[w] = lo | hi << 16;
        ent_b[w] = svr_ent_b_pack((uint32_t)p.len, p.jcode, p.cpc);
    }

    const int n_tot = svr_table_work(nU, nD, n_ins);
    CHECK(n_tot % 64 == n_ins % 64 && n_tot - n_ins - n_ent < 128 && n_tot - n_ins >= n_ent, "np %d kc %d: %d work items for %d + %d entries", np, kc, n_tot, n_ent, n_ins);
    std::vector<int> seen_arm(n_ent, 0), seen_ins(n_ins, 0);
    for (int parity = 0; parity < 2; parity++) {
        const uint32_t PF_a = pf_a0 + parity * pf_bytes, rowk_a = rows_a + parity * SVR_GROUP * SV_ROW * 8;
        for (int base = 0; base < n_tot; base += 64) {
            const SvrBatch B = svr_batch(base, nU, nD, n_ins);
            CHECK(B.live > 0 || B.role != SVR_BATCH_INSERT, "np %d kc %d base %d: an insert batch without entries", np, kc, base);
            for (int lane = 0; lane < 64; lane++) {
                if (lane >= B.live) { idle_lanes++; continue; }                  // produces nothing
                if (B.role != SVR_BATCH_INSERT) {
                    const int e = B.first + lane;
                    CHECK(e >= 0 && e < n_ent, "np %d kc %d base %d lane %d: entry %d of %d", np, kc, base, lane, e, n_ent);
                    if (e < 0 || e >= n_ent) continue;
                    const Plain& p = plain[e];
                    CHECK(p.up == (B.role == SVR_BATCH_UP), "np %d kc %d base %d lane %d: entry %d in a batch of the other role", np, kc, base, lane, e);
                    if (parity == 0) seen_arm[e]++;
                    const uint32_t rw = B.role == SVR_BATCH_UP ? roleU : roleD;
                    const SvrArmAddr A = svr_arm_decode(ent_a[e], ent_b[e], PF_a, svr_role_dB(rw), PF_a + svr_role_k(rw), PF_a + tj_off, rv_a, lg_a, tb_a);
                    const uint32_t Sc = rowk_a + svr_role_copy_row(rw);
                    // the formulas of the kernel before the change, from the plain fields
                    const uint32_t lenS = (uint32_t)p.len * SLOT;
                    const uint32_t A1 = PF_a + (uint32_t)(3 * S_ins + (p.up ? 0 : 2 * S_up) + p.s0) * SLOT, A0 = A1 + lenS;
                    const uint32_t Bp = A1 + (p.up ? dBu : dBd), B0 = Bp + lenS;
                    const uint32_t Kp = PF_a + (p.up ? kU : kD) + lenS, Tj = PF_a + tj_off + p.jcode * SLOT;
                    const uint32_t Sc_ref = rowk_a + (uint32_t)(p.up ? up_cp_f : dn_cp_f) * SLOT;
                    const uint32_t rv = rv_a + (uint32_t)p.len * 24u, lc = lg_a + p.cpc * 8u;
                    const uint32_t dst = tb_a + (uint32_t)((p.up ? L.tu : L.td) + p.wl * n_arm + p.li) * SLOT;
                    CHECK(A.A1 == A1 && A.A0 == A0 && A.Bp == Bp && A.B0 == B0, "np %d kc %d entry %d: prefix slots %u %u %u %u, expected %u %u %u %u", np, kc, e,
                          A.A1, A.A0, A.Bp, A.B0, A1, A0, Bp, B0);
                    CHECK(A.Kp == Kp && A.Tj == Tj && Sc == Sc_ref, "np %d kc %d entry %d: constants %u %u %u, expected %u %u %u", np, kc, e, A.Kp, A.Tj, Sc, Kp, Tj, Sc_ref);
                    CHECK(A.rv == rv && A.lc == lc && A.dst == dst, "np %d kc %d entry %d: rinv / log10 / dst %u %u %u, expected %u %u %u", np, kc, e, A.rv, A.lc, A.dst, rv, lc, dst);
                    CHECK(A.dst + SLOT <= it_a && A.dst >= tb_a, "np %d kc %d entry %d: dst %u outside TB", np, kc, e, A.dst);
                    checked_arm++;
                } else {
                    const int wi = B.first + lane;
                    CHECK(wi >= 0 && wi < n_ins, "np %d kc %d base %d lane %d: insert %d of %d", np, kc, base, lane, wi, n_ins);
                    if (wi < 0 || wi >= n_ins) continue;
                    if (parity == 0) seen_ins[wi]++;
                    const int bq = B.first / ssr, br = B.first - bq * ssr;
                    const uint32_t lane_qS = (uint32_t)(lane / ssr) * SLOT, lane_rS = (uint32_t)(lane % ssr) * SLOT;
                    const SvrInsAddr I = svr_ins_decode((uint32_t)bq * SLOT, (uint32_t)br * SLOT, lane_qS, lane_rS, (uint32_t)ssr * SLOT, PF_a, ss0, i1, PF_a + ti_off, rv_a,
                                                        it_a, (uint32_t)L.it_p);
                    // the formulas of the kernel before the change
                    const int pi = wi / ssr, ssi = wi - pi * ssr;
                    const uint32_t ssiS = (uint32_t)ssi * SLOT;
                    const uint32_t F1 = PF_a + (uint32_t)pi * SLOT, E1 = F1 + ss0 + ssiS, F2 = F1 + i1, F3 = F2 + i1;
                    const uint32_t E2 = E1 + (i1 - SLOT), E3 = E1 + (2u * i1 - 2u * SLOT), Ti = PF_a + ti_off + ssiS;
                    const uint32_t rv = rv_a + (uint32_t)(ssmin + ssi) * 24u;
                    const uint32_t dst = it_a + (uint32_t)(ssi * L.it_p + pi) * SLOT;
                    CHECK(I.F1 == F1 && I.F2 == F2 && I.F3 == F3 && I.E1 == E1 && I.E2 == E2 && I.E3 == E3, "np %d kc %d insert %d: prefix slots differ (F1 %u / %u, E1 %u / %u)",
                          np, kc, wi, I.F1, F1, I.E1, E1);
                    CHECK(I.Ti == Ti && I.rv == rv && I.dst == dst, "np %d kc %d insert %d: Ti / rinv / dst %u %u %u, expected %u %u %u", np, kc, wi, I.Ti, I.rv, I.dst, Ti, rv, dst);
                    CHECK(I.dst >= it_a && I.dst + SLOT <= (uint32_t)L.bytes_desc, "np %d kc %d insert %d: dst %u outside IT", np, kc, wi, I.dst);
                    checked_ins++;
                }
            }
        }
    }
    for (int w = 0; w < n_ent; w++) CHECK(seen_arm[w] == 1, "np %d kc %d %c: %s entry %d produced %d times", np, kc, minus ? '-' : '+', w < nU ? "upstream" : "downstream", w, seen_arm[w]);
    for (int w = 0; w < n_ins; w++) CHECK(seen_ins[w] == 1, "np %d kc %d %c: insert %d produced %d times", np, kc, minus ? '-' : '+', w, seen_ins[w]);
}

int main()
{
    const Pairs def = {16, 27, 18, 29, 40, 45};        // the default arm pairs: extension arms 16..27, ligation arms 18..29 (sums 40..45)
    const Pairs uneven = {16, 18, 24, 25, 40, 42};     // (16,24) (17,24) (18,24) (16,25): n_e = 3, n_l = 2
    for (const Pairs* Q : {&def, &uneven})
        for (int minus = 0; minus < 2; minus++) {
            for (int kc = 1; kc <= 9; kc++)
                for (int np = 1; np <= 28; np++) walk_tile(*Q, np, kc, minus != 0);
            for (int np = 29; np <= 90; np++) walk_tile(*Q, np, 1, minus != 0);
        }
    {   // the counts the GPU cases are built on (default pairs, 27 positions per tile): last tiles of 5, 6 and 16 positions
        const SvrBatch b5 = svr_batch(0, 5 * 12, 600, 230), b6 = svr_batch(64, 6 * 12, 612, 276), b16 = svr_batch(192, 16 * 12, 732, 736);
        CHECK(b5.role == SVR_BATCH_UP && b5.live == 60, "nU = 60: one batch with 60 live lanes");
        CHECK(b6.role == SVR_BATCH_UP && b6.first == 64 && b6.live == 8, "nU = 72: a second batch of 8");
        CHECK(b16.role == SVR_BATCH_DOWN && b16.first == 192 && b16.live == 732, "nU = 192: the downstream range starts at the fourth batch");
    }
    printf("%ld tile walks, %ld arm entries and %ld insert entries decoded, %ld idle lanes; %d failures\n", tiles, checked_arm, checked_ins, idle_lanes, fails);
    return fails ? 1 : 0;
}
