// Host check of the insert-factor table's pitch (mipgen_amd/csrc/common.h: svr_np_lane, svr_it_pitch, svr_layout), compiled on its own by
// tests/test_svr_it_banks_cpu.py.  For every tile of 1..28 positions and 1..9 capture sizes (capture increment 5, the default arm pairs, 256 lanes per
// pair chunk) it enumerates the LDS addresses the candidate steps of k_svr_dense read the insert factors from, half-wavefront by half-wavefront, as
// the kernel computes them: lane j = kci * np_lane + pl reads the 24-byte slot ((C - ssmin - sum) * pitch + pl) of IT with C = Cmax - kci * inc; a lane
// that owns no candidate reads column j mod 32 of the first size's row (column 0 where the pitch is shorter).
//   * wherever the chosen pitch is a conflict-free one, the 32 lanes of a half-wavefront that read different slots read different bank pairs
//     (64 banks of 4 bytes: an 8-byte read takes the pair (address / 8) mod 32) - for each of the slot's three doubles and every arm sum;
//   * the same for the downstream-factor loads of every tile whose lane pitch is a padded one (np_lane = -inc mod 32);
//   * the table stage's writes (consecutive scan sizes from consecutive lanes: a lane stride of pitch slots) stay conflict free: the pitch is odd;
//   * the tile's LDS stays within 160 KiB for both strands' role assignments, whatever pitch was chosen;
//   * the shapes the benchmark runs (27 and 25 positions x 9 sizes) do get the padded pitch, 33.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <map>
#include "../mipgen_amd/csrc/common.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c) && fails++ < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

int main()
{
    // the default arm pairs: extension arms 16..27, ligation arms 18..29 (sums 40..45)
    const int e_min = 16, e_max = 27, l_min = 18, l_max = 29, min_sum = 40, max_sum = 45, inc = 5, lanes = 256, group = SVR_GROUP, max_capture = 180;
    const int n_e = e_max - e_min + 1, n_l = l_max - l_min + 1, Lmax = l_max > e_max ? l_max : e_max, n_arm = (n_e > n_l ? n_e : n_l) | 1, n_threads = 1024;
    int n_padded = 0, n_fallback = 0, n_plain = 0, n_down = 0;
    for (int kc = 1; kc <= 9; kc++) {
        for (int np = 1; np <= 28; np++) {
            const int Cmax = max_capture, Cmin = Cmax - (kc - 1) * inc, ssmax = Cmax - min_sum, ssmin = Cmin - max_sum;
            // the tile exists: it fits with the unpadded table (that is how accel_tiles.hip sizes np)
            const SvrLayout L0 = svr_layout(np, ssmin, ssmax, Lmax, n_arm, group, n_e, n_l, n_threads, 0);
            if (L0.total_bytes > SVR_LDS_LIMIT || np * kc > lanes) continue;
            const int pitch = svr_it_pitch(np, kc, inc, lanes, ssmin, ssmax, Lmax, n_arm, group, n_e, n_l, n_threads);
            const int np_lane = svr_np_lane(np, kc, inc, lanes);
            const SvrLayout La = svr_layout(np, ssmin, ssmax, Lmax, n_arm, group, n_e, n_l, n_threads, pitch);
            const SvrLayout Lb = svr_layout(np, ssmin, ssmax, Lmax, n_arm, group, n_l, n_e, n_threads, pitch);
            CHECK(La.total_bytes <= SVR_LDS_LIMIT && Lb.total_bytes <= SVR_LDS_LIMIT, "np %d kc %d pitch %d: %d / %d bytes of LDS", np, kc, pitch, La.total_bytes, Lb.total_bytes);
            CHECK(La.it_p >= np && (pitch == 0 || La.it_p == pitch), "np %d kc %d: pitch %d in the layout, %d chosen", np, kc, La.it_p, pitch);
            // the table ends inside its reservation: the last slot read is ((ssr - 1) * pitch + np - 1)
            const int ssr = ssmax - ssmin + 1;
            CHECK(((ssr - 1) * La.it_p + np) * group * 8 + La.it * 8 <= La.bytes_desc, "np %d kc %d: the insert table overruns its area", np, kc);
            CHECK(max_sum * La.it_p < 65536, "np %d kc %d: arm sum x pitch does not fit 16 bits", np, kc);
            // the downstream-factor loads (TB row pl + C - max_sum - ssmin + (max_sum - sum), n_arm slots per row): conflict free at a padded lane pitch, the
            // lanes without a candidate on the rows of their own residue
            if (svr_lane_pitch_spreads(np_lane, kc, inc)) {
                for (int sum = min_sum; sum <= max_sum; sum++) {
                    for (int h0 = 0; h0 < lanes; h0 += 32) {
                        std::map<int, int> bank_of;
                        for (int j = h0; j < h0 + 32; j++) {
                            const int kci = j / np_lane, pl = j - kci * np_lane;
                            const bool own = kci < kc && pl < np;
                            const int row = (own ? pl + (Cmax - kci * inc) - max_sum - ssmin : svr_idle_d_row(j, np_lane, kc, inc, La.nq, max_sum - min_sum)) + (max_sum - sum);
                            CHECK(row >= 0 && row < La.nq, "np %d kc %d: downstream row %d outside the table of %d", np, kc, row, La.nq);
                            const int slot = La.td + row * n_arm, bank = (La.tb + slot * group) % 32;
                            auto it = bank_of.find(bank);
                            if (it == bank_of.end()) bank_of[bank] = slot;
                            else CHECK(it->second == slot, "np %d kc %d sum %d: lanes %d.. share bank pair %d on their downstream rows (slots %d, %d)", np, kc, sum, h0, bank, it->second, slot);
                        }
                    }
                }
                n_down++;
            }
            if (pitch == 0) { n_plain++; continue; }
            CHECK(pitch & 1, "np %d kc %d: even pitch %d (table-stage writes conflict)", np, kc, pitch);
            if (!svr_it_pitch_spreads(pitch, np_lane, kc, inc)) { n_fallback++; continue; }
            n_padded++;
            for (int sum = min_sum; sum <= max_sum; sum++) {
                for (int h0 = 0; h0 < lanes; h0 += 32) {
                    for (int g = 0; g < group; g++) {
                        std::map<int, int> bank_of;                        // bank pair -> the slot that took it
                        for (int j = h0; j < h0 + 32; j++) {
                            int kci = j / np_lane, pl = j - kci * np_lane;
                            if (!(kci < kc && pl < np)) { kci = 0; pl = svr_idle_it_col(j, La.it_p, np_lane, kc, inc); }   // a lane without a candidate: first size, column j mod 32
                            const int C = Cmax - kci * inc;
                            const int slot = (C - ssmin - sum) * La.it_p + pl;
                            CHECK(slot >= 0 && slot < ssr * La.it_p, "np %d kc %d: slot %d outside the table", np, kc, slot);
                            const int bank = ((La.it + slot * group + g)) % 32;
                            auto it = bank_of.find(bank);
                            if (it == bank_of.end()) bank_of[bank] = slot;
                            else CHECK(it->second == slot, "np %d kc %d pitch %d sum %d: lanes %d.. share bank pair %d (slots %d, %d)", np, kc, pitch, sum, h0, bank, it->second, slot);
                        }
                    }
                }
            }
        }
    }
    {   // the benchmark's shapes are padded: 27 and 25 positions x 9 capture sizes -> pitch 33; 28 x 5 cannot be (lane pitch 28: no odd pitch spreads it)
        const int ssmax = 140, ssmin9 = 140 - 45, ssmin5 = 160 - 45;
        CHECK(svr_it_pitch(27, 9, inc, lanes, ssmin9, ssmax, Lmax, n_arm, group, n_e, n_l, n_threads) == 33, "27 x 9 is not padded to 33");
        CHECK(svr_it_pitch(25, 9, inc, lanes, ssmin9, ssmax, Lmax, n_arm, group, n_e, n_l, n_threads) == 33, "25 x 9 is not padded to 33");
        CHECK(svr_it_pitch(1, 9, inc, lanes, ssmin9, ssmax, Lmax, n_arm, group, n_e, n_l, n_threads) == 1, "1 x 9 does not keep pitch 1");
        CHECK(svr_it_pitch(28, 5, inc, lanes, ssmin5, ssmax, Lmax, n_arm, group, n_e, n_l, n_threads) == 29, "28 x 5 does not fall back to 29");
    }
    printf("%d tiles padded conflict free, %d at the odd fallback pitch, %d unpadded; %d failures\n", n_padded, n_fallback, n_plain, fails);
    printf("%d tiles with conflict-free downstream rows\n", n_down);
    return fails ? 1 : 0;
}
