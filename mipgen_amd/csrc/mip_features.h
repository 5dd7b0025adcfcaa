// mip_features.h — SVMipv4::get_parameters (SVMipv4.cpp:60-113) as the list kernels restate it: one definition each of the mer histogram over
// an oriented sequence in LDS and of the 192 feature values formed from it.  Both list kernels (kernels_misc.hip: k_candidates, a workgroup per
// entry, and k_features_batch, a wavefront per entry) go through these, whichever source staged the sequence (list_stage.h).
//
// Count layout (int[128]): 0..83 the insert mers in the reference's lexicographic list (x: 21 x, xy: 21 x + 1 + 5 y, xyz: 21 x + 1 + 5 y + 1 + z),
// 84..103 the extension arm's mers (x: 5 x, xy: 5 x + 1 + y), 104..123 the ligation arm's.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include "logistic_device.h"

#define MAX_INSERT 1024              // bases of an insert staged in LDS at a time (+ two of look-ahead); longer inserts pass in pieces

// a byte of a sequence as a file holds it -> base code.  The reference compares characters (std::string::find of "A", "AC", ..., "N", "-":
// SVMipv4.cpp:31-57, 63, 116; `current_base == "G"`, :123-134), so a lower-case letter or any other byte matches no mer, is no guard base
// and counts as "anything else" in the run walk: BASE_OTHER
__device__ __forceinline__ uint8_t ascii_base_code(uint8_t c)
{
    return c == 'A' ? BASE_A : c == 'C' ? BASE_C : c == 'G' ? BASE_G : c == 'T' ? BASE_T : c == 'N' ? BASE_N : c == '-' ? BASE_DASH : BASE_OTHER;
}

// mer histogram of one staged piece of the oriented insert, a lane per window start (stride `nl` lanes): windows that START in s[0, len) and end
// inside s[0, lenx); a window touching a non-ACGT code counts nowhere
__device__ __forceinline__ void hist_insert_piece(const uint8_t* s, int len, int lenx, int* cnt, int lane, int nl)
{
    for (int i = lane; i < len; i += nl) {
        const int x = s[i];
        if (x < 4) {
            atomicAdd(&cnt[21 * x], 1);
            if (i + 1 < lenx) {
                const int y = s[i + 1];
                if (y < 4) {
                    atomicAdd(&cnt[21 * x + 1 + 5 * y], 1);
                    if (i + 2 < lenx) { const int z = s[i + 2]; if (z < 4) atomicAdd(&cnt[21 * x + 1 + 5 * y + 1 + z], 1); }
                }
            }
        }
    }
}

// ... and of an oriented arm of n <= 64 bases, lane i on base i; cnt = the arm's 20 counters
__device__ __forceinline__ void hist_arm(const uint8_t* s, int n, int* cnt, int lane)
{
    if (lane < n) {
        const int x = s[lane];
        if (x < 4) { atomicAdd(&cnt[5 * x], 1); if (lane + 1 < n) { const int y = s[lane + 1]; if (y < 4) atomicAdd(&cnt[5 * x + 1 + y], 1); } }
    }
}

// feature f of the 192, SVMipv4.cpp:72-112: divisions are count / (len - k + 1.) in the reference's own types (int - size_t wraps for a sequence
// shorter than the mer), the GC entry sits in front of "T", and the EXTENSION arm's GC entry divides by an integer expression (:76 has no "1.").
// lrc: the region's 44 long-range frequencies, or null = zeros.  guard: N in an arm or '-' in the MIP sequence (:63) -> the all-zero vector.
__device__ __forceinline__ double mip_feature(int f, const int* s_cnt, int e, int l, int ss, const double* lrc, int jc, int ext_copy, int lig_copy, bool guard,
                                              const HostConsts* HC)
{
    double v;
    if (guard) v = 0.0;
    else if (f < F_LRC) {                         // ext block
        if (f == F_EXT_LEN) v = (double)e;
        else if (f == F_EXT_GC) v = ((double)s_cnt[84 + 10] + (double)s_cnt[84 + 5]) / (double)(uint64_t)((uint64_t)e - 1 + 1);
        else { int idx = f < F_EXT_GC ? f : f - 1; int k = (idx % 5) ? 2 : 1; v = (double)s_cnt[84 + idx] / ((double)(uint64_t)((uint64_t)e - k) + 1.); }
    } else if (f < F_INS) v = lrc ? lrc[f - F_LRC] : 0.0;
    else if (f < F_LIG) {                         // insert block
        const int g = f - F_INS;
        if (f == F_INS_LEN) v = (double)ss;
        else if (f == F_INS_GC) v = ((double)s_cnt[42] + (double)s_cnt[21]) / ((double)(uint64_t)((uint64_t)ss - 1) + 1.);
        else {
            int idx = g < 63 ? g : g - 1;
            int r = idx % 21; int k = r == 0 ? 1 : (((r - 1) % 5) == 0 ? 2 : 3);
            v = (double)s_cnt[idx] / ((double)(uint64_t)((uint64_t)ss - k) + 1.);
        }
    } else if (f < F_JUNC) {                      // lig block
        const int g = f - F_LIG;
        if (f == F_LIG_LEN) v = (double)l;
        else if (f == F_LIG_GC) v = ((double)s_cnt[104 + 10] + (double)s_cnt[104 + 5]) / ((double)(uint64_t)((uint64_t)l - 1) + 1.);
        else { int idx = g < 15 ? g : g - 1; int k = (idx % 5) ? 2 : 1; v = (double)s_cnt[104 + idx] / ((double)(uint64_t)((uint64_t)l - k) + 1.); }
    } else if (f < F_LEC) v = (jc == f - F_JUNC) ? 1.0 : 0.0;
    else v = log_copy_dev(HC, f == F_LEC ? ext_copy : lig_copy);
    return v;
}
