// kernels_probe.hip — k_probe_features: the 192 features (SVMipv4::get_parameters, SVMipv4.cpp:60-113) and the integer record of probes given by
// their SEQUENCES (mipgen_accel_score_probes), the front end of the matrix-core SVR (kernels_svr_gemm.hip) for lists of such probes - what
// k_features_batch (kernels_misc.hip) is for candidates addressed by coordinates.
//
// A probe is three strand-oriented byte strings as a MIP table prints them (mipgen.cpp:765-794): extension arm, ligation arm, insert.  There is no
// resident batch behind it - no prefix tables, no copy tables, no masks: the 20 + 20 arm mers and the 84 insert mers are counted from the bytes
// themselves (LDS histogram, a lane per window start: mip_features.h), the copy numbers and the long-range row come with the probe, and nothing is
// reverse-complemented.
//
// Mapping: ONE WAVEFRONT PER PROBE, four probes per workgroup, launched in order of falling insert length.
//   * The work of a probe is its insert (tens to thousands of bases; the arms are 16-30): a 64-lane wavefront covers a 150-base insert in three
//     strides and a 1,200-base one in nineteen, with no barrier wider than the wavefront and no idle waves - a 256-thread workgroup per probe
//     would leave three of its four waves without a base to count on a typical insert and pay four workgroup barriers per probe.
//   * Wavefronts of a workgroup finish at different times only as far as their inserts differ; the host hands the kernel the probes sorted by
//     insert length (ProbeSrc::order, a counting sort), so the four probes of a workgroup are of one length class and the long ones start first:
//     the tail of the launch is made of the shortest probes.
//   * Any insert length: the insert passes through LDS in pieces of MAX_INSERT bases + two of look-ahead, as in the list kernels.
// Memory: a probe's bytes are read once, coalesced (lane i reads byte i); 1.5 KB of features are written per probe - for a 150-base insert the
// stores are 8x the loads, the kernel is bound by its feature stores like k_features_batch.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "device_utils.h"
#include "mip_record.h"
#include "mip_features.h"

#define PF_WAVES 4

__global__ __launch_bounds__(PF_WAVES * 64) void k_probe_features(int n, const ProbeSrc S, const HostConsts* __restrict__ HC, uint64_t* __restrict__ records,
                                                                   double* __restrict__ features)
{
    __shared__ uint8_t s_ext_a[PF_WAVES][MIPGEN_MAX_OLIGO + 2], s_lig_a[PF_WAVES][MIPGEN_MAX_OLIGO + 2], s_ins_a[PF_WAVES][MAX_INSERT + 2];
    __shared__ int s_cnt_a[PF_WAVES][128];          // 0..83 insert mers, 84..103 ext mers, 104..123 lig mers
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = blockIdx.x * PF_WAVES + wave;
    if (wi >= n) return;
    const int pi = S.order ? S.order[wi] : wi;
    uint8_t* s_ext = s_ext_a[wave]; uint8_t* s_lig = s_lig_a[wave]; uint8_t* s_ins = s_ins_a[wave];
    int* s_cnt = s_cnt_a[wave];
    const ProbeRec pr = S.probes[pi];
    const int e = pr.ext_len, l = pr.lig_len, ss = pr.ins_len;      // 1 <= e, l <= MIPGEN_MAX_OLIGO (checked by the host)
    s_cnt[lane] = 0; s_cnt[lane + 64] = 0;
    const uint8_t code_e = lane < e ? ascii_base_code(S.bytes[pr.ext_off + lane]) : (uint8_t)BASE_A;
    const uint8_t code_l = lane < l ? ascii_base_code(S.bytes[pr.lig_off + lane]) : (uint8_t)BASE_A;
    if (lane < e) s_ext[lane] = code_e;
    if (lane < l) s_lig[lane] = code_l;
    if (lane == 0 && l < 2) s_lig[1] = BASE_OTHER;                    // a one-base arm has no junction dimer (SVMipv4.cpp:103)
    // the guard of SVMipv4.cpp:63: N in an arm, '-' in mip_seq = ligation arm + middle + extension arm (the host looked at the middle: pr.guard)
    const bool bad_lane = (lane < e && (code_e == BASE_N || code_e == BASE_DASH)) || (lane < l && (code_l == BASE_N || code_l == BASE_DASH));
    const bool guard = pr.guard != 0 || __ballot(bad_lane) != 0ull;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int jc = (int)junction_code(s_lig[0], s_lig[1]);
    if (lane == 0) records[pi] = pack_record(pr.ext_copy, pr.lig_copy, 0, 0, MIPGEN_FLAG_VALID | (guard ? MIPGEN_FLAG_GUARD : 0u), (uint32_t)jc);
    for (int c0 = 0; c0 < ss; c0 += MAX_INSERT) {
        const int len = min(MAX_INSERT, ss - c0), lenx = min(len + 2, ss - c0);
        if (c0) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
        for (int i = lane; i < lenx; i += 64) s_ins[i] = ascii_base_code(S.bytes[pr.ins_off + c0 + i]);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        hist_insert_piece(s_ins, len, lenx, s_cnt, lane, 64);
    }
    hist_arm(s_ext, e, s_cnt + 84, lane);
    hist_arm(s_lig, l, s_cnt + 104, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const double* lrc = pr.lrc_index >= 0 ? S.lrc + (int64_t)pr.lrc_index * MIPGEN_N_LRC : nullptr;
    double* fo = features + (int64_t)pi * MIPGEN_N_FEATURES;
    for (int f = lane; f < MIPGEN_N_FEATURES; f += 64) fo[f] = mip_feature(f, s_cnt, e, l, ss, lrc, jc, pr.ext_copy, pr.lig_copy, guard, HC);
}

extern "C" hipError_t mipgen_launch_probe_features(hipStream_t stream, int n, const ProbeSrc* S, const HostConsts* HC, uint64_t* records, double* features)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_probe_features, dim3((n + PF_WAVES - 1) / PF_WAVES), dim3(PF_WAVES * 64), 0, stream, n, *S, HC, records, features);
    return hipGetLastError();
}
