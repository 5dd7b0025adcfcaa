// kernels_logistic.hip — dense-grid candidate construction (integer record of design_mip) and the logistic
// scorer, hand-written for gfx950.
//
// Replaces, per candidate (p, C, (e,l), strand) of the dense grid:
//   Plus/MinusSVMipv4 ctor geometry      /root/reference/PlusSVMipv4.cpp:7-14, MinusSVMipv4.cpp:30-37
//   design_mip ints                      /root/reference/mipgen.cpp:599-762 (copies, masked N, mapping/masking/SNP flags)
//   SVMipv4::get_score                   /root/reference/SVMipv4.cpp:114-248
//
// Mapping to the hardware: one workgroup per run of scan-start positions of one region.  The region bytes the
// tile can touch are staged in LDS once and turned into packed 16-bit prefix counts (three u64 words per base:
// prefix_words.h, the front this kernel shares with k_logistic_dense), so every window statistic of a candidate
// (A/C/G counts, N guard, masked N, SNP counts, GC/AT class switches) is two ds_read_b64 and a subtract - no
// per-base loop, no std::string.  One candidate per lane; consecutive
// lanes own consecutive dense-grid indices, so the 8-byte score and 8-byte record stores of a wave are two
// contiguous 512-byte segments (coalesced, the only compulsory HBM traffic of this kernel: 16 B/candidate).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "device_utils.h"

#include "logistic_device.h"
#include "mip_record.h"
#include "prefix_words.h"

// grid = number of tiles; block = LOG_THREADS; dynamic LDS = lds_bytes(span_max)
#define LOG_RINV 512
template <bool SCORE>
__global__ __launch_bounds__(LOG_THREADS) void k_records_logistic(
    const DevParams* __restrict__ P, const DevRegion* __restrict__ regions, const LogTile* __restrict__ tiles,
    int n_tiles, const uint8_t* __restrict__ bases, const int32_t* __restrict__ copy,
    const uint8_t* __restrict__ unmap, const HostConsts* __restrict__ HC, double* __restrict__ scores,
    uint64_t* __restrict__ records, int64_t* __restrict__ sat_idx, unsigned int* __restrict__ sat_count, unsigned int sat_cap)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const LogTile tile = tiles[xcd_remap(blockIdx.x, n_tiles)];
    const DevRegion& R = regions[tile.region];
    const int tid = threadIdx.x;

    const int A = P->n_pairs;
    const int nK = R.n_sizes;
    const int Cmax = P->max_capture - R.k0 * P->inc;
    const int Lmax = max(P->e_max, P->l_max);
    const int p_first = R.first_pos + tile.p0;                 // chromosome coordinate of the tile's first p
    const int lo = p_first - Lmax;                             // chromosome coordinate of tile-local base 0
    const int span = tile.np + Cmax + Lmax;                    // bases [lo, lo+span)

    PrefixWords W = prefix_words_carve(smem, span);
    double* rinv = (double*)(W.scratch + PW_SCRATCH);          // LOG_RINV entries: 1.0 / i by true division
    W.sb = (uint8_t*)(rinv + LOG_RINV);                        // span

    for (int i = tid; i < LOG_RINV; i += LOG_THREADS) rinv[i] = i > 0 ? 1.0 / (double)i : 0.0;
    prefix_words_build<LOG_THREADS>(W, R, bases, lo, span);

    // ---- one candidate per lane --------------------------------------------------------------------
    const uint32_t row = (uint32_t)(2 * A);                    // candidates per (p, C)
    const uint32_t per_pos = row * (uint32_t)nK;
    const uint32_t n_cand = per_pos * (uint32_t)tile.np;
    const uint32_t M_row = 0xFFFFFFFFu / row + 1, M_k = 0xFFFFFFFFu / (uint32_t)nK + 1;
    const int64_t out_base = R.out_off + (int64_t)tile.p0 * per_pos;
    const double thr = P->masked_arm_threshold;

    for (uint32_t idx = tid; idx < n_cand; idx += LOG_THREADS) {
        uint32_t rc = fastdiv(idx, M_row);                     // (pl, ki)
        uint32_t in_row = idx - rc * row;
        uint32_t pl = nK == 1 ? rc : fastdiv(rc, M_k);            // the magic constant overflows for divisor 1
        uint32_t ki = rc - pl * (uint32_t)nK;
        const bool minus = in_row >= (uint32_t)A;              // strand-major inside a (position, size) row
        const int a = (int)(minus ? in_row - (uint32_t)A : in_row);
        const int e = P->arm_ext[a], l = P->arm_lig[a];
        const int C = Cmax - (int)ki * P->inc;
        const int ss = C - e - l;
        const int p = p_first + (int)pl;

        uint64_t rec = 0;
        double score = 0.0;
        if (constructed(R, p, C, e, l)) {                      // :443-444
            const ArmStarts st = arm_starts(p, ss, e, l, minus);
            const int ext_start = st.ext, lig_start = st.lig;
            const int be = ext_start - lo, bl = lig_start - lo, bi = p - lo;    // tile-local
            const ArmCounts ce = arm_window(W, be, e), cl = arm_window(W, bl, l);
            const bool guard = (ce.bad + cl.bad) != 0;                          // SVMipv4.cpp:63,116
            const int ext_copy = oligo_copy(P, R, copy, ext_start, e), lig_copy = oligo_copy(P, R, copy, lig_start, l);
            const bool mapping = unmapped(P, R, unmap, R.k0 + (int)ki, minus, ext_start, lig_start);
            const uint32_t masked_n = ce.masked + cl.masked;
            int snp_count;
            const uint32_t flags = record_flags(mapping, (int)masked_n, l + e, thr, (int)(ce.snp_any + cl.snp_any), (int)(ce.snp_bad + cl.snp_bad),
                                                (int)(ce.snp_ok + cl.snp_ok), guard, snp_count);
            const uint32_t jc = lig_junction(W.sb, bl, l, minus);
            rec = pack_record(ext_copy, lig_copy, (int)masked_n, snp_count, flags, jc);

            if (SCORE) {
                if (guard) score = -1000.0;
                else {
                    const InsertCounts t = insert_window(W, bi, ss, minus);
                    const int run = t.run;
                    Vars x;
                    const double dl = (double)e, ll = (double)l, dn = (double)ss;
                    // counts on the oriented strand: revcomp swaps G<->C and A<->T
                    const double e_g = minus ? (double)ce.nC : (double)ce.nG, l_g = minus ? (double)cl.nC : (double)cl.nG,
                                 t_g = minus ? (double)t.nC : (double)t.nG;
                    const double e_a = minus ? (double)ce.nT : (double)ce.nA, l_a = minus ? (double)cl.nT : (double)cl.nA,
                                 t_a = minus ? (double)t.nT : (double)t.nA;
                    const double e_gc = (double)(ce.nC + ce.nG), l_gc = (double)(cl.nC + cl.nG), t_gc = (double)(t.nC + t.nG);
                    // contents = count * (1/len) with 1/len from the table (the reference divides; the quotients agree to 1 ulp)
                    const double re = rinv[e], rl = rinv[l], rn = ss < LOG_RINV ? rinv[ss] : 1.0 / dn;
                    x.v[MLV_BPS] = run < LOG_RINV ? dn * rinv[run] : dn / (double)run;
                    x.v[MLV_TLEN] = ss > 250 ? 250.0 : dn;
                    x.v[MLV_ELEN] = dl; x.v[MLV_LLEN] = ll;
                    x.v[MLV_EGC] = e_gc * re; x.v[MLV_LGC] = l_gc * rl; x.v[MLV_TGC] = t_gc * rn;
                    x.v[MLV_EG] = e_g * re; x.v[MLV_LG] = l_g * rl; x.v[MLV_TG] = t_g * rn;
                    x.v[MLV_EA] = e_a * re; x.v[MLV_LA] = l_a * rl; x.v[MLV_TA] = t_a * rn;
                    x.v[MLV_JS] = jc < 16 ? c_junction_scores[jc] : 0.0;
                    x.v[MLV_LEC] = log_copy_dev(HC, ext_copy);
                    x.v[MLV_LLC] = log_copy_dev(HC, lig_copy);
                    const double ex = logistic_exponent(x);
                    score = logistic_from_exponent_fast(HC, ex);
                    // b^x in [2^53, 2^54): the reference's score turns on the last bit of its pow there (kernels_logistic_dense.hip): listed for the
                    // re-score in the reference's term order with the correctly rounded power (accel_score.hip)
                    const double tb = ex * (HC->ln_base * 1.4426950408889634074);
                    if (SCORE && sat_count && tb >= 52.99 && tb <= 54.01) { const unsigned int at = atomicAdd(sat_count, 1u); if (at < sat_cap) sat_idx[at] = out_base + idx; }
                }
            }
        }
        records[out_base + idx] = rec;
        if (SCORE) scores[out_base + idx] = score;
    }
}

extern "C" size_t mipgen_logistic_lds_bytes(int span)
{
    return (prefix_words_u64(span) + LOG_RINV) * sizeof(uint64_t) + (size_t)span + 16;
}

extern "C" hipError_t mipgen_launch_records_logistic(
    hipStream_t stream, int score, int n_tiles, int span_max, const DevParams* P, const DevRegion* regions,
    const LogTile* tiles, const uint8_t* bases, const int32_t* copy, const uint8_t* unmap, const HostConsts* HC, double* scores,
    uint64_t* records, int64_t* sat_idx, unsigned int* sat_count, unsigned int sat_cap)
{
    if (n_tiles <= 0) return hipSuccess;
    size_t lds = mipgen_logistic_lds_bytes(span_max);
    if (score)
        hipLaunchKernelGGL(k_records_logistic<true>, dim3(n_tiles), dim3(LOG_THREADS), lds, stream, P, regions, tiles, n_tiles,
                           bases, copy, unmap, HC, scores, records, sat_idx, sat_count, sat_cap);
    else
        hipLaunchKernelGGL(k_records_logistic<false>, dim3(n_tiles), dim3(LOG_THREADS), lds, stream, P, regions, tiles, n_tiles,
                           bases, copy, unmap, HC, scores, records, (int64_t*)nullptr, (unsigned int*)nullptr, 0u);
    return hipGetLastError();
}
