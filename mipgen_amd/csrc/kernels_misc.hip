// kernels_misc.hip — sparse-candidate scorer (mixed-mode re-scores, inspection) and Featurev5::get_long_range_content.
//
// k_candidates: one workgroup per candidate.  It is the literal form of the reference arithmetic:
//   * the strand-oriented ext / lig / insert sequences are materialised in LDS (list_stage.h: the one front of both list kernels),
//   * their overlapping 1- / 2- / 3-mers are counted into an LDS histogram (mip_features.h; SVMipv4.cpp:31-57),
//   * the 192 features are formed with the reference's own expressions (SVMipv4.cpp:72-112),
//   * lanes then own support vectors: each walks the 192 dimensions in index order (svm.cpp:329-368), takes
//     exp(-gamma*d2) and the partial sums coef*k are reduced with wavefront shuffles (svm.cpp:2511-2515).
// It doubles as an on-device cross-check of the window-separable dense kernel (kernels_svr.hip).
// k_features_batch: a wavefront per entry, features + record only - the front end of the matrix-core SVR (kernels_svr_gemm.hip).
// Both are templates over the SOURCE of a list entry (common.h): BatchSrc, coordinates in the resident region batch, or ProbeSrc, a probe given
// by its oriented sequences (mipgen_accel_score_probes).  The source decides how the bytes get to LDS and where copies and the long-range row come
// from (list_stage.h); everything behind the staged sequences - mer counts, features, integer features, the logistic score, the SVR walks - is the
// same code.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "kernels.h"
#include "device_utils.h"
#include "mip_record.h"
#include "logistic_device.h"
#include "mip_features.h"
#include "list_stage.h"
#include "pow_base_cr.h"

#define CAND_THREADS 256

namespace {

// one piece of the class-switch walk of run_count_slow (logistic_device.h; SVMipv4.cpp:118-142) over oriented codes: `last` < 0 before the first base
__device__ void run_count_piece(const uint8_t* s, int n, int& last, int& run)
{
    for (int i = 0; i < n; i++) {
        const int b = s[i];
        const int c = (b == BASE_G || b == BASE_C) ? 0 : ((b == BASE_A || b == BASE_T) ? 1 : 2);
        if (last < 0) last = c;
        else if (c == 0) { if (last != 0) { run++; last = 0; } }
        else if (last != 1) { run++; last = c; }
    }
}

}  // namespace

template <class Src>
__global__ __launch_bounds__(CAND_THREADS) void k_candidates(
    const Src S, const HostConsts* __restrict__ HC, const double* __restrict__ model, int n_sv, double gamma, double rho, int method,
    double* __restrict__ scores, uint64_t* __restrict__ records, double* __restrict__ features,
    mipgen_candidate_ints* __restrict__ ints_out, int literal, const unsigned int* __restrict__ n_dev)
{
    if (n_dev && blockIdx.x >= *n_dev) return;          // a device-side list length (the grid is the list's capacity): no host round trip
    __shared__ double s_term[CAND_THREADS];
    __shared__ uint8_t s_ext[MIPGEN_MAX_OLIGO + 2], s_lig[MIPGEN_MAX_OLIGO + 2], s_ins[MAX_INSERT + 2];
    __shared__ int s_cnt[128];          // 0..83 insert mers, 84..103 ext mers, 104..123 lig mers
    __shared__ double s_x[MIPGEN_N_FEATURES];
    __shared__ double s_red[CAND_THREADS / WAVE];
    __shared__ int s_info[16];

    const int tid = threadIdx.x;
    const auto en = list_entry(S, blockIdx.x);
    const int64_t oi = en.out;                            // where this workgroup's results go
    const int e = en.e, l = en.l, ss = en.ss;
    if (!en.valid) {
        if (tid == 0) {
            if (scores) scores[oi] = 0.0;
            if (records) records[oi] = 0;
        }
        if (features) for (int j = tid; j < MIPGEN_N_FEATURES; j += CAND_THREADS) features[oi * MIPGEN_N_FEATURES + j] = 0.0;
        if (ints_out && tid == 0) { mipgen_candidate_ints z = {}; ints_out[oi] = z; }
        return;
    }
    // wave 0 stages the arms and the integer record fields (design_mip, mipgen.cpp:606-760)
    if (tid < 128) s_cnt[tid] = 0;
    if (tid < WAVE) {
        const ArmInts a = en.stage_arms(s_ext, s_lig, tid);
        if (tid == 0) {
            s_info[0] = a.ext_copy; s_info[1] = a.lig_copy; s_info[2] = a.masked_n; s_info[3] = a.snp_count; s_info[4] = a.flags;
            s_info[5] = a.guard; s_info[6] = a.jc;
        }
    }
    __syncthreads();
    const int ext_copy = s_info[0], lig_copy = s_info[1];
    const bool guard = s_info[5] != 0;
    const int jc = s_info[6];

    // mer counts: the histogram of mip_features.h.  The oriented insert passes through LDS in pieces of MAX_INSERT bases (+ two of look-ahead for the
    // 2- / 3-mers that start in a piece): one piece for every realistic capture size, no limit on the others; the class-switch walk
    // (SVMipv4.cpp:118-142) of the logistic score carries its state across the pieces
    const bool want_run = ints_out || method == MIPGEN_SCORE_LOGISTIC;
    int run_last = -1, run_n = 0;
    for (int c0 = 0; c0 < ss; c0 += MAX_INSERT) {
        const int len = min(MAX_INSERT, ss - c0), lenx = min(len + 2, ss - c0);
        if (c0) __syncthreads();
        en.stage_insert(s_ins, c0, lenx, tid, CAND_THREADS);
        __syncthreads();
        hist_insert_piece(s_ins, len, lenx, s_cnt, tid, CAND_THREADS);
        if (tid == 0 && want_run) run_count_piece(s_ins, len, run_last, run_n);   // (a serial walk: only where it is used)
    }
    hist_arm(s_ext, e, s_cnt + 84, tid);
    hist_arm(s_lig, l, s_cnt + 104, tid);
    __syncthreads();

    // 192 features, SVMipv4.cpp:72-112
    if (tid < MIPGEN_N_FEATURES) {
        const int f = tid;
        const double v = mip_feature(f, s_cnt, e, l, ss, en.lrc, jc, ext_copy, lig_copy, guard, HC);
        s_x[f] = v;
        if (features) features[oi * MIPGEN_N_FEATURES + f] = v;
    }
    __syncthreads();

    // integer features + logistic score
    double logistic = 0.0;
    if (tid == 0) {
        const int eA = s_cnt[84 + 0], eC = s_cnt[84 + 5], eG = s_cnt[84 + 10], eT = s_cnt[84 + 15];
        const int lA = s_cnt[104 + 0], lC = s_cnt[104 + 5], lG = s_cnt[104 + 10], lT = s_cnt[104 + 15];
        const int tA = s_cnt[0], tC = s_cnt[21], tG = s_cnt[42], tT = s_cnt[63];
        const int run = want_run ? run_n + 1 : 1;
        if (ints_out) {
            mipgen_candidate_ints o;
            o.ext_a = eA; o.ext_c = eC; o.ext_g = eG; o.ext_t = eT;
            o.lig_a = lA; o.lig_c = lC; o.lig_g = lG; o.lig_t = lT;
            o.ins_a = tA; o.ins_c = tC; o.ins_g = tG; o.ins_t = tT;
            o.run_count = run; o.junction = jc; o.ext_copy = ext_copy; o.lig_copy = lig_copy;
            o.masked_n = s_info[2]; o.snp_count = s_info[3]; o.flags = s_info[4]; o.scan_size = ss;
            ints_out[oi] = o;
        }
        if (records) {
            records[oi] = pack_record(ext_copy, lig_copy, s_info[2], s_info[3], (uint32_t)s_info[4], (uint32_t)jc);
        }
        if (method == MIPGEN_SCORE_LOGISTIC) {
            if (guard) logistic = -1000.0;
            else {
                Vars x;
                const double dl = (double)e, ll = (double)l, dn = (double)ss;
                x.v[MLV_BPS] = dn / (double)run;
                x.v[MLV_TLEN] = ss > 250 ? 250.0 : dn;
                x.v[MLV_ELEN] = dl; x.v[MLV_LLEN] = ll;
                x.v[MLV_EGC] = ((double)eC + (double)eG) / dl; x.v[MLV_LGC] = ((double)lC + (double)lG) / ll; x.v[MLV_TGC] = ((double)tC + (double)tG) / dn;
                x.v[MLV_EG] = (double)eG / dl; x.v[MLV_LG] = (double)lG / ll; x.v[MLV_TG] = (double)tG / dn;
                x.v[MLV_EA] = (double)eA / dl; x.v[MLV_LA] = (double)lA / ll; x.v[MLV_TA] = (double)tA / dn;
                x.v[MLV_JS] = jc < 16 ? c_junction_scores[jc] : 0.0;
                x.v[MLV_LEC] = log_copy_dev(HC, ext_copy); x.v[MLV_LLC] = log_copy_dev(HC, lig_copy);
                const double ex = logistic_exponent_exact(x);                     // every operation rounded on its own, as the reference's
                // SVMipv4.cpp:247: pow(2.71828, ex), correctly rounded (pow_base_cr.h: glibc's own double in 99.9 % of cases; the device math library's pow in 91 %)
                const double y = fabs(ex) < 700.0 ? pow_base_cr(ex) : pow(MIPGEN_LOGISTIC_BASE, ex);
                logistic = y / (1.0 + y);
            }
            if (scores) scores[oi] = logistic;
        }
    }
    if (method != MIPGEN_SCORE_SVR || !scores) return;

    if (literal) {
        // the reference's own operation order (svm.cpp:329-368 k_function: d = x - y, sum += d * d in index order; :2511-2515 svm_predict_values:
        // sum += coef * k in support-vector order, then - rho), every operation rounded on its own (g++ on x86-64 does not contract to FMA):
        // what mipgen_accel prints for the scores that sit on a rounding boundary of the 6 printed digits (accel_score.hip: rescore).
        // Plain operators under `fp contract(off)`: HIP's __dmul_rn / __dadd_rn are plain operators compiled under contract(fast) - inlined, hipcc
        // fuses them into FMAs whatever the caller says.
#pragma clang fp contract(off)
        double total = 0.0;
        for (int base = 0; base < n_sv; base += CAND_THREADS) {
            const int i = base + tid;
            double term = 0.0;
            if (i < n_sv) {
                const double* sv = model + (int64_t)i * SV_ROW;
                double sum = 0.0;
                for (int j = 0; j < MIPGEN_N_FEATURES; j++) {
                    const double d = s_x[j] - sv[j];
                    const double dd = d * d;
                    sum = sum + dd;
                }
                sum = sum + sv[SVR_N_EXTRA];
                const double arg = -gamma * sum;
                const double k = exp(arg);
                term = sv[SVR_COEF] * k;
            }
            s_term[tid] = term;
            __syncthreads();
            if (tid == 0) { const int m = min(CAND_THREADS, n_sv - base); for (int q = 0; q < m; q++) total = total + s_term[q]; }
            __syncthreads();
        }
        if (tid == 0) scores[oi] = total - rho;
        return;
    }
    // SVR: lanes own support vectors; 192-dimension walk in index order, then shuffle reduction
    double part = 0.0;
    for (int i = tid; i < n_sv; i += CAND_THREADS) {
        const double* sv = model + (int64_t)i * SV_ROW;
        double sum = 0.0;
        for (int j = 0; j < MIPGEN_N_FEATURES; j++) {
            const double d = s_x[j] - sv[j];
            sum += d * d;
        }
        sum += sv[SVR_N_EXTRA];
        part += sv[SVR_COEF] * exp(-gamma * sum);
    }
    part = wave_sum_f64(part);
    if ((tid & (WAVE - 1)) == 0) s_red[tid / WAVE] = part;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < CAND_THREADS / WAVE; w++) s += s_red[w];
        scores[oi] = s - rho;
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_features_batch: the 192 features + the integer record of every entry of a LIST (the list scorer's front end: kernels_svr_gemm.hip).  Same
// values as k_candidates (SVMipv4.cpp:60-113, mipgen.cpp:606-760), through the same staging front and the same histogram.
//
// Mapping: ONE WAVEFRONT PER ENTRY, four entries per workgroup, nothing wider than a wave barrier.
//   * The work of an entry is its insert (tens to thousands of bases; the arms are 16-30): a 64-lane wavefront covers a 150-base insert in three
//     strides and a 1,200-base one in nineteen, with no idle waves - a 256-thread workgroup per entry would leave three of its four waves without
//     a base to count on a typical insert and pay four workgroup barriers per entry.
//   * Any insert length: the insert passes through LDS in pieces of MAX_INSERT bases + two of look-ahead (one piece for every realistic capture size).
//   * Wavefronts of a workgroup finish at different times only as far as their inserts differ.  Probes come with any mix of lengths, so the host
//     hands them over sorted by insert length (ProbeSrc::order, a counting sort): the four probes of a workgroup are of one length class and the
//     long ones start first - the tail of the launch is made of the shortest probes.
// Memory: an entry's bytes are read once, coalesced (lane i reads byte i); 1.5 KB of features are written per entry - for a 150-base insert the
// stores are 8x the loads, the kernel is bound by its feature stores.
// ---------------------------------------------------------------------------------------------------------
#define FB_WAVES 4

template <class Src>
__global__ __launch_bounds__(FB_WAVES * 64) void k_features_batch(int n, const Src S, const HostConsts* __restrict__ HC, uint64_t* __restrict__ records,
                                                                   double* __restrict__ features)
{
    __shared__ uint8_t s_ext_a[FB_WAVES][MIPGEN_MAX_OLIGO + 2], s_lig_a[FB_WAVES][MIPGEN_MAX_OLIGO + 2], s_ins_a[FB_WAVES][MAX_INSERT + 2];
    __shared__ int s_cnt_a[FB_WAVES][128];          // 0..83 insert mers, 84..103 ext mers, 104..123 lig mers
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = blockIdx.x * FB_WAVES + wave;
    if (wi >= n) return;
    uint8_t* s_ext = s_ext_a[wave]; uint8_t* s_lig = s_lig_a[wave]; uint8_t* s_ins = s_ins_a[wave];
    int* s_cnt = s_cnt_a[wave];
    const auto en = list_entry(S, wi);
    const int e = en.e, l = en.l, ss = en.ss;
    double* fo = features + en.out * MIPGEN_N_FEATURES;
    if (!en.valid) {
        if (lane == 0) records[en.out] = 0;
        for (int j = lane; j < MIPGEN_N_FEATURES; j += 64) fo[j] = 0.0;
        return;
    }
    s_cnt[lane] = 0; s_cnt[lane + 64] = 0;
    const ArmInts a = en.stage_arms(s_ext, s_lig, lane);
    if (lane == 0) records[en.out] = pack_record(a.ext_copy, a.lig_copy, a.masked_n, a.snp_count, (uint32_t)a.flags, (uint32_t)a.jc);
    for (int c0 = 0; c0 < ss; c0 += MAX_INSERT) {
        const int len = min(MAX_INSERT, ss - c0), lenx = min(len + 2, ss - c0);
        if (c0) wave_lds_sync();
        en.stage_insert(s_ins, c0, lenx, lane, 64);
        wave_lds_sync();
        hist_insert_piece(s_ins, len, lenx, s_cnt, lane, 64);
    }
    hist_arm(s_ext, e, s_cnt + 84, lane);
    hist_arm(s_lig, l, s_cnt + 104, lane);
    wave_lds_sync();
    // 192 features, SVMipv4.cpp:72-112 (the arithmetic of k_candidates, three features per lane)
    for (int f = lane; f < MIPGEN_N_FEATURES; f += 64)
        fo[f] = mip_feature(f, s_cnt, e, l, ss, en.lrc, a.jc, a.ext_copy, a.lig_copy, a.guard != 0, HC);
}

// ---------------------------------------------------------------------------------------------------------
// Dense index -> candidate: the one decode of every kernel below that turns a window-relative dense index (DevRegion::out_off is
// window-relative too; layout [position][capture size][strand][arm pair], mipgen_accel.h) into its candidate.  The region is the last of
// [r0, r1) with out_off <= idx: an empty region shares the offset of its successor and comes before it.  False where the index lies past
// the region's scan positions.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool dense_candidate(const DevParams* P, const DevRegion* regions, int r0, int r1, int64_t idx, mipgen_candidate& c)
{
    int lo = r0, hi = r1 - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (regions[mid].out_off <= idx) lo = mid; else hi = mid - 1; }
    const DevRegion& R = regions[lo];
    const int A = P->n_pairs;
    const int64_t local = idx - R.out_off, row = local / A, rest = row >> 1;
    const int a = (int)(local % A), ki = (int)(rest % R.n_sizes), pi = (int)(rest / R.n_sizes);
    c.region = lo; c.scan_start = R.first_pos + pi; c.capture_size = P->max_capture - (R.k0 + ki) * P->inc;
    c.ext_len = P->arm_ext[a]; c.lig_len = P->arm_lig[a]; c.strand = (int)(row & 1);
    return pi < R.n_pos;
}

// ---------------------------------------------------------------------------------------------------------
// The slow SVR route of the dense grid (parameter sets the tiled kernel of kernels_svr.hip cannot take: scan sizes below 3, more than
// 240 arm pairs, a tile beyond 160 KiB of LDS - the reference accepts any -arm_lengths / -capture_increment / range, mipgen.cpp:222-261,
// 427-444): the candidates of a chunk of the window's dense index range are written out as a LIST (k_dense_candidates) and go through the
// list scorer (k_features_batch + k_svr_gemm); k_dense_list_fix then applies the constants of the dense kernel's own fix-ups from the
// integer records, so that both routes hand out identical values for the flagged candidates.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dense_candidates(const DevParams* __restrict__ P, const DevRegion* __restrict__ regions, int r0, int r1, int64_t c0, int n,
                                                          mipgen_candidate* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mipgen_candidate c;
    dense_candidate(P, regions, r0, r1, c0 + i, c);
    out[i] = c;
}
__global__ __launch_bounds__(256) void k_dense_list_fix(int n, const uint64_t* __restrict__ records, double rho, double s_guard, double* __restrict__ scores)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t rec = records[i];
    if (score_is_constant(rec)) scores[i] = record_score(rec, 0.0, rho, s_guard);
}
extern "C" hipError_t mipgen_launch_dense_candidates(hipStream_t stream, const DevParams* P, const DevRegion* regions, int r0, int r1, int64_t c0, int n,
                                                     mipgen_candidate* out)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_dense_candidates, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, P, regions, r0, r1, c0, n, out);
    return hipGetLastError();
}
extern "C" hipError_t mipgen_launch_dense_list_fix(hipStream_t stream, int n, const uint64_t* records, double rho, double s_guard, double* scores)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_dense_list_fix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, records, rho, s_guard, scores);
    return hipGetLastError();
}

// the list kernels over either source of S
extern "C" hipError_t mipgen_launch_features_batch(hipStream_t stream, int n, const ListSrc& S, const HostConsts* HC, uint64_t* records, double* features)
{
    if (n <= 0) return hipSuccess;
    const dim3 grid((n + FB_WAVES - 1) / FB_WAVES), block(FB_WAVES * 64);
    if (S.kind == LIST_PROBES) hipLaunchKernelGGL(k_features_batch<ProbeSrc>, grid, block, 0, stream, n, S.probes, HC, records, features);
    else hipLaunchKernelGGL(k_features_batch<BatchSrc>, grid, block, 0, stream, n, S.batch, HC, records, features);
    return hipGetLastError();
}
extern "C" hipError_t mipgen_launch_candidates(hipStream_t stream, int n, const ListSrc& S, const HostConsts* HC, const double* model, int n_sv, double gamma, double rho,
                                               int method, double* scores, uint64_t* records, double* features, mipgen_candidate_ints* ints, int literal,
                                               const unsigned int* n_dev)
{
    if (n <= 0) return hipSuccess;
    if (S.kind == LIST_PROBES)
        hipLaunchKernelGGL(k_candidates<ProbeSrc>, dim3(n), dim3(CAND_THREADS), 0, stream, S.probes, HC, model, n_sv, gamma, rho, method, scores, records, features, ints,
                           literal, n_dev);
    else
        hipLaunchKernelGGL(k_candidates<BatchSrc>, dim3(n), dim3(CAND_THREADS), 0, stream, S.batch, HC, model, n_sv, gamma, rho, method, scores, records, features, ints,
                           literal, n_dev);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Scores on a rounding boundary of the printed digits.  The front end prints scores with 6 significant digits (mipgen.cpp:774: default
// ostream precision); a dense SVR score differs from the reference's double by ~1e-12 (another summation order, table factors), so a
// score within that distance of a midpoint between two 6-digit numbers could print another last digit.  k_print_boundary_scan lists the
// entries whose score lies within tol of such a midpoint (scores the record fixes carry exact constants and are skipped) - entries of a
// window's dense grid, of a candidate list or of a window's condensed survivors (RescoreSrc); they are re-scored by k_candidates in the
// reference's own operation order and written back (k_scatter_scores).
// ---------------------------------------------------------------------------------------------------------

// distance of |s| to the nearest midpoint between two 6-significant-digit decimal numbers (what "%g" / the default ostream precision prints,
// mipgen.cpp:774), relative test against tol: decade from the binary exponent + a table for 1e-13 .. 1e13, log10 / pow outside
__device__ __forceinline__ bool near_print_midpoint(double s, double tol_rel, double tol_abs)
{
    const double a = fabs(s);
    if (!(a > 1e-300) || !(a < 1e300)) return false;                        // 0, NaN, inf
    double unit;
    if (a >= 1e-8 && a < 1e8) {
        constexpr double P10[32] = {1e-15, 1e-14, 1e-13, 1e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1e0,
                                    1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16};
        const int e2 = (int)((__double2hiint(a) >> 20) & 0x7FF) - 1023;
        int e10 = (e2 * 1233) >> 12;                                        // ~ floor(e2 * log10(2)), off by at most one
        if (a < P10[e10 + 15]) e10--; else if (a >= P10[e10 + 16]) e10++;
        unit = P10[e10 + 10];                                               // 10^(e10 - 5)
    } else {
        int e10 = (int)floor(log10(a));
        unit = pow(10.0, (double)(e10 - 5));
        const double t0 = a / unit;
        if (t0 >= 1e6) unit *= 10.0; else if (t0 < 1e5) unit *= 0.1;        // log10 rounding at powers of ten
    }
    const double t = a / unit;
    const double frac = t - floor(t);
    return fabs(frac - 0.5) * unit <= tol_rel * a + tol_abs;
}

// out_idx[k]: entry i of the source (a dense index, a list position, a survivor slot).  The midpoint test comes first: only entries near a
// midpoint read their record.  The dense-grid scan runs over every candidate of a non-silent window: grid-stride, its grid capped by the
// launch; the list and survivor scans take one entry per thread (a loop there more than doubles their VGPRs).
template <int KIND>
__global__ __launch_bounds__(256) void k_print_boundary_scan(const DevParams* __restrict__ P, const DevRegion* __restrict__ regions, int r0, int r1, int64_t n,
                                                             const double* __restrict__ scores, const uint64_t* __restrict__ records,
                                                             const mipgen_candidate* __restrict__ cands, const mipgen_survivor* __restrict__ surv, int64_t cand0,
                                                             double tol_rel, double tol_abs, mipgen_candidate* __restrict__ out, int64_t* __restrict__ out_idx,
                                                             unsigned int* __restrict__ count, unsigned int cap)
{
    auto scan = [&](int64_t i) {
        uint64_t rec;
        int64_t idx = i;                                                    // the window-relative dense index of a DENSE / SURV entry
        if constexpr (KIND == RESCORE_SURV) {
            const mipgen_survivor sv = surv[i];
            if (sv.cand_index < 0 || !near_print_midpoint(sv.score, tol_rel, tol_abs)) return;
            rec = sv.record; idx = sv.cand_index - cand0;
        } else {
            if (!near_print_midpoint(scores[i], tol_rel, tol_abs)) return;
            rec = records[i];
        }
        if (score_is_constant(rec)) return;
        mipgen_candidate c;
        if constexpr (KIND != RESCORE_LIST && KIND != RESCORE_PROBES) { if (!dense_candidate(P, regions, r0, r1, idx, c)) return; }
        const unsigned int at = atomicAdd(count, 1u);
        if (at >= cap) return;
        if constexpr (KIND == RESCORE_LIST) out[at] = cands[i]; else if constexpr (KIND != RESCORE_PROBES) out[at] = c;
        out_idx[at] = i;
    };
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (KIND == RESCORE_DENSE) { for (int64_t i = i0; i < n; i += (int64_t)gridDim.x * blockDim.x) scan(i); }
    else if (i0 < n) scan(i0);
}

// dense indices of a window -> candidates: the saturated logistic candidates the dense kernel listed
__global__ __launch_bounds__(256) void k_index_candidates(const DevParams* __restrict__ P, const DevRegion* __restrict__ regions, int r0, int r1, const int64_t* __restrict__ idx_list,
                                                          const unsigned int* __restrict__ count, unsigned int cap, mipgen_candidate* __restrict__ out)
{
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || i >= *count) return;
    mipgen_candidate c;
    dense_candidate(P, regions, r0, r1, idx_list[i], c);
    out[i] = c;
}

// re-scored values back where they came from: entry i of the list -> dst[idx[i]] (a score array or the score field of a survivor).  n_dev: the
// list length on the device (null: cap); `over` (host-mapped word, may be null): set when the scan listed more entries than the list holds -
// the surplus was not re-scored, the caller reports it
__device__ __forceinline__ double& score_at(double* d, int64_t i) { return d[i]; }
__device__ __forceinline__ double& score_at(mipgen_survivor* d, int64_t i) { return d[i].score; }
template <typename T>
__global__ __launch_bounds__(256) void k_scatter_scores(const double* __restrict__ src, const int64_t* __restrict__ idx, int64_t cap, const unsigned int* __restrict__ n_dev,
                                                        T* __restrict__ dst, unsigned int* __restrict__ over)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = n_dev ? (int64_t)*n_dev : cap;
    if (i < cap && i < n) score_at(dst, idx[i]) = src[i];
    if (i == 0 && over && n > cap) *over = (unsigned int)(n - cap);
}

extern "C" hipError_t mipgen_launch_print_boundary_scan(hipStream_t stream, const DevParams* P, const DevRegion* regions, const RescoreSrc* s, double tol_rel,
                                                        double tol_abs, mipgen_candidate* out, int64_t* out_idx, unsigned int* count, unsigned int cap, int n_cu)
{
    if (s->n <= 0 || (s->kind != RESCORE_LIST && s->kind != RESCORE_PROBES && s->r1 <= s->r0)) return hipSuccess;
    const int64_t want = (s->n + 255) / 256;
    const unsigned grid = (unsigned)(s->kind == RESCORE_DENSE ? std::min<int64_t>(want, (int64_t)std::max(n_cu, 1) * 16) : want);
#define SCAN(K) hipLaunchKernelGGL(k_print_boundary_scan<K>, dim3(grid), dim3(256), 0, stream, P, regions, s->r0, s->r1, s->n, s->scores, s->records, s->cands, \
                                   s->surv, s->cand0, tol_rel, tol_abs, out, out_idx, count, cap)
    switch (s->kind) {
        case RESCORE_DENSE: SCAN(RESCORE_DENSE); break;
        case RESCORE_LIST: SCAN(RESCORE_LIST); break;
        case RESCORE_SURV: SCAN(RESCORE_SURV); break;
        case RESCORE_PROBES: SCAN(RESCORE_PROBES); break;
        default: return hipErrorInvalidValue;
    }
#undef SCAN
    return hipGetLastError();
}
extern "C" hipError_t mipgen_launch_index_candidates(hipStream_t stream, const DevParams* P, const DevRegion* regions, int r0, int r1, const int64_t* idx, const unsigned int* count,
                                                     unsigned int cap, mipgen_candidate* out)
{
    if (cap == 0) return hipSuccess;
    hipLaunchKernelGGL(k_index_candidates, dim3((cap + 255) / 256), dim3(256), 0, stream, P, regions, r0, r1, idx, count, cap, out);
    return hipGetLastError();
}
// one of dst / dst_surv
extern "C" hipError_t mipgen_launch_scatter_scores(hipStream_t stream, const double* src, const int64_t* idx, int64_t cap, const unsigned int* n_dev, double* dst,
                                                   mipgen_survivor* dst_surv, unsigned int* over)
{
    if (cap <= 0) return hipSuccess;
    const dim3 grid((unsigned)((cap + 255) / 256));
    if (dst_surv) hipLaunchKernelGGL(k_scatter_scores<mipgen_survivor>, grid, dim3(256), 0, stream, src, idx, cap, n_dev, dst_surv, over);
    else hipLaunchKernelGGL(k_scatter_scores<double>, grid, dim3(256), 0, stream, src, idx, cap, n_dev, dst, over);
    return hipGetLastError();
}

// ---- every condensed survivor of a window as a candidate list, in slot order (mixed designs: the pick stage re-scores survivors with the SVR,
// mipgen.cpp:1523-1527,1873-1877 - all of them are scored here in one list call and the selection stage looks the values up) ----
__global__ __launch_bounds__(256) void k_surv_keep(const mipgen_survivor* __restrict__ surv, int64_t n, int64_t* __restrict__ keep, double* __restrict__ svr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    keep[i] = (i < n && surv[i].cand_index >= 0) ? 1 : 0;
    if (i < n) svr[i] = __longlong_as_double(0x7ff8000000000000ll);         // NaN: no survivor in this slot
}
__global__ __launch_bounds__(256) void k_surv_candidates(const DevParams* __restrict__ P, const DevRegion* __restrict__ regions, int r0, int r1,
                                                         const mipgen_survivor* __restrict__ surv, int64_t n, int64_t cand0, const int64_t* __restrict__ offs,
                                                         mipgen_candidate* __restrict__ out, int64_t* __restrict__ out_idx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mipgen_survivor sv = surv[i];
    if (sv.cand_index < 0) return;
    mipgen_candidate c;
    dense_candidate(P, regions, r0, r1, sv.cand_index - cand0, c);         // (cand_index is batch-wide)
    const int64_t at = offs[i];
    out[at] = c; out_idx[at] = i;
}
extern "C" hipError_t mipgen_launch_surv_keep(hipStream_t stream, const mipgen_survivor* surv, int64_t n, int64_t* keep, double* svr)
{
    hipLaunchKernelGGL(k_surv_keep, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, stream, surv, n, keep, svr);
    return hipGetLastError();
}
extern "C" hipError_t mipgen_launch_surv_candidates(hipStream_t stream, const DevParams* P, const DevRegion* regions, int r0, int r1, const mipgen_survivor* surv,
                                                    int64_t n, int64_t cand0, const int64_t* offs, mipgen_candidate* out, int64_t* out_idx)
{
    if (n <= 0 || r1 <= r0) return hipSuccess;
    hipLaunchKernelGGL(k_surv_candidates, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, P, regions, r0, r1, surv, n, cand0, offs, out, out_idx);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Featurev5::get_long_range_content (/root/reference/Featurev5.cpp:18-56; mers mipgen.cpp:32)
// ---------------------------------------------------------------------------------------------------------
// one workgroup per region: LDS histogram of the 1/2/3-mers of its extended sequence, then the 44 frequencies
__global__ __launch_bounds__(256) void k_long_range(const char* __restrict__ seqs, const int64_t* __restrict__ offs, const int32_t* __restrict__ lens,
                                                    const int32_t* __restrict__ denoms, LrcMers M, double* __restrict__ out_all)
{
    __shared__ int c1[4], c2[16], c3[64];
    const int tid = threadIdx.x;
    const char* seq = seqs + offs[blockIdx.x];
    const int len = lens[blockIdx.x], denom = denoms[blockIdx.x];
    double* out = out_all + (int64_t)blockIdx.x * MIPGEN_N_LRC;
    if (tid < 4) c1[tid] = 0;
    if (tid < 16) c2[tid] = 0;
    if (tid < 64) c3[tid] = 0;
    __syncthreads();
    auto code = [](char ch) { return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4; };
    for (int i = tid; i < len; i += 256) {
        const int b0 = code(seq[i]);
        if (b0 > 3) continue;
        atomicAdd(&c1[b0], 1);
        if (i + 1 >= len) continue;
        const int b1 = code(seq[i + 1]);
        if (b1 > 3) continue;
        atomicAdd(&c2[4 * b0 + b1], 1);
        if (i + 2 >= len) continue;
        const int b2 = code(seq[i + 2]);
        if (b2 > 3) continue;
        atomicAdd(&c3[16 * b0 + 4 * b1 + b2], 1);
    }
    __syncthreads();
    if (tid < MIPGEN_N_LRC) {
        const int k = M.k[tid];
        auto cnt = [&](int cd) { return k == 1 ? c1[cd] : (k == 2 ? c2[cd] : c3[cd]); };
        double fwd = (double)cnt(M.code[tid]);
        if (M.rc[tid] >= 0) out[tid] = (fwd + (double)cnt(M.rc[tid])) / denom;      // Featurev5.cpp:49
        else out[tid] = fwd / denom;                                                // :53
    }
}

extern "C" hipError_t mipgen_launch_long_range(hipStream_t stream, int n, const char* seqs, const int64_t* offs, const int32_t* lens,
                                               const int32_t* denoms, const LrcMers* M, double* out_dev)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_long_range, dim3(n), dim3(256), 0, stream, seqs, offs, lens, denoms, *M, out_dev);
    return hipGetLastError();
}

