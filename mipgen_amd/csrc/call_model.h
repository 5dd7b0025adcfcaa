// call_model.h — the variant-calling model of DESIGN 4.14 as the pieces the kernels of kernels_call.hip are made of: the depth and the allele count of a count-table
// row, the qualification rule of the background, the leave-one-out subtraction, the four integer filters, one term of the binomial tail in log space and the
// scalar tail.  Every piece is __host__ __device__ and reads nothing but its arguments, so a plain C++ program can include this file without HIP
// (tests/call_host.cpp does, under the sanitizers).
//
// Integers.  Counts are the int32 columns of a pileup row; the sums K, N of the pool are int32 as well: a count is at most the groups of a cell, the pool adds the
// same cell over the sample rows, and a session holds fewer than 2^31 groups in all.  Every product of the filters is taken in int64: k, n <= 2^31, 10^6 < 2^20 and
// N_o + n0 < 2^31 + 2^30, so a product stays below 2^63.
//
// Accuracy of the score.  Q = floor(-10 log10 P), P = sum_{i=k..n} C(n,i) e^i (1-e)^(n-i), e = A / B with the integers A = K_o + a0 and B = N_o + n0.  The tail
// is summed in log space: ln P = lt_k + ln S, S = sum exp(lt_i - lt_k), lt_i = lnfact(n) - lnfact(i) - lnfact(n-i) + i ln(A/B) + (n-i) ln((B-A)/B).
//  - ln(1-e) is taken as the logarithm of the exact integer B - A over B, not as log1p(-e): A / B rounded first would lose everything when e is close to 1.  Both
//    logarithms carry one rounding of the quotient and one of log: at most 2.3e-16 absolute each, times i + (n-i) = n.
//  - lnfact: a table of the correctly rounded ln(m!) for m < 32; above it Stirling's series (m + 1/2) ln m - m + ln(2 pi)/2 + 1/(12m) - 1/(360m^3) + 1/(1260m^5)
//    - 1/(1680m^7), whose first dropped term 1/(1188 m^9) is below 3e-17 at m = 32.  Its error is that of the product (m + 1/2) ln m: about 2 roundings of
//    1.1e-16 relative to m ln m.
//  - a candidate lies strictly above expectation (k B > n A), so the terms fall from i = k on: t_{i+1} / t_i = (n-i) A / ((i+1)(B-A)) < 1 and falling.  The sum
//    stops once a term is below 2^-60 of the running sum; what is left is at most that term over 1 - ratio, and the ratio is by then far below 1 (at the depth cap
//    and e = 1/2 it is 0.98: 2^-54 relative).  S >= 1, every exp argument is <= 0, and ln S adds a few 1e-16.
//  At the depth cap n = 2^20 the magnitudes that meet in lt_k - three lnfact of up to 1.4e7, two products of up to 2.2e7 - sum to about 7e7; some six roundings of
//  1.1e-16 of that are 5e-8 in natural-log units, 2e-7 in phred units (x 4.34), below the band of 1e-6 around an integer within which the tests do not compare.
//  MIPGEN_CALL_MAX_DEPTH exists so that this holds: do not raise it without redoing the sum.
//  What is compared.  Up to n = 5,000 the tests hold an exact integer sum (tests/call_ref.py::exact_phred); there the magnitudes sum to 2e5 and the error is
//  6e-10.  From there to the cap the reference is hp_phred of the same file: the sum over every term in fixed point with 320 fractional bits, the logarithms in
//  80-digit decimal, good to 1e-70 and equal to the exact sum to 6e-11 where both exist.  tests/golden/call_sharp_cells.json (tools/call_sharp_cells.py) holds, for
//  each of the depths 200, 5,000, 5,001, 2^14, 2^16, 2^18, 2^20 - 1, 2^20 and each background near 1e-3, 1e-2, 0.3, 0.5, 0.9, a candidate whose score lies 2e-6 to
//  2e-5 above an integer and one as far below - an error of either sign beyond 2e-6 flips a floor - plus k = n - 17 .. n under e = 0.999 (the last round of lanes
//  runs into i > n) and e = (B - 1) / B at B = 10^6 and 2^31 - 1 + 2^30.  The host functions of this file stay within 8e-9 of hp_phred on all of them (4.9e-13 at
//  n = 200, 4e-11 at 5,001, 3.5e-10 at 2^16, 1.3e-9 at 2^18, 8e-9 at 2^20: a twenty-fifth of the 2e-7 bounded above, the roundings partly cancelling), and
//  k_call_tail returns the floor of hp_phred for every one, in every position of the wavefront and beside neighbours of any length
//  (tests/test_call_cpu.py, tests/test_gpu_call_deep.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CALL_HD __host__ __device__ static inline
#else
#define CALL_HD static inline
#endif

#ifndef MIPGEN_CALL_MAX_DEPTH
#define MIPGEN_CALL_MAX_DEPTH (1 << 20)   // (include/mipgen_accel.h states the same number)
#endif
#define CALL_ALLELES 5               // A, C, G, T, del
#define CALL_Q_CAP 9999
#define CALL_MILLION 1000000ll

// the seven numbers of mipgen_call_params, as the kernels take them
struct CallModel { int32_t min_depth, min_alt, min_ppm, min_q, a0, n0, bg_max_ppm; };

// 0..3 for A C G T in either case, -1 for anything else: such a position is never tested
CALL_HD int call_ref_class(uint8_t ref)
{
    switch (ref & 0xDF) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return -1; }
}

// the count of allele class a in a row of `columns` (5: A C G T discordant; 8: ... del ins ins_discordant) numbers; del exists in the gapped table only
CALL_HD int32_t call_allele_count(const int32_t* row, int columns, int a) { return a < 4 ? row[a] : columns == 8 ? row[5] : 0; }
CALL_HD int call_alleles(int columns) { return columns == 8 ? 5 : 4; }
// the depth: A + C + G + T, plus del in the gapped table; discordant is in neither
CALL_HD int64_t call_depth(const int32_t* row, int columns) { return (int64_t)row[0] + row[1] + row[2] + row[3] + (columns == 8 ? row[5] : 0); }

// a row belongs to the background of (x, a) if it has depth there and its alt fraction is at most bg_max_ppm
CALL_HD bool call_qualifies(int64_t k, int64_t n, int32_t bg_max_ppm) { return n > 0 && k * CALL_MILLION <= (int64_t)bg_max_ppm * n; }

// the pool without the row being called: its own k, n leave K, N when the row is a sample row that qualified
CALL_HD void call_leave_one_out(int64_t K, int64_t N, int64_t k, int64_t n, bool own_row_is_sample, int32_t bg_max_ppm, int64_t* K_o, int64_t* N_o)
{
    const bool in_pool = own_row_is_sample && call_qualifies(k, n, bg_max_ppm);
    *K_o = in_pool ? K - k : K;
    *N_o = in_pool ? N - n : N;
}

CALL_HD bool call_depth_tested(int64_t n, const CallModel& P) { return n >= P.min_depth && n <= MIPGEN_CALL_MAX_DEPTH; }

// the four integer filters of a cell whose depth is tested
CALL_HD bool call_candidate(int64_t k, int64_t n, int64_t K_o, int64_t N_o, const CallModel& P)
{
    return call_depth_tested(n, P) && k >= P.min_alt && k * CALL_MILLION >= (int64_t)P.min_ppm * n && k * (N_o + P.n0) > n * (K_o + P.a0);
}

CALL_HD double call_lnfact(int64_t m)
{
    static constexpr double T[32] = {
        0x0.0p+0, 0x0.0p+0, 0x1.62e42fefa39efp-1, 0x1.cab0bfa2a2002p+0, 0x1.96ca77c922cf9p+1, 0x1.326643c4479c9p+2, 0x1.a51273acf01cap+2, 0x1.10ce1f32dcc30p+3,
        0x1.5358e82fcb70dp+3, 0x1.99a8921a7f7cfp+3, 0x1.e357590954d15p+3, 0x1.180973f3a8d74p+4, 0x1.3fcba16d50143p+4, 0x1.68d5a9c3b32cep+4, 0x1.930f3df162a42p+4,
        0x1.be636a63fd346p+4, 0x1.eabff061f1a84p+4, 0x1.0c0a63f2f353ap+5, 0x1.2329df2d5ee52p+5, 0x1.3ab8153363985p+5, 0x1.52af57aed77bep+5, 0x1.6b0a8643472a9p+5,
        0x1.83c4faba84f06p+5, 0x1.9cda78b856a45p+5, 0x1.b6472034e8d14p+5, 0x1.d007622cd65e7p+5, 0x1.ea17f717c6794p+5, 0x1.023aeb67e4fefp+6, 0x1.0f8f18d330240p+6,
        0x1.1d07353917231p+6, 0x1.2aa208b59d0e5p+6, 0x1.385e6fd9e5a40p+6};
    if (m < 32) return T[m < 0 ? 0 : m];
    const double x = (double)m, r = 1.0 / x, r2 = r * r;
    const double series = r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0))));
    return (x + 0.5) * log(x) - x + 0x1.d67f1c864beb4p-1 + series;      // (ln(2 pi) / 2)
}

// what every term of one tail shares: ln e, ln(1 - e) and lnfact(n), from the integers A = K_o + a0 < B = N_o + n0
struct CallTail { int64_t n; double ln_e, ln_1e, lnfact_n; };
CALL_HD CallTail call_tail_of(int64_t n, int64_t A, int64_t B) { return {n, log((double)A / (double)B), log((double)(B - A) / (double)B), call_lnfact(n)}; }
// lt_i
CALL_HD double call_log_term(const CallTail& T, int64_t i)
{
    return T.lnfact_n - call_lnfact(i) - call_lnfact(T.n - i) + (double)i * T.ln_e + (double)(T.n - i) * T.ln_1e;
}
// Q from lt_k and S = sum exp(lt_i - lt_k)
CALL_HD int32_t call_q_of(double lt_k, double S)
{
    const double phred = -(lt_k + log(S)) * 0x1.15f2ced384f28p+2;       // (10 / ln 10)
    return phred >= (double)CALL_Q_CAP ? CALL_Q_CAP : phred <= 0.0 ? 0 : (int32_t)floor(phred);
}
CALL_HD double call_phred_of(double lt_k, double S) { return -(lt_k + log(S)) * 0x1.15f2ced384f28p+2; }

// The scalar tail: the terms one after the other, each computed on its own as the lanes of k_call_tail compute theirs, until a term falls below 2^-60 of the sum.
// *phred (may be NULL): the score before the floor and the cap.
CALL_HD int32_t call_tail_q(int64_t k, int64_t n, int64_t A, int64_t B, double* phred)
{
    const CallTail T = call_tail_of(n, A, B);
    const double lt_k = call_log_term(T, k);
    double S = 1.0;
    for (int64_t i = k + 1; i <= n; i++) {
        const double t = exp(call_log_term(T, i) - lt_k);
        S += t;
        if (t < S * 0x1p-60) break;
    }
    if (phred) *phred = call_phred_of(lt_k, S);
    return call_q_of(lt_k, S);
}
