// mip_bounds.h — the bounds skips of mipgen.cpp:443-444 (the record's MIPGEN_FLAG_VALID), once, in the three forms the dense-grid kernels use.  Every function
// is __host__ __device__ and reads nothing but its integer arguments, so a plain C++ program can include this file without HIP (tests/bounds_host.cpp does,
// under the sanitizers, and compares the forms over a whole box of arguments: tests/test_bounds_cpu.py).
//
// A candidate is the scan start p (1-based chromosome coordinate), the capture size C and the arm pair (e, l); seq_stop is the last coordinate of the
// region's sequence.  All quantities are far below 2^30: no sum or difference here can overflow an int.
#pragma once

#if defined(__HIPCC__)
#define BOUNDS_HD __host__ __device__ static inline
#else
#define BOUNDS_HD static inline
#endif

BOUNDS_HD int bounds_min(int a, int b) { return a < b ? a : b; }
BOUNDS_HD int bounds_max(int a, int b) { return a > b ? a : b; }

// ---- the literal rule: :443-444 as the reference writes it, and a non-empty scan target (ss = C - e - l > 0) --------------------------------------------
BOUNDS_HD bool constructed(int seq_stop, int p, int C, int e, int l)
{
    const int ss = C - e - l;
    return !(p - e <= 0 || p - l <= 0) && !(p + C - e - 1 > seq_stop || p + C - l - 1 > seq_stop) && ss > 0;
}

// ---- the row form (k_logistic_dense: one (p, C) row per wavefront pass, lanes on the pairs) ----------------------------------------------------------------
// The literal rule, clause by clause:  p - e <= 0 || p - l <= 0  <=>  p <= max(e, l);  with over = p + C - 1 - seq_stop ("the arms must be longer than
// this"),  p + C - e - 1 > seq_stop || p + C - l - 1 > seq_stop  <=>  over > e || over > l  <=>  over > min(e, l);  ss > 0  <=>  C > e + l.  Hence the lane
// test below equals the literal rule.  The uniform test replaces max(e, l), min(e, l) and e + l by bounds over the whole pair list (arm_hi >= every arm,
// arm_lo <= every arm, max_sum >= every e + l): where it holds, the lane test holds for every pair - a row this far inside the region needs no lane test.
// k_logistic_dense takes `over` from row_over and writes the two compare chains below out at its call site, operand for operand: there the uniform chain is a
// short circuit that ends in a load (P->max_sum) and stays a scalar branch around the lane compares; as calls the chains are flattened and every row pays the
// lane compares (k_logistic_dense + 2.3 %, measured: DESIGN 4.1).  tests/test_gpu_bounds_edges.py holds the kernel's text to the rule where it cuts.
BOUNDS_HD int row_over(int seq_stop, int p, int C) { return p + C - 1 - seq_stop; }
BOUNDS_HD bool row_all_constructed(int p, int C, int over, int arm_hi, int arm_lo, int max_sum) { return p > arm_hi && over <= arm_lo && C > max_sum; }
BOUNDS_HD bool row_lane_constructed(int p, int C, int over, int e, int l) { return p > bounds_max(e, l) && over <= bounds_min(e, l) && C > e + l; }

// ---- the span form (k_replay_condense_narrow: one (position, pair) per lane, a row per capture size) -------------------------------------------------------
// By the clauses above a pair is constructed at p for exactly the capture sizes e + l < C <= c_lim, c_lim = seq_stop - p + 1 + min(e, l), provided
// p > max(e, l).  In x = C - (e + l) - 1 that is 0 <= x <= c_span, c_span = c_lim - (e + l) - 1, and for c_span >= 0 the two compares are the one unsigned
// compare (unsigned)x <= (unsigned)c_span (a negative x wraps above every non-negative int); c_span < 0 means no capture size fits and is part of ok_lo.
// bounds_span is computed once per (position, pair); the row of size index ki has x = span_top(largest C) - ki * inc.
struct BoundsSpan { bool ok_lo; int c_span; };
BOUNDS_HD BoundsSpan bounds_span(int seq_stop, int p, int e, int l)
{
    const int c_lim = seq_stop - p + 1 + bounds_min(e, l);                  // largest capture size that still fits
    const int c_span = c_lim - (e + l) - 1;
    return BoundsSpan{p > bounds_max(e, l) && c_span >= 0, c_span};
}
BOUNDS_HD int span_top(int C_top, int e, int l) { return C_top - (e + l) - 1; }
BOUNDS_HD bool span_constructed(bool ok_lo, int c_span, int x) { return ok_lo && (unsigned)x <= (unsigned)c_span; }
