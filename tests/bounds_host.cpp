// Host side of mipgen_amd/csrc/mip_bounds.h, compiled on its own by tests/test_bounds_cpu.py (g++, under the address and undefined-behaviour sanitizers):
// the three forms of the bounds skips against the rule as mipgen.cpp:443-444 states it, over the whole box
//     e, l in 1..12, C in 1..40, p in -2..48, seq_stop in {30, 31, 45}
// with no case left out.  Prints one "name value" line per counter; the test asserts on them.
#include <cstdio>
#include "../mipgen_amd/csrc/mip_bounds.h"

// the two `continue`s of mipgen.cpp:443-444 in the reference's own words, and the empty scan target the kernels add
static bool skipped_by_the_reference(int seq_stop, int p, int C, int e, int l)
{
    if (p - e <= 0 || p - l <= 0) return true;
    if (p + C - e - 1 > seq_stop || p + C - l - 1 > seq_stop) return true;
    return C - e - l <= 0;
}

int main()
{
    const int stops[3] = {30, 31, 45}, incs[3] = {1, 2, 5};
    long cases = 0, n_constructed = 0, n_small_C = 0, n_low_p = 0, n_small_C_else_ok = 0;
    long bad_literal = 0, bad_lane = 0, span_cases = 0, bad_span = 0;
    for (int s = 0; s < 3; s++)
        for (int e = 1; e <= 12; e++)
            for (int l = 1; l <= 12; l++)
                for (int C = 1; C <= 40; C++)
                    for (int p = -2; p <= 48; p++) {
                        const int seq_stop = stops[s];
                        const bool want = !skipped_by_the_reference(seq_stop, p, C, e, l);
                        cases++;
                        n_constructed += want;
                        n_small_C += C <= e + l;
                        n_low_p += p <= 0;
                        // the clause the span form once lacked decides: everything else lets the candidate through
                        n_small_C_else_ok += C <= e + l && !(p - e <= 0 || p - l <= 0) && !(p + C - e - 1 > seq_stop || p + C - l - 1 > seq_stop);
                        bad_literal += constructed(seq_stop, p, C, e, l) != want;
                        bad_lane += row_lane_constructed(p, C, row_over(seq_stop, p, C), e, l) != want;
                        // the span form as k_replay_condense_narrow evaluates it: C is the capture size of row ki below the largest one
                        const BoundsSpan sp = bounds_span(seq_stop, p, e, l);
                        for (int i = 0; i < 3; i++)
                            for (int ki = 0; ki <= 7; ki++) {
                                const int c_inc = incs[i], c_top = span_top(C + ki * c_inc, e, l);
                                span_cases++;
                                bad_span += span_constructed(sp.ok_lo, sp.c_span, c_top - ki * c_inc) != want;
                            }
                    }
    // the uniform test of the row form: whenever it says "every pair of this row is constructed", every pair of a list whose arms lie in
    // [a_lo, a_hi] and whose sums do not exceed max_sum is
    long uniform_cases = 0, uniform_all = 0, uniform_pairs = 0, bad_uniform = 0;
    for (int a_lo = 1; a_lo <= 12; a_lo++)
        for (int a_hi = a_lo; a_hi <= 12; a_hi++)
            for (int max_sum = 2 * a_lo; max_sum <= 2 * a_hi; max_sum++)
                for (int s = 0; s < 3; s++)
                    for (int C = 1; C <= 40; C++)
                        for (int p = -2; p <= 48; p++) {
                            const int seq_stop = stops[s];
                            uniform_cases++;
                            if (!row_all_constructed(p, C, row_over(seq_stop, p, C), a_hi, a_lo, max_sum)) continue;
                            uniform_all++;
                            for (int e = a_lo; e <= a_hi; e++)
                                for (int l = a_lo; l <= a_hi; l++) {
                                    if (e + l > max_sum) continue;
                                    uniform_pairs++;
                                    bad_uniform += skipped_by_the_reference(seq_stop, p, C, e, l);
                                }
                        }
    printf("cases %ld\nconstructed %ld\nsmall_C %ld\nsmall_C_else_ok %ld\nlow_p %ld\nbad_literal %ld\nbad_lane %ld\nspan_cases %ld\nbad_span %ld\n", cases, n_constructed,
           n_small_C, n_small_C_else_ok, n_low_p, bad_literal, bad_lane, span_cases, bad_span);
    printf("uniform_cases %ld\nuniform_all %ld\nuniform_pairs %ld\nbad_uniform %ld\n", uniform_cases, uniform_all, uniform_pairs, bad_uniform);
    return fflush(stdout) != 0 ? 2 : 0;
}
