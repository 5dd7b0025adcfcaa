// svt_exp.h — exp(v) for the SVR trainer's RBF kernel (kernels_svr_train.hip), in a header of its own so that the host can be held against a
// correctly rounded reference (tests/svt_exp_host.cpp, tests/test_svt_exp_cpu.py) with the very text the device compiles.
#pragma once
#include <math.h>
#include "pow_base_cr.h"

// exp(v) correctly rounded for the RBF argument (v <= 0 up to rounding): argument reduction by ln 2 (k * L2H exact), exp of r / 16 by its Taylor
// series in double-double, four squarings (the construction of pow_base_cr, pow_base_cr.h).  Below -110 the float of the result is 0 either way.
// Computed under `fp contract(off)` (g++: -ffp-contract=off), as the helpers of pow_base_cr.h are.
PBC_FN double svt_exp_cr(double v)
{
    PBC_EXACT
    if (v != v) return v;
    if (v < -110.0) return 0.0;
    if (v > 709.0) return HUGE_VAL;
    const double L2H = 0x1.62e42fefa3000p-1, L2M = 0x1.3de6af278ece6p-42, L2L = 0x1.f97b57a079a19p-103, INVLN2 = 0x1.71547652b82fep+0;
    const double kd = nearbyint(v * INVLN2);
    pbc_dd r = pbc_two_sum(v, -kd * L2H);                     // exact product
    r = pbc_add(r, pbc_two_prod(-kd, L2M));
    r = pbc_add_d(r, -kd * L2L);
    r.h *= 0.0625; r.l *= 0.0625;
    pbc_dd s = {1.0, 0.0};
    for (int m = 18; m >= 1; m--) {
        s = pbc_mul(s, r);
        const double inv = 1.0 / (double)m;
        pbc_dd q = pbc_mul_d(s, inv);
        pbc_dd back = pbc_mul_d(q, (double)m);
        const double err = ((s.h - back.h) - back.l) + s.l;
        q = pbc_add_d(q, err * inv);
        s = pbc_add_d(q, 1.0);
    }
    for (int i = 0; i < 4; i++) s = pbc_mul(s, s);
    return ldexp(s.h, (int)kd);
}
