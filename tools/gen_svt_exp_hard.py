#!/usr/bin/env python3
"""Writes tests/golden/svt_exp_hard.txt: of 400,000 uniform arguments in [-110, 0] (fixed seed) the 4,096 whose exp lies closest to the midpoint of two
doubles, one hex double per line, hardest first.  These are the arguments where an exp that is merely accurate to an ulp rounds the other way; the tests
hold svt_exp_cr to the correctly rounded value there (tests/test_svt_exp_cpu.py on the host, tests/test_gpu_svt_kernels.py on the device).  stdlib only."""
import math
import os
import random
from decimal import Decimal, localcontext

N, KEEP, SEED = 400000, 4096, 20240613


def main():
    rnd = random.Random(SEED)
    scored = []
    with localcontext() as ctx:
        ctx.prec = 60
        for _ in range(N):
            v = rnd.uniform(-110.0, 0.0)
            e = Decimal(v).exp()
            f = float(e)
            off = abs(e - Decimal(f)) / Decimal(math.ulp(f))        # 0 .. 0.5: the distance from the nearest double, in ulps
            scored.append((float(off), v))
    scored.sort(reverse=True)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "svt_exp_hard.txt")
    with open(out, "w") as fh:
        for off, v in scored[:KEEP]:
            fh.write(v.hex() + "\n")
    print(f"{out}: {KEEP} arguments, distance from a midpoint at most {0.5 - scored[KEEP - 1][0]:.2e} ulp")


if __name__ == "__main__":
    main()
