"""CPU: svt_exp_cr (mipgen_amd/csrc/svt_exp.h), the exp of the SVR trainer's RBF kernel, against a correctly rounded reference.  The header is host-compiled
into the stand-alone program tests/svt_exp_host.cpp (g++ -ffp-contract=off, under the address and undefined-behaviour sanitizers); the reference is
float(Decimal(v).exp()) at 60 digits - stdlib decimal rounds exp correctly to the context's precision, and 60 digits leave a double's rounding decided for
every argument here.  The comparison is exact equality of the double for every argument; none is left out."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.svt_ref import exp_cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = math.log(2.0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is what the host tools are built with"
    out = str(tmp_path_factory.mktemp("svt_exp") / "svt_exp_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-o", out, os.path.join(ROOT, "tests", "svt_exp_host.cpp")], check=True)
    return out


def device_text_on_host(exe, values):
    text = "".join(float(v).hex() + "\n" for v in values)
    p = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    got = [float.fromhex(t) if t not in ("nan", "-nan", "inf", "-inf") else float(t.replace("-nan", "nan")) for t in p.stdout.decode().split()]
    assert len(got) == len(values)
    return got


def neighbours(c, width=2):
    """c and the `width` doubles on either side of it"""
    out, lo, hi = [c], c, c
    for _ in range(width):
        lo = math.nextafter(lo, -math.inf); hi = math.nextafter(hi, math.inf)
        out += [lo, hi]
    return out


def negative_arguments():
    rng = np.random.default_rng(20240611)
    vals = list(rng.uniform(-110.0, 0.0, 20000))
    vals += list(-(10.0 ** rng.uniform(-20.0, 0.0, 2000)))
    for k in range(-1, -159, -1):                            # where nearbyint(v / ln 2) flips, and the multiples of ln 2 / 2 between
        vals += [v for v in neighbours(k * LN2 / 2) if v >= -110.0]
    vals += [-0.0, 0.0, -110.0, math.nextafter(-110.0, 0.0), -1e-300, -5e-324]
    return [float(v) for v in vals]


def positive_arguments():
    rng = np.random.default_rng(20240612)
    vals = list(rng.uniform(0.0, 709.0, 5000))
    vals += list(10.0 ** rng.uniform(-20.0, 0.0, 1000))
    for k in range(1, 1023):
        vals += [v for v in neighbours(k * LN2 / 2) if v <= 709.0]
    vals += [709.0, math.nextafter(709.0, 0.0), 1e-300, 5e-324, 1.0, 0.5]
    return [float(v) for v in vals]


def compare(exe, vals):
    got = device_text_on_host(exe, vals)
    bad = [(v.hex(), g.hex(), exp_cr(v).hex()) for v, g in zip(vals, got) if g != exp_cr(v)]
    assert not bad, f"{len(bad)} of {len(vals)} arguments differ (argument, svt_exp_cr, correctly rounded): {bad[:10]}"


def test_negative_arguments_are_correctly_rounded(exe):
    vals = negative_arguments()
    assert len(vals) > 22000 and min(vals) == -110.0
    compare(exe, vals)


def test_positive_arguments_are_correctly_rounded(exe):
    vals = positive_arguments()
    assert max(vals) == 709.0
    compare(exe, vals)


def test_arguments_next_to_a_rounding_midpoint(exe):
    """tests/golden/svt_exp_hard.txt: the 4,096 of 400,000 arguments in [-110, 0] whose exp lies closest to the midpoint of two doubles
    (tools/gen_svt_exp_hard.py)"""
    vals = [float.fromhex(t) for t in open(os.path.join(ROOT, "tests", "golden", "svt_exp_hard.txt")).read().split()]
    assert len(vals) == 4096 and all(-110.0 <= v <= 0.0 for v in vals)
    compare(exe, vals)


def test_special_cases(exe):
    below = [math.nextafter(-110.0, -math.inf), -111.0, -745.0, -1e308, -math.inf]
    above = [math.nextafter(709.0, math.inf), 710.0, 1e308, math.inf]
    got = device_text_on_host(exe, [math.nan] + below + above)
    assert math.isnan(got[0])
    assert all(g == 0.0 and math.copysign(1.0, g) == 1.0 for g in got[1:1 + len(below)]), got
    assert all(g == math.inf for g in got[1 + len(below):]), got
    # the reference follows the same three rules, so that the kernels' models need not repeat them
    assert math.isnan(exp_cr(math.nan)) and exp_cr(-110.00001) == 0.0 and exp_cr(709.5) == math.inf
