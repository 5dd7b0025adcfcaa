"""fmt_g6.h on the host: the routine that prints every score of the all_mips file (k_fmt_records) is `__host__ __device__`, so the same text compiles
with the host compiler.  A small shim over it is built at test time and held, by exact equality, against printf("%g") as CPython restates it
(tests/fmt_cases.py): every crafted value and two million random bit patterns.  The device side of the same routine: tests/test_gpu_format.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import fmt_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mipgen_amd", "csrc")
CXX = os.environ.get("CXX", "g++")                       # the compiler of tests/stub_accel/Makefile

SHIM = r"""
#include "fmt_g6.h"
static const Pow10DD tab[] = POW10_DD_TABLE;
extern "C" int fmt_g6_host(double v, char* out) { return fmt_g6(v, out, tab); }
// n values into 16-byte slots, zero padded (fmt_g6 writes at most 16 bytes, no terminator)
extern "C" void fmt_g6_host_many(const double* v, long n, char* out)
{
    for (long i = 0; i < n; i++) {
        char* o = out + 16 * i;
        const int k = fmt_g6(v[i], o, tab);
        for (int j = k; j < 16; j++) o[j] = 0;
    }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("fmt_g6")
    src, so = d / "fmt_g6_host.cpp", d / "libfmt_g6_host.so"
    src.write_text(SHIM)
    r = subprocess.run([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so), "-lm"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    lib = C.CDLL(str(so))
    lib.fmt_g6_host.argtypes = [C.c_double, C.c_char_p]
    lib.fmt_g6_host.restype = C.c_int
    lib.fmt_g6_host_many.argtypes = [C.POINTER(C.c_double), C.c_long, C.c_char_p]
    lib.fmt_g6_host_many.restype = None
    return lib


def _printed(lib, values):
    v = np.ascontiguousarray(values, dtype=np.float64)
    out = C.create_string_buffer(16 * v.shape[0])
    lib.fmt_g6_host_many(v.ctypes.data_as(C.POINTER(C.c_double)), v.shape[0], out)
    return np.frombuffer(out.raw, dtype="S16")


def _require_equal(values, got, want):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{bad.size} of {len(values)} differ", [(float(values[i]).hex(), bytes(got[i]), bytes(want[i])) for i in bad[:10]])


def test_crafted_cases_are_what_they_claim():
    """The shared case list holds the values the device test relies on: no repeated bit pattern, both NaNs, the named singles, and expected() is
    printf("%g") on the cases whose text is known by heart."""
    v = FC.crafted()
    bits = v.view(np.uint64)
    assert np.unique(bits).size == bits.size > 20000
    for b in (FC.NAN_NEGATIVE_BITS, FC.NAN_POSITIVE_BITS, 0x8000000000000000, 0x0000000000000001, 0x7FF0000000000000, 0xFFF0000000000000):
        assert (bits == np.uint64(b)).sum() == 1, hex(b)
    for x in FC.SINGLES + (123456.5, float(np.nextafter(123456.5, 0.0)), float(np.nextafter(123456.5, np.inf)), 1234565e17):
        assert (bits == np.float64(x).view(np.uint64)).sum() == 1, x
    known = [(0.0, b"0"), (-0.0, b"-0"), (float("inf"), b"inf"), (float("-inf"), b"-inf"), (5e-324, b"4.94066e-324"), (123456.5, b"123456"),
             (123457.5, b"123458"), (float(np.nextafter(123456.5, np.inf)), b"123457"), (999999.5, b"1e+06"), (999999.49999999994, b"999999"),
             (0.0001, b"0.0001"), (0.000099999949, b"9.99999e-05"), (1e5, b"100000"), (1e6, b"1e+06"), (1.7976931348623157e308, b"1.79769e+308"),
             (2.2250738585072014e-308, b"2.22507e-308"), (float("nan"), b"-nan"), (-float("nan"), b"-nan"), (1.5e-7, b"1.5e-07")]
    for x, s in known:
        assert FC.expected(x) == s, (x, FC.expected(x), s)
    lens = {len(s) for s in FC.expected_all(v)}
    assert lens == set(range(1, 14)), lens                 # "0" .. "-1.23456e-308": every printed length a wave scan can meet


def test_single_call_entry(shim):
    """The one-value entry point (returned length, nothing written past it) on the singles."""
    for x in FC.SINGLES + (float("nan"), -float("nan")):
        buf = C.create_string_buffer(b"#" * 24, 24)
        n = shim.fmt_g6_host(x, buf)
        assert buf.raw[:n] == FC.expected(x) and buf.raw[n:] == b"#" * (24 - n), (x, buf.raw)


def test_fmt_g6_crafted_values(shim):
    """Every crafted value, none left out: ties of the `k < 0 && k >= -22` branch and their neighbours, the carry into the next decade, both notation
    switches, three-digit exponents, denormals (two table factors), -0, inf, both NaNs."""
    v = FC.crafted()
    _require_equal(v, _printed(shim, v), np.array(FC.expected_all(v), dtype="S16"))


def test_fmt_g6_random_bit_patterns(shim):
    """2e6 seeded random bit patterns (all exponents, denormals and infinities among them; NaN payloads other than the two crafted ones are skipped)."""
    bits = np.random.default_rng(20240607).integers(0, 2 ** 64, size=2_000_000, dtype=np.uint64, endpoint=False)
    v = bits.view(np.float64)
    v = v[~np.isnan(v)]
    assert v.size > 1_990_000
    _require_equal(v, _printed(shim, v), np.array(FC.expected_all(v), dtype="S16"))
