"""The doubles at which a printf("%g") written by hand goes wrong, and what the C library prints for them: shared by tests/test_fmt_cpu.py (fmt_g6.h
compiled for the host) and tests/test_gpu_format.py (the same routine inside k_fmt_records).  Plain Python / numpy, no device.

  crafted()    exact ties of the 6-digit rounding and their one-ulp neighbours, the 999999.5 -> 1e+06 carry, both sides of the switches between fixed
               and exponent notation, every decade from the smallest denormal to the largest double, signed zeros, infinities and two NaNs
  expected(v)  the bytes printf("%g", v) gives: CPython's float formatting is correctly rounded, as glibc's is
"""
import numpy as np

TIE_N = (100000, 100001, 123456, 123457, 250001, 500000, 999998, 999999)       # 6-digit integers: both parities, both ends of the decade
DECADE_F = ("1", "0.9999995", "0.99999949999", "0.9999994", "9.999995", "9.9999949", "1.000005", "1.0000005", "0.5", "0.1234565", "0.1234575")
SINGLES = (0.0, -0.0, float("inf"), float("-inf"), 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 0.0001, 0.00009999995, 999999.5,
           999999.49999999994, 1e5, 1e6, 99999.95)
NAN_NEGATIVE_BITS = 0xFFF8000000000000                                          # what inf - inf leaves on x86: the sign bit set
NAN_POSITIVE_BITS = 0x7FF8000000000000

_crafted = None


def _with_neighbours(v):
    a = np.asarray(v, dtype=np.float64)
    away = np.where(np.signbit(a), -np.inf, np.inf)
    return np.concatenate([a, np.nextafter(a, 0.0), np.nextafter(a, away)])


def crafted() -> np.ndarray:
    """float64 array without repeated bit patterns (computed once; callers must not write to it)."""
    global _crafted
    if _crafted is not None:
        return _crafted
    ties = []
    for n in TIE_N:
        for j in range(23):
            ties.append(((2 * n + 1) * 10 ** j) / 2)                            # (N + 1/2) * 10^j: int / int is correctly rounded, exact while it fits 53 bits
        for m in range(1, 21):
            ties.append((2 * n + 1) / 2 ** (m + 1))                             # (N + 1/2) / 2^m: exact
    decades = []
    for e in range(-323, 309):
        for f in DECADE_F:
            x = float(f"{f}e{e}")                                               # correctly rounded from the decimal string; 9.99..e308 is inf, 0.12..e-323 is 0
            decades += [x, -x]
    p = 2.2250738585072014e-308
    vals = np.concatenate([_with_neighbours(ties), _with_neighbours(decades), np.array(SINGLES + (float(np.nextafter(p, 0.0)),)),
                           np.array([NAN_NEGATIVE_BITS, NAN_POSITIVE_BITS], dtype=np.uint64).view(np.float64)])
    bits = vals.view(np.uint64)
    _, first = np.unique(bits, return_index=True)
    out = vals[np.sort(first)].copy()
    out.setflags(write=False)
    _crafted = out
    return out


def expected(v) -> bytes:
    """printf("%g", v); every NaN prints "-nan" (the contract stated in fmt_g6.h)."""
    v = float(v)
    if v != v:
        return b"-nan"
    return b"%g" % v


def expected_all(values) -> list:
    return [expected(x) for x in np.asarray(values, dtype=np.float64).tolist()]
