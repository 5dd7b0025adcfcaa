"""GPU: variant calls from synthetic count tables through mipgen_accel_call_tables, against tests/call_ref.py - plain loops and the exact integer
binomial tail - by exact equality of the totals and of every record, after the one exclusion the model allows: a candidate whose exact score lies within 1e-6 of
an integer (or of the cap) is dropped from both sides, and each test asserts that at most 1 in 1,000 of its candidates is.  Every call is made twice and must
return the same bytes.  The tables of every test come from one generator and one oracle pass per case (module cache)."""
import faulthandler

import numpy as np
import pytest

from mipgen_amd import capi
from tests import call_ref as CR

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE = -1, -6
CAP = capi.CALL_MAX_DEPTH


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test's device work runs under a time limit of its own: a stuck call ends the process with a traceback instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def acc():
    a = capi.Accel(capi.make_params(130, 140))
    yield a
    a.close()


def c_params(p):
    return capi.CallParams(**p)


def set_cell(counts, columns, x, r, a, n, k):
    """Position x: depth n, k of it on allele class a, the rest on the ref class r; the columns outside the depth get noise that must not matter."""
    counts[x] = 0
    counts[x][5 if a == 4 else a] = k
    counts[x][r] += n - k
    counts[x][4] = (x * 7) % 5                                             # discordant
    if columns == 8:
        counts[x][6], counts[x][7] = (x * 3) % 4, x % 2                    # ins, ins_discordant


def random_tables(n_pos, columns, seed, dirty):
    """A table of every kind of cell: depths 1-300 and a few of 5,000; alt counts 0, at min_alt, one above expectation, near the mean and k = n; two alts at some
    positions; refs in both cases and some that are no base.  dirty: a pool with alt fractions from 1e-4 to 0.3 instead of the bare prior."""
    rng = np.random.default_rng(seed)
    counts = np.zeros((n_pos, columns), dtype=np.int32)
    pool = np.zeros((n_pos, 10), dtype=np.int32)
    ref = bytearray(n_pos)
    n_alleles = CR.alleles(columns)
    for x in range(n_pos):
        r = int(rng.integers(0, 4))
        ref[x] = b"ACGTacgtN-"[r + (4 if x % 11 == 3 else 0)] if x % 29 != 7 else b"N-"[x % 2]
        n = 5000 if x % 997 == 5 else int(rng.integers(1, 301))
        a = int((r + 1 + rng.integers(0, n_alleles - 1)) % n_alleles)
        if dirty:
            N = int(rng.integers(1, 2_000_000))
            frac = float(rng.choice([1e-4, 1e-3, 1e-2, 0.2, 0.3]))
            pool[x][:5] = rng.binomial(N, frac, 5)
            pool[x][5:] = N
            if x % 5 == 0:
                pool[x][5:] += rng.integers(0, 1000, 5)                    # the depths of the pool differ per allele class
        e = (int(pool[x][a]) + 3) / (int(pool[x][5 + a]) + 2999)                # (the prior of the test that uses these tables)
        kind = x % 7
        mean = n * e
        k = {0: 0, 1: 3, 2: int(mean) + 1, 3: int(mean + (mean * (1 - e)) ** 0.5) + 1, 4: n, 5: int(rng.integers(0, n + 1)), 6: max(3, int(mean * 1.5))}[kind]
        k = min(k, n)
        set_cell(counts, columns, x, r, a, n, k)
        if x % 13 == 0 and n - k >= 6:                                     # a second alt at the same position
            b = next(c for c in range(n_alleles) if c not in (r, a))
            counts[x][5 if b == 4 else b] += 3 + x % 3
            counts[x][r] -= 3 + x % 3
    return counts, pool, bytes(ref)


_oracle_cache = {}


def oracle(key, counts, pool, ref, own, p, **kw):
    if key not in _oracle_cache:
        _oracle_cache[key] = CR.call_cells(counts, pool, ref, own, p, **kw)
    return _oracle_cache[key]


def check(acc, key, counts, pool, ref, own, p, max_excluded_per_mille=1):
    """The device against the oracle: totals and records exactly, the band's cells dropped from both sides; twice, the same bytes.  Returns (records, oracle cells)."""
    totals, cands = oracle(key, counts, pool, ref, own, p)
    assert totals["excluded"] * 1000 <= max_excluded_per_mille * max(totals["candidates"], 1), (key, totals)
    got, got_totals = acc.call_tables(counts, pool, ref, own, c_params(p))
    again, again_totals = acc.call_tables(counts, pool, ref, own, c_params(p))
    assert got.tobytes() == again.tobytes() and got_totals == again_totals
    assert {k: got_totals[k] for k in ("tested", "too_deep", "candidates")} == {k: totals[k] for k in ("tested", "too_deep", "candidates")}, key
    want = CR.kept_calls(cands, p)
    assert CR.drop_excluded(got, cands) == want, key
    if not totals["excluded"]:
        assert got_totals["calls"] == totals["calls"] == len(got)
    keys = [(int(r["pos"]), int(r["allele"])) for r in got]
    assert keys == sorted(set(keys))                                       # ascending (pos, allele), no cell twice
    return got, cands


@pytest.mark.parametrize("columns", [5, 8])
@pytest.mark.parametrize("n_pos", [1, 63, 64, 65, 257, 4099])
def test_sizes_shapes_depths_and_backgrounds(acc, n_pos, columns):
    """Every table size around a wavefront and a block, both table shapes, the bare prior and a dirty pool, the row inside and outside the pool."""
    seen = 0
    for dirty in (False, True):
        counts, pool, ref = random_tables(n_pos, columns, 7000 + n_pos + columns + dirty, dirty)
        own = bool(dirty) != (columns == 8)
        p = CR.params(min_depth=4, min_alt=2, min_ppm=1000 if dirty else 0, min_q=13, a0=3, n0=2999, bg_max_ppm=250000)   # (no power of ten: k = n would score an integer)
        if own:                                                            # the row is a sample row: what of it qualifies is part of the pool it is called against
            pool = pool + CR.pool([counts], p["bg_max_ppm"])
        got, cands = check(acc, ("sizes", n_pos, columns, dirty), counts, pool, ref, own, p)
        seen += len(cands)
        if n_pos == 4099:
            assert len(cands) > 1500 and 100 < len(got) < len(cands)
            assert any(c["depth"] == 5000 and c["alt"] > 100 for c in cands) and any(c["alt"] == c["depth"] for c in cands)
            if columns == 8:
                assert any(c["allele"] == 4 for c in cands)
    assert n_pos < 63 or seen > 0


def test_chosen_cells(acc):
    """One position per named case: k at min_alt and one below; k one above expectation and at it; mean + 1 sigma at n = 5,000 and e about 0.2 (hundreds of terms);
    k = n small and deep; a score that reaches the cap; a non-base ref; depth at min_depth and one below."""
    p = CR.params(min_depth=20, min_alt=3, min_ppm=0, min_q=0, a0=1, n0=997, bg_max_ppm=1000000)
    cells = [  # (n, k, K, N, ref byte)
        (100, 3, 0, 0, b"A"), (100, 2, 0, 0, b"A"),                                                         # 0 at min_alt, 1 below it
        (2990, 3, 0, 0, b"C"), (2991, 3, 0, 0, b"C"), (2000, 3, 0, 0, b"C"),                                # 2 just above expectation (3 x 997 > 2990), 3 at it, 4 above
        (5000, 1029, 199999, 999003, b"G"), (5000, 1001, 199999, 999003, b"G"), (5000, 1000, 199999, 999003, b"G"), (5000, 1300, 199999, 999003, b"g"),
        (3, 3, 0, 0, b"T"), (20, 20, 0, 0, b"T"), (5000, 5000, 0, 0, b"T"), (4000, 3500, 0, 0, b"T"),       # 9 below min_depth, 10 k = n, 11 and 12 beyond the cap of the score
        (500, 40, 5, 100000, b"N"), (500, 40, 5, 100000, b"a"),                                             # 13 no base, 14 a lower-case one
        (20, 5, 0, 0, b"A"), (19, 5, 0, 0, b"A"),                                                           # 15 at min_depth, 16 below
    ]                                                                                                       # (5..8: e = 200,000 / 1,000,000, mean 1,000, sigma 28.3; 7 is AT expectation)
    for columns in (5, 8):
        n_pos = len(cells)
        counts = np.zeros((n_pos, columns), dtype=np.int32)
        pool = np.zeros((n_pos, 10), dtype=np.int32)
        ref = b"".join(c[4] for c in cells)
        for x, (n, k, K, N, rb) in enumerate(cells):
            r = max(CR.ref_class(rb[0]), 0)
            a = 4 if columns == 8 and x % 2 else (r + 1) % 4
            set_cell(counts, columns, x, r, a, n, k)
            pool[x][a], pool[x][5 + a] = K, N
        got, cands = check(acc, ("chosen", columns), counts, pool, ref, False, p, max_excluded_per_mille=0)
        by_pos = {c["pos"]: c for c in cands}
        assert sorted(by_pos) == [0, 2, 4, 5, 6, 8, 10, 11, 12, 14, 15]
        assert by_pos[11]["q"] == by_pos[12]["q"] == CR.Q_CAP and by_pos[10]["q"] == 599                    # (20 x 10 log10 997 = 599.7)
        assert 0 < by_pos[5]["q"] < 10 and by_pos[6]["q"] < by_pos[5]["q"] and by_pos[8]["q"] > 20


def test_the_depth_cap(acc):
    """n = cap is tested, n = cap + 1 is too deep.  Only these two cells are deep; the oracle is asked for the filters there, and the score of the cell at the cap
    is known in closed form: every molecule shows the alt, so P = e^n, far beyond the cap of the score."""
    p = CR.params(min_depth=1, min_alt=1, min_q=0)
    for columns in (5, 8):
        counts = np.zeros((3, columns), dtype=np.int32)
        pool = np.zeros((3, 10), dtype=np.int32)
        set_cell(counts, columns, 0, 0, 1, CAP, CAP)
        set_cell(counts, columns, 1, 0, 1, CAP + 1, CAP + 1)
        set_cell(counts, columns, 2, 0, 1, 50, 0)
        totals, cands = CR.call_cells(counts, pool, b"AAA", False, p, filters_only=True)
        assert totals["tested"] == 2 and totals["too_deep"] == 1 and [(c["pos"], c["allele"]) for c in cands] == [(0, 1)]
        for _ in range(2):
            got, got_totals = acc.call_tables(counts, pool, b"AAA", False, c_params(p))
            assert got_totals == {"tested": 2, "too_deep": 1, "candidates": 1, "calls": 1}
            assert got.tolist() == [(0, 1, CAP, CAP, 0, 0, CR.Q_CAP)]


@pytest.mark.parametrize("columns", [5, 8])
def test_all_cells_candidates_and_none(acc, columns):
    """Every alt class of every position a candidate - the candidate list at its worst case, 3 or 4 per position - and the same table with no candidate at all."""
    n_pos, n_alt = 321, CR.alleles(columns) - 1
    rng = np.random.default_rng(7100 + columns)
    counts = np.zeros((n_pos, columns), dtype=np.int32)
    counts[:, :4] = rng.integers(30, 60, (n_pos, 4))
    if columns == 8:
        counts[:, 5:] = rng.integers(30, 60, (n_pos, 3))
    ref = bytes(rng.choice(list(b"ACGT"), n_pos).astype(np.uint8))
    p = CR.params(min_depth=1, min_alt=1, min_q=0)
    pool = CR.pool([counts], p["bg_max_ppm"])                              # the row itself is the whole pool: leave-one-out leaves the prior alone
    got, cands = check(acc, ("all", columns), counts, pool, ref, True, p)
    assert len(cands) == n_alt * n_pos == len(got)
    none = CR.params(min_depth=1, min_alt=61, min_q=0)
    got, got_totals = acc.call_tables(counts, pool, ref, True, c_params(none))
    assert len(got) == 0 and got_totals == {"tested": n_pos, "too_deep": 0, "candidates": 0, "calls": 0}
    nothing_tested = CR.params(min_depth=10 ** 6)
    assert acc.call_tables(counts, pool, ref, True, c_params(nothing_tested))[1] == {"tested": 0, "too_deep": 0, "candidates": 0, "calls": 0}


@pytest.mark.parametrize("n_cand", [0, 1, 15, 16, 17, 65])
def test_the_order_of_the_records(acc, n_cand):
    """0, 1, 15, 16, 17 and 65 candidates - none, one group of lanes, a full block of quarter wavefronts less one, full, one more, several blocks - scattered over 200
    positions: the records come in ascending (pos, allele), and only the calls among them."""
    rng = np.random.default_rng(7200 + n_cand)
    n_pos = 200
    counts = np.zeros((n_pos, 8), dtype=np.int32)
    pool = np.zeros((n_pos, 10), dtype=np.int32)
    ref = b"ACGT" * 50
    for x in range(n_pos):
        set_cell(counts, 8, x, x % 4, (x + 1) % 4, 60 + x, 0)
    cells = sorted(rng.choice(n_pos * 2, n_cand, replace=False).tolist())
    for c in cells:                                                        # two alt classes per position may be taken: a base and del
        x, second = divmod(c, 2)
        a = 4 if second else (x + 1) % 4
        k = 3 + c % 4                                                      # (3 of 60 under the prior alone scores 37: k = 3..6 straddles min_q = 45)
        counts[x][5 if a == 4 else a] += k
        counts[x][x % 4] -= k
    p = CR.params(min_depth=20, min_alt=3, min_q=45)
    got, cands = check(acc, ("order", n_cand), counts, pool, ref, False, p)
    assert len(cands) == n_cand
    if n_cand >= 15:
        assert 0 < len(got) < n_cand


def test_refusals(acc):
    counts = np.zeros((4, 5), dtype=np.int32)
    pool = np.zeros((4, 10), dtype=np.int32)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)
    lib, h, C = acc.lib, acc.h, capi.C
    i32p = C.POINTER(C.c_int32)
    tot = capi.CallTotals(-7, -7, -7, -7)
    good = CR.params()

    def call(counts_=counts, columns=5, pool_=pool, ref_=ref, n_pos=4, params=good, handle=h):
        prm = c_params(params) if params is not None else None
        return lib.mipgen_accel_call_tables(handle, counts_.ctypes.data_as(i32p) if counts_ is not None else None, columns,
                                            pool_.ctypes.data_as(i32p) if pool_ is not None else None, ref_.ctypes.data if ref_ is not None else None, n_pos, 0,
                                            C.byref(prm) if prm is not None else None, C.byref(tot))

    fresh = capi.Accel(capi.make_params(130, 140))
    try:                                                                   # a handle that never called holds no records
        assert fresh.lib.mipgen_accel_call_fetch(fresh.h, None, 0) == E_STATE and b"holds no calls" in lib.mipgen_accel_last_error()
    finally:
        fresh.close()
    bad = [dict(counts_=None), dict(pool_=None), dict(ref_=None), dict(params=None), dict(columns=4), dict(columns=6), dict(columns=0), dict(n_pos=0), dict(n_pos=-1),
           dict(n_pos=1 << 29), dict(handle=None)]
    for key, values in dict(min_depth=(0, -1), min_alt=(0,), min_ppm=(-1, 10 ** 6 + 1), bg_max_ppm=(-1, 10 ** 6 + 1), min_q=(-1, 10000), a0=(0, -1, 1000, 2000),
                            n0=((1 << 30) + 1, 0)).items():
        bad += [dict(params=CR.params(**{key: v})) for v in values]
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
    assert call(params=CR.params(min_q=10000)) == E_INVALID and b"min_q 10000" in lib.mipgen_accel_last_error()
    assert (tot.tested, tot.calls) == (-7, -7)
    # the limits themselves are accepted
    for ok in (dict(min_ppm=10 ** 6), dict(bg_max_ppm=0), dict(min_q=9999), dict(a0=(1 << 30) - 1, n0=1 << 30), dict(min_q=0, min_ppm=0)):
        assert call(params=CR.params(**ok)) == 0, ok
    assert tot.calls == 0 and lib.mipgen_accel_call_fetch(h, None, 0) == 0
    assert lib.mipgen_accel_call_fetch(h, None, 1) == E_INVALID and lib.mipgen_accel_call_fetch(None, None, 0) == E_INVALID
    # timing: off, nothing booked; on, the kernels of the last call
    assert acc.last_kernel_ms(13) < 0
    acc.set_timing(True)
    counts[:, 0], counts[:, 1] = 50, 5
    records, totals = acc.call_tables(counts, pool, b"AAAA", False, c_params(good))
    assert acc.last_kernel_ms(13) > 0 and totals["calls"] == 4 == len(records)
    buf = np.zeros(3, dtype=capi.CALL_RECORD_DTYPE)
    assert lib.mipgen_accel_call_fetch(h, buf.ctypes.data, 3) == E_INVALID and lib.mipgen_accel_call_fetch(h, None, 4) == E_INVALID
    acc.set_timing(False)
    acc.call_tables(counts, pool, b"AAAA", False, c_params(good))
    assert acc.last_kernel_ms(13) < 0
