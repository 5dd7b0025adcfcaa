"""GPU: insertion calls from host arrays (mipgen_accel_insertion_call_tables, mipgen_accel_insertion_call_fetch).  Synthetic allele records, spans and
sparse pools; every comparison is exact equality of the records and the totals with tests/insertion_call_ref.py, and every call is made twice and returns the same
bytes.  A candidate whose exact score lies within 1e-6 of an integer or of the cap is dropped from both sides, and at most 1 in 1,000 candidates of a test may be;
the scores are exact integer sums (depths of a few hundred), the fixture's high-precision strings for the sharp cells up to the depth cap."""
import decimal
import faulthandler
import json
import math
import os

import numpy as np
import pytest

from mipgen_amd import capi
from tests import call_ref as CR
from tests import insertion_call_ref as IC
from tests import insertion_ref as I

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE = -1, -6
CAP = CR.MAX_DEPTH
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_sharp_cells.json")
P0 = CR.params(min_depth=20, min_alt=3, min_ppm=0, min_q=30, a0=1, n0=1000, bg_max_ppm=200000)


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


def keyof(a, ambiguous=False):
    return I.key(a[0], a[1], ambiguous, a[2])


def records_of(items):
    """INSERTION_RECORD_DTYPE in ascending key order from (allele, count, ambiguous) items."""
    items = sorted(items, key=lambda it: keyof(it[0], it[2]))
    out = np.zeros(len(items), dtype=capi.INSERTION_RECORD_DTYPE)
    for i, (a, k, amb) in enumerate(items):
        out[i] = (a[0], a[1], k, 0 if amb else a[2], int(amb))
    return out


def pool_of(items):
    """INSERTION_POOL_RECORD_DTYPE in ascending key order from (allele, K, X) items."""
    items = sorted(items, key=lambda it: keyof(it[0]))
    out = np.zeros(len(items), dtype=capi.INSERTION_POOL_RECORD_DTYPE)
    for i, (a, K, X) in enumerate(items):
        out[i] = (a[0], a[1], a[2], K, X)
    return out


def check(acc, records, span, pool, S, own, p, score=CR.exact_phred, budget=None):
    """One tables call, twice, against the oracle; (device records, oracle candidates).  budget: a [candidates, excluded] pair the caller sums over its calls."""
    params = capi.CallParams(**p)
    got, totals = acc.insertion_call_tables(records, span, pool, S, own, params)
    again, totals2 = acc.insertion_call_tables(records, span, pool, S, own, params)
    assert got.tobytes() == again.tobytes() and totals == totals2 and got.dtype == capi.INSERTION_CALL_RECORD_DTYPE
    assert acc.insertion_call_fetch(len(got)).tobytes() == got.tobytes()
    w_totals, cands = IC.call_cells(IC.Row(np.asarray(span, dtype=np.int32), records), IC.pool_lookup(pool, S), own, p, score)
    assert {k: totals[k] for k in ("tested", "too_deep", "candidates")} == {k: w_totals[k] for k in ("tested", "too_deep", "candidates")}, (totals, w_totals)
    assert IC.drop_excluded(got, cands) == IC.kept_calls(cands, p)
    assert w_totals["calls"] <= totals["calls"] <= w_totals["calls"] + w_totals["excluded"] and not got["reserved"].any()
    if budget is None:
        assert w_totals["excluded"] * 1000 <= w_totals["candidates"], w_totals
    else:
        budget[0] += w_totals["candidates"]; budget[1] += w_totals["excluded"]
    return got, cands


def random_allele(rng, n_pos):
    l = int(rng.choice([1, 1, 2, 3, 15]))
    return int(rng.integers(0, n_pos)), l, int(rng.integers(0, 4 ** l))


def generated(rng, n_records, n_pool, n_pos, shared=0.5, ambiguous=(), own_bg=None):
    """A row of n_records records over n_pos anchors and a pool of n_pool alleles, about `shared` of the records' alleles among them; spans of a few hundred.
    ambiguous: the places (negative: from the end) of the record array that are ambiguous.  own_bg: the row is a sample row of a pool built with this bg_max_ppm -
    every allele of it is in the pool, with its own count or span inside the sums."""
    alleles = set()
    while len(alleles) < n_records:
        alleles.add(random_allele(rng, n_pos))
    alleles = sorted(alleles, key=keyof)
    items, per_pos = [], np.zeros(n_pos, dtype=np.int64)
    places = {i % max(n_records, 1) for i in ambiguous}
    for i, a in enumerate(alleles):
        k = int(rng.choice([1, 2, 3, 5, 9, 30]))
        amb = i in places
        items.append(((a[0], a[1], 0) if amb else a, k, amb))
        per_pos[a[0]] += k
    assert len({keyof(it[0], it[2]) for it in items}) == len(items)
    span = (per_pos + rng.integers(10, 300, n_pos)).astype(np.int32)
    in_pool = {a for a in alleles if own_bg is not None or rng.random() < shared}
    assert own_bg is None or (n_pool >= n_records and not places)
    while len(in_pool) > n_pool:
        in_pool.pop()
    while len(in_pool) < n_pool:
        in_pool.add(random_allele(rng, n_pos))
    S = rng.integers(2000, 6000, n_pos).astype(np.int32)
    own = {it[0]: it[1] for it in items} if own_bg is not None else {}
    entries = []
    for a in in_pool:
        K, X = int(rng.integers(0, 40)), int(rng.choice([0, 0, 150, 700]))
        if a in own and CR.qualifies(own[a], int(span[a[0]]), own_bg):
            K += own[a]
        elif a in own:
            X += int(span[a[0]])
        entries.append((a, K, X))
    records = records_of(items)
    assert [bool(v) for v in records["ambiguous"]] == [i in places for i in range(len(records))]    # (the places survive the key order: the seed is chosen so)
    return records, span, pool_of(entries), S


SIZES = [(r, 65) for r in (0, 1, 63, 64, 65, 257)] + [(65, q) for q in (0, 1, 63, 64, 1000)]


@pytest.mark.parametrize("n_records,n_pool", SIZES)
def test_numbers_of_records_and_pool_entries(acc, n_records, n_pool):
    rng = np.random.default_rng(701 + 7 * n_records + n_pool)
    budget = [0, 0]
    for n_pos, own in ((1 if n_records <= 64 and n_pool <= 64 else 40, False), (4099, n_pool >= n_records), (4099, False)):
        p = dict(P0, min_q=int(rng.choice([0, 30])))
        records, span, pool, S = generated(rng, n_records, n_pool, n_pos, own_bg=p["bg_max_ppm"] if own else None)
        assert len(records) == n_records and len(pool) == n_pool
        check(acc, records, span, pool, S, own, p, budget=budget)
    assert budget[1] * 1000 <= budget[0]


def test_keys_at_the_ends_of_the_pool_and_absent_around_them(acc):
    """A pool of three alleles at positions 2 and 5; records below the first, at the first, between, at the last and above the last; positions 0 and n_pos - 1."""
    pool = pool_of([((2, 2, 5), 4, 0), ((2, 3, 17), 0, 120), ((5, 1, 2), 9, 40)])
    recs = [((0, 1, 0), 10, False), ((2, 2, 5), 11, False), ((2, 2, 6), 12, False), ((3, 15, 4 ** 15 - 1), 13, False), ((5, 1, 2), 14, False), ((5, 1, 3), 15, False),
            ((7, 2, 0), 16, False)]
    span = np.full(8, 150, dtype=np.int32)
    S = np.arange(1000, 1800, 100, dtype=np.int32)
    got, cands = check(acc, records_of(recs), span, pool, S, False, dict(P0, min_q=0))
    assert [(int(r["pos"]), int(r["bg_alt"]), int(r["bg_depth"])) for r in got] == [(0, 0, 1000), (2, 4, 1200), (2, 0, 1200), (3, 0, 1300), (5, 9, 1460), (5, 0, 1500), (7, 0, 1700)]
    got, cands = check(acc, records_of(recs), span, pool, S, False, dict(P0, min_q=0, bg_max_ppm=0))      # (the row is not in the pool: its own rate is no matter)
    assert len(got) == 7


def test_pool_keys_equal_up_to_the_last_base_and_lengths_at_one_position(acc):
    pool = pool_of([((3, 1, 1), 1, 0), ((3, 2, 6), 2, 0), ((3, 15, 4 ** 15 - 2), 3, 10), ((3, 15, 4 ** 15 - 1), 4, 20), ((3, 3, I.pack(b"CAA")), 5, 30),
                    ((3, 3, I.pack(b"CAC")), 6, 40)])
    recs = [(a, 12, False) for a in ((3, 1, 1), (3, 2, 6), (3, 15, 4 ** 15 - 2), (3, 15, 4 ** 15 - 1), (3, 3, I.pack(b"CAA")), (3, 3, I.pack(b"CAC")), (3, 3, I.pack(b"CAG")),
                                     (3, 15, 0))]
    span, S = np.full(4, 120, dtype=np.int32), np.full(4, 900, dtype=np.int32)
    got, cands = check(acc, records_of(recs), span, pool, S, False, dict(P0, min_q=0))
    assert [(int(r["length"]), int(r["bases"]), int(r["bg_alt"]), int(r["bg_depth"])) for r in got] == [
        (1, 1, 1, 900), (2, 6, 2, 900), (3, I.pack(b"CAA"), 5, 870), (3, I.pack(b"CAC"), 6, 860), (3, I.pack(b"CAG"), 0, 900), (15, 0, 0, 900), (15, 4 ** 15 - 2, 3, 890),
        (15, 4 ** 15 - 1, 4, 880)]


@pytest.mark.parametrize("where", ["first", "last", "every second", "all"])
def test_ambiguous_records_are_skipped(acc, where):
    rng = np.random.default_rng(719)
    n = 130
    amb = {"first": (0,), "last": (-1,), "every second": range(1, n, 2), "all": range(n)}[where]
    records, span, pool, S = generated(rng, n, 40, 3000, ambiguous=amb)
    assert records["ambiguous"][0] == (where in ("first", "all")) and records["ambiguous"][-1] == (where in ("last", "all", "every second"))
    got, cands = check(acc, records, span, pool, S, False, dict(P0, min_q=0))
    assert (len(got) == 0) == (where == "all")


@pytest.mark.parametrize("n_cand", [0, 1, 15, 16, 17, 65])
def test_numbers_of_candidates(acc, n_cand):
    """257 records of which exactly n_cand are candidates (10 of 100 against a background of nothing); the others show one molecule, below min_alt."""
    rng = np.random.default_rng(727 + n_cand)
    chosen = set(rng.choice(257, n_cand, replace=False).tolist())
    recs = [((x, 1 + x % 3, x % 4), 10 if x in chosen else 1, False) for x in range(257)]
    span, S = np.full(257, 100, dtype=np.int32), np.full(257, 3000, dtype=np.int32)
    got, cands = check(acc, records_of(recs), span, np.zeros(0, dtype=capi.INSERTION_POOL_RECORD_DTYPE), S, False, P0)
    assert len(got) == len(cands) == n_cand and sorted(int(r["pos"]) for r in got) == sorted(chosen)
    if n_cand == 65:                                                                # all records candidates
        got, cands = check(acc, records_of([(a, 10, False) for a, _k, _amb in recs]), span, np.zeros(0, dtype=capi.INSERTION_POOL_RECORD_DTYPE), S, False, P0)
        assert len(got) == 257


def test_the_depth_cap_and_the_score_cap(acc):
    """n at the cap is tested, n one above is too deep; every molecule of 2^20 showing the allele under e = 1 / 1000 scores far above 9999."""
    recs = [((0, 1, 0), CAP, False), ((1, 1, 0), CAP, False), ((2, 2, 7), 40, False)]
    span = np.array([CAP, CAP + 1, 40], dtype=np.int32)
    S = np.zeros(3, dtype=np.int32)
    p = dict(P0, n0=1024)
    got, cands = check(acc, records_of(recs), span, np.zeros(0, dtype=capi.INSERTION_POOL_RECORD_DTYPE), S, False, p)
    assert [(int(r["pos"]), int(r["depth"]), int(r["q"])) for r in got] == [(0, CAP, 9999), (2, 40, 1204)]
    _got, totals = acc.insertion_call_tables(records_of(recs), span, np.zeros(0, dtype=capi.INSERTION_POOL_RECORD_DTYPE), S, False, capi.CallParams(**p))
    assert totals == {"tested": 2, "too_deep": 1, "candidates": 2, "calls": 2}


def test_the_three_kinds_of_own_row(acc):
    """The carrier cell of the CPU test through the sparse form: S = 300, X = 100 (the carrier's span), K = 10."""
    pool, S = pool_of([((0, 1, 0), 10, 100)]), np.array([300], dtype=np.int32)
    p = dict(P0, min_q=0)
    one = lambda k, n, own: [(int(r["depth"]), int(r["alt"]), int(r["bg_alt"]), int(r["bg_depth"])) for r in
                             check(acc, records_of([((0, 1, 0), k, False)]), np.array([n], dtype=np.int32), pool, S, own, p)[0]]
    assert one(5, 100, True) == [(100, 5, 5, 100)] and one(30, 100, True) == [(100, 30, 10, 200)] and one(8, 50, False) == [(50, 8, 10, 200)]


# ---- the score across depth: the sharp cells of the variant calls, planted as insertion alleles ------------------------------------------------------------------
DOC = json.load(open(FIXTURE))
CELLS = [dict(c, kind=kind) for kind in ("sharp", "loop_end", "near_one") for c in DOC[kind]]
PRIORS = sorted({(c["a0"], c["n0"]) for c in CELLS})


def test_every_sharp_cell_as_one_record(acc):
    """Per prior of the fixture one call: cell x is the allele (x, 1 + x % 3, x % 4) with k of n; the pool holds it with bg_alt = A - a0 and S, bg_excluded arranged so
    that N_o + n0 = B.  Every q is the floor of the fixture's high-precision score; no cell lies in the band."""
    seen = 0
    for prior in PRIORS:
        cells = [c for c in CELLS if (c["a0"], c["n0"]) == prior]
        hp = {(c["k"], c["n"], c["K_o"] + c["a0"], c["N_o"] + c["n0"]): decimal.Decimal(c["hp"]) for c in cells}
        recs, pool, span, S = [], [], [], []
        for x, c in enumerate(cells):
            a = (x, 1 + x % 3, x % 4)
            X = min(7 * (x % 3), 2 ** 31 - 1 - c["N_o"])
            recs.append((a, c["k"], False)); pool.append((a, c["K_o"], X)); span.append(c["n"]); S.append(c["N_o"] + X)
        p = CR.params(**dict(DOC["filters"], a0=prior[0], n0=prior[1]))
        got, cands = check(acc, records_of(recs), np.array(span, dtype=np.int32), pool_of(pool), np.array(S, dtype=np.int32), False, p, score=lambda k, n, A, B: hp[(k, n, A, B)])
        assert len(got) == len(cells) == len(cands) and not any(c["excluded"] for c in cands)
        for r, c in zip(got, cells):
            assert (int(r["depth"]), int(r["alt"]), int(r["bg_alt"]), int(r["bg_depth"])) == (c["n"], c["k"], c["K_o"], c["N_o"])
            assert int(r["q"]) == min(CR.Q_CAP, math.floor(decimal.Decimal(c["hp"]))), (c, r)
        seen += len(cells)
    assert seen == len(CELLS) >= 64 + 10 + 4


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_state():
    a = capi.Accel(capi.make_params(130, 140))
    try:
        lib, h = a.lib, a.h
        i32p = capi.C.POINTER(capi.C.c_int32)
        out = np.zeros(4, dtype=capi.INSERTION_CALL_RECORD_DTYPE)
        assert lib.mipgen_accel_insertion_call_fetch(h, out.ctypes.data, 0) == E_STATE and b"holds no insertion calls" in lib.mipgen_accel_last_error()
        assert lib.mipgen_accel_insertion_pool_fetch(h, None, 0, None) == E_STATE                              # no consensus reads
        assert lib.mipgen_accel_reads_consensus_insertion_call(h, 0, capi.C.byref(capi.CallParams()), None, None, None, None) == E_STATE
        good_r = records_of([((1, 1, 0), 10, False), ((2, 2, 3), 10, False)])
        good_p = pool_of([((1, 1, 0), 1, 0), ((3, 15, 9), 2, 0)])
        span, S = np.full(4, 100, dtype=np.int32), np.full(4, 1000, dtype=np.int32)
        tot = capi.CallTotals()

        def call(records=good_r, n_records=None, pool=good_p, n_pool=None, n_pos=4, span_=span, S_=S, prm=capi.CallParams(min_q=0)):
            return lib.mipgen_accel_insertion_call_tables(h, records.ctypes.data if records is not None else None, len(records) if n_records is None else n_records,
                                                          span_.ctypes.data_as(i32p) if span_ is not None else None, n_pos,
                                                          pool.ctypes.data if pool is not None else None, len(pool) if n_pool is None else n_pool,
                                                          S_.ctypes.data_as(i32p) if S_ is not None else None, 0, capi.C.byref(prm) if prm is not None else None, capi.C.byref(tot))

        def edited(arr, i, **kw):
            out = arr.copy()
            for k, v in kw.items():
                out[k][i] = v
            return out

        bad = [{"prm": None}, {"prm": capi.CallParams(min_depth=0)}, {"prm": capi.CallParams(min_alt=0)}, {"prm": capi.CallParams(min_ppm=1000001)},
               {"prm": capi.CallParams(min_q=10000)}, {"prm": capi.CallParams(a0=5, n0=5)}, {"prm": capi.CallParams(bg_max_ppm=-1)},
               {"n_pos": 0}, {"n_pos": 1 << 29}, {"n_records": -1}, {"n_records": 1 << 29}, {"n_pool": -1}, {"n_pool": 1 << 29},
               {"records": edited(good_r, 1, pos=4)}, {"records": edited(good_r, 0, pos=-1)}, {"pool": edited(good_p, 1, pos=4)}, {"pool": edited(good_p, 0, pos=-1)},
               {"records": good_r[::-1].copy()}, {"records": np.concatenate([good_r[:1], good_r[:1]])},
               {"pool": good_p[::-1].copy()}, {"pool": np.concatenate([good_p[:1], good_p[:1]])},
               {"pool": edited(good_p, 0, length=0)}, {"pool": edited(good_p, 1, length=16)},
               {"span_": None}, {"S_": None}, {"records": None, "n_records": 2}, {"pool": None, "n_pool": 2}]
        for kw in bad:
            assert call(**kw) == E_INVALID, kw
        assert lib.mipgen_accel_insertion_call_fetch(h, out.ctypes.data, 0) == E_STATE                           # nothing was run by any of them
        assert call() == 0 and tot.calls == 2 and tot.candidates == 2 and tot.tested == 2
        for n in (0, 1, 3, -1):
            assert lib.mipgen_accel_insertion_call_fetch(h, out.ctypes.data, n) == E_INVALID, n
        assert b"left 2" in lib.mipgen_accel_last_error() and lib.mipgen_accel_insertion_call_fetch(h, None, 2) == E_INVALID
        assert lib.mipgen_accel_insertion_call_fetch(h, out.ctypes.data, 2) == 0 and out["pos"][:2].tolist() == [1, 2] and out["bg_alt"][:2].tolist() == [1, 0]
        assert call(n_pos=0) == E_INVALID and lib.mipgen_accel_insertion_call_fetch(h, out.ctypes.data, 2) == 0    # a refused call leaves the records of the last one
        # the variant calls of the handle are another list: none was made, and this call left none
        assert lib.mipgen_accel_call_fetch(h, None, 0) == E_STATE
        # timing index 16
        a.set_timing(True)
        assert a.last_kernel_ms(16) < 0
        assert call() == 0 and a.last_kernel_ms(16) > 0 and a.last_kernel_ms(13) < 0 and a.last_kernel_ms(15) < 0
        assert call(records=good_r[:0], n_records=0) == 0 and tot.calls == 0 and lib.mipgen_accel_insertion_call_fetch(h, None, 0) == 0
        a.set_timing(False)
    finally:
        a.close()
