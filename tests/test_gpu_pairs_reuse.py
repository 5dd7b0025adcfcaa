"""GPU: one handle's sorted-pairs buffers reused from call to call (SortedPairs), through the three entry points that need no read
session: mipgen_accel_call_tables, mipgen_accel_insertion_call_tables and mipgen_accel_locus_tables.  Each is called five times in a row on ONE handle with 1, 65,
1, 200 and 65 pairs in the sorted set - the first reserve (DevBuf::reserve takes n + n / 8 + 64: a capacity of 65), a set that fills that capacity exactly (a
wavefront and one lane of the gather), a smaller set in larger buffers with a larger scratch, a set beyond the capacity (release and regrow), and a reuse of the
regrown buffers.  The pairs of the two calls are their candidates, planted so that every position or record is one; those of the fold are its positions.  Every
call's records or merged table and its totals equal the oracle's (tests/call_ref.py, tests/insertion_call_ref.py, tests/locus_ref.py) exactly - no planted cell lies
in the oracle's exclusion band, which the test asserts - and equal, byte for byte, the same call on a fresh handle."""
import faulthandler

import numpy as np
import pytest

from mipgen_amd import capi
from tests import call_ref as CR
from tests import insertion_call_ref as IC
from tests import locus_ref as LR
from tests.test_gpu_call_tables import set_cell
from tests.test_gpu_insertion_call_tables import records_of

pytestmark = pytest.mark.gpu
SIZES = (1, 65, 1, 200, 65)
P_CALL = CR.params(min_depth=20, min_alt=3, min_q=45)                      # (3 of 60 under the prior alone scores 37: k = 3..6 straddles min_q)
P_INS = CR.params(min_depth=20, min_alt=3, min_ppm=0, min_q=60, a0=1, n0=1000, bg_max_ppm=200000)
NO_POOL = np.zeros(0, dtype=capi.INSERTION_POOL_RECORD_DTYPE)


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test's device work runs under a time limit of its own: a stuck call ends the process with a traceback instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _accel():
    return capi.Accel(capi.make_params(130, 140))


@pytest.fixture(scope="module")
def acc():
    a = _accel()
    yield a
    a.close()


def call_case(n):
    """n positions, each with exactly one candidate, the first a call: k = 6..3 of 60..99 on one alt class (every fifth position: the deletion) over an empty pool."""
    counts = np.zeros((n, 8), dtype=np.int32)
    for x in range(n):
        set_cell(counts, 8, x, x % 4, 4 if x % 5 == 2 else (x + 1) % 4, 60 + x % 40, 6 - x % 4)
    pool, ref = np.zeros((n, 10), dtype=np.int32), (b"ACGT" * (n // 4 + 1))[:n]
    totals, cands = CR.call_cells(counts, pool, ref, False, P_CALL)
    assert totals["candidates"] == n == totals["tested"] and totals["excluded"] == 0
    assert 0 < totals["calls"] and (n < 65 or totals["calls"] < n)
    want = (CR.kept_calls(cands, P_CALL), {k: totals[k] for k in ("tested", "too_deep", "candidates", "calls")})

    def run(a):
        got, got_totals = a.call_tables(counts, pool, ref, False, capi.CallParams(**P_CALL))
        assert a.call_fetch(len(got)).tobytes() == got.tobytes()
        return [tuple(int(v) for v in r) for r in got], got_totals, got.tobytes()
    return run, want


def insertion_case(n):
    """n allele records at n anchors, each a candidate and the first a call: 11..4 molecules of a span of 100..139 against an empty pool (k = 4 scores 48 to 54, below min_q)."""
    recs = [((x, 1 + x % 3, x % 4), 11 - x % 8, False) for x in range(n)]
    records, span, S = records_of(recs), (100 + np.arange(n) % 40).astype(np.int32), np.zeros(n, dtype=np.int32)
    totals, cands = IC.call_cells(IC.Row(span, records), IC.pool_lookup(NO_POOL, S), False, P_INS)
    assert totals["candidates"] == n == totals["tested"] and totals["excluded"] == 0
    assert 0 < totals["calls"] and (n < 65 or totals["calls"] < n)
    want = (IC.kept_calls(cands, P_INS), {k: totals[k] for k in ("tested", "too_deep", "candidates", "calls")})

    def run(a):
        got, got_totals = a.insertion_call_tables(records, span, NO_POOL, S, False, capi.CallParams(**P_INS))
        assert a.insertion_call_fetch(len(got)).tobytes() == got.tobytes()
        return IC.drop_excluded(got, cands), got_totals, got.tobytes()          # (nothing is excluded: the records as the oracle's tuples)
    return run, want


def locus_case(n):
    """n positions over (n + 1) // 2 loci in reversed order - the sort turns the whole order round -, both strands, bit 1 on a third, a seventh excluded."""
    n_loci = (n + 1) // 2
    plan = [-1 if x % 7 == 3 else (n_loci - 1 - x // 2) * 4 + (x & 1) + (2 if x >= 1 and x % 3 == 0 else 0) for x in range(n)]
    counts = np.random.default_rng(9300 + n).integers(0, 1 << 20, (n, 8)).astype(np.int32)
    merged = LR.merge(counts, plan, n_loci)
    want = (merged.tolist(), LR.totals(merged))

    def run(a):
        got, got_totals = a.locus_tables(counts, plan, n_loci)
        assert got.dtype == np.int32 and got.shape == merged.shape
        return got.tolist(), got_totals, got.tobytes()
    return run, want


@pytest.mark.parametrize("case", [call_case, insertion_case, locus_case])
def test_five_calls_in_a_row_on_one_handle(acc, case):
    cases = {n: case(n) for n in set(SIZES)}                               # one oracle pass per size
    for step, n in enumerate(SIZES):
        run, (want, want_totals) = cases[n]
        got, got_totals, got_bytes = run(acc)
        assert got == want and got_totals == want_totals, (case.__name__, step, n)
        fresh = _accel()
        try:
            assert run(fresh)[2] == got_bytes, (case.__name__, step, n)
        finally:
            fresh.close()
