"""GPU: the score of the variant calls between depth 5,000 and the depth cap 2^20, where the exact integer sum of tests/call_ref.py cannot go.  The
reference is call_ref.hp_phred - a fixed-point integer sum over every term and `decimal` logarithms, good to 1e-70 - and the cells are those of
tests/golden/call_sharp_cells.json (tools/call_sharp_cells.py): per depth and background a candidate whose score lies 2e-6 to 2e-5 above an integer and one as far
below, so that an error of the device's log, exp or lnfact of more than 2e-6 in either direction flips a floor; the cells whose last round of 16 lanes runs
beyond n; and e = (B - 1) / B.  Everything goes through mipgen_accel_call_tables and test_gpu_call_tables.check: totals and every record, q included, exactly; the
exclusion band stays at 1e-6 and no cell of any table here may lie in it.  The fixture's strings are checked against hp_phred on the CPU (tests/test_call_cpu.py);
here they are read, and hp_phred itself is run once per distinct cell of the dense table."""
import decimal
import faulthandler
import json
import math
import os

import numpy as np
import pytest

from tests import call_ref as CR
from tests import test_gpu_call_tables as T

pytestmark = pytest.mark.gpu
CAP = CR.MAX_DEPTH
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_sharp_cells.json")


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test's device work runs under a time limit of its own: a stuck call ends the process with a traceback instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def acc():
    a = T.capi.Accel(T.capi.make_params(130, 140))
    yield a
    a.close()


DOC = json.load(open(FIXTURE))
CELLS = [dict(c, kind=kind) for kind in ("sharp", "loop_end", "near_one") for c in DOC[kind]]
PRIORS = sorted({(c["a0"], c["n0"]) for c in CELLS})
SHARP_PRIORS = sorted({(c["a0"], c["n0"]) for c in CELLS if c["kind"] == "sharp"})
_hp = {(c["k"], c["n"], c["K_o"] + c["a0"], c["N_o"] + c["n0"]): decimal.Decimal(c["hp"]) for c in CELLS}


def hp(k, n, A, B):
    """call_ref.hp_phred, once per distinct cell of the module; the fixture's cells come from the file."""
    if (k, n, A, B) not in _hp:
        _hp[(k, n, A, B)] = CR.hp_phred(k, n, A, B)
    return _hp[(k, n, A, B)]


def params_of(prior, **kw):
    return CR.params(**dict(DOC["filters"], a0=prior[0], n0=prior[1], **kw))


def table_of(cells, columns, own=False, bg_max_ppm=10 ** 6):
    """One position per cell (n, k, K_o, N_o): ref class x % 4, the alt class the next base, or del at every second position of the gapped shape.  own: the row is a
    sample row, so the pool holds K_o + k, N_o + n wherever the row qualifies - what leave-one-out then takes off again."""
    n_pos = len(cells)
    counts = np.zeros((n_pos, columns), dtype=np.int32)
    pool = np.zeros((n_pos, 10), dtype=np.int32)
    for x, (n, k, K_o, N_o) in enumerate(cells):
        r = x % 4
        a = 4 if columns == 8 and x % 2 else (r + 1) % 4
        T.set_cell(counts, columns, x, r, a, n, k)
        inside = own and CR.qualifies(k, n, bg_max_ppm)
        pool[x][a], pool[x][5 + a] = K_o + (k if inside else 0), N_o + (n if inside else 0)
    return counts, pool, (b"ACGT" * (n_pos // 4 + 1))[:n_pos]


def check(acc, key, counts, pool, ref, own, p):
    """test_gpu_call_tables.check with hp as the score: the oracle pass is made here under the key that check then finds in the module cache.  No cell may lie in
    the exclusion band."""
    totals, cands = T.oracle(("deep",) + key, counts, pool, ref, own, p, score=hp)
    assert totals["excluded"] == 0, (key, [c for c in cands if c["excluded"]])
    got, cands = T.check(acc, ("deep",) + key, counts, pool, ref, own, p, max_excluded_per_mille=0)
    assert len(got) == len(cands) == totals["candidates"]                  # (min_q is 0 in every table of this file: every candidate is a call)
    return got, cands


def cell_key(c):
    return (c["n"], c["k"], c["K_o"], c["N_o"])


@pytest.mark.parametrize("columns", [5, 8])
def test_every_fixture_cell_as_one_position_of_one_table(acc, columns):
    """A table per prior of the fixture (a table has one prior): every record, q included, and the totals, exactly."""
    seen = 0
    for prior in PRIORS:
        cells = [c for c in CELLS if (c["a0"], c["n0"]) == prior]
        counts, pool, ref = table_of([cell_key(c) for c in cells], columns)
        got, cands = check(acc, ("fixture", prior, columns), counts, pool, ref, False, params_of(prior))
        assert len(got) == len(cells)
        for r, c in zip(got, cells):                                       # (said once more without the oracle in between: the floor of the stored string)
            assert (int(r["depth"]), int(r["alt"]), int(r["bg_alt"]), int(r["bg_depth"])) == cell_key(c)
            assert int(r["q"]) == math.floor(decimal.Decimal(c["hp"])), (c, r)
        seen += len(cells)
    assert seen == len(CELLS) >= 64 + 10 + 4


@pytest.mark.parametrize("columns", [5, 8])
def test_the_row_inside_its_own_pool_at_depth(acc, columns):
    """own_row_is_sample = 1 and pool sums that include the row: the leave-one-out subtraction in front of a deep tail.  With bg_max_ppm = 200,000 the cells
    under e <= 1e-2 qualify and leave their pool; the cells whose alt fraction is above 20 % were never in it."""
    for prior in SHARP_PRIORS:
        cells = [c for c in CELLS if (c["a0"], c["n0"]) == prior and c["n"] >= 1 << 14]
        assert any(CR.qualifies(c["k"], c["n"], 200000) for c in cells) and not all(CR.qualifies(c["k"], c["n"], 200000) for c in cells)
        counts, pool, ref = table_of([cell_key(c) for c in cells], columns, own=True, bg_max_ppm=200000)
        got, _ = check(acc, ("own", prior, columns), counts, pool, ref, True, params_of(prior, bg_max_ppm=200000))
        assert [(int(r["depth"]), int(r["alt"]), int(r["bg_alt"]), int(r["bg_depth"]), int(r["q"])) for r in got] == \
               [cell_key(c) + (math.floor(decimal.Decimal(c["hp"])),) for c in cells]


@pytest.mark.parametrize("n_cand", [61, 64, 67])
def test_q_does_not_depend_on_the_neighbours_in_the_wavefront(acc, n_cand):
    """A quarter wavefront per candidate, and the wavefront leaves the loop together: the deep near-mean cells of the fixture (n >= 2^18, e >= 0.3: hundreds of rounds)
    beside one-round cells (n = 60, k = 3 under the bare prior), laid out deep first, deep last, and one to one.  61, 64 and 67 candidates: the last wavefront of
    the tail kernel holds 1, 4 and 3 candidates, so idle quarter wavefronts sit beside a deep one.  q by (n, k, K_o, N_o) is the fixture's in every layout."""
    prior = max(SHARP_PRIORS, key=lambda pr: sum((c["a0"], c["n0"]) == pr and c["kind"] == "sharp" and c["n"] >= 1 << 18 and c["e"] >= 0.3 for c in CELLS))
    deep = [cell_key(c) for c in CELLS if (c["a0"], c["n0"]) == prior and c["kind"] == "sharp" and c["n"] >= 1 << 18 and c["e"] >= 0.3]
    assert len(deep) >= 5
    n_deep = 30
    deep = [deep[i % len(deep)] for i in range(n_deep)]
    ones = [(60, 3, 0, 0)] * (n_cand - n_deep)
    one_to_one = [c for pair in zip(deep, ones) for c in pair] + ones[n_deep:]
    want = {c: math.floor(hp(c[1], c[0], c[2] + prior[0], c[3] + prior[1])) for c in set(deep + ones)}
    assert want[(60, 3, 0, 0)] > 30
    seen = {c: set() for c in want}
    for name, cells in (("first", deep + ones), ("last", ones + deep), ("one_to_one", one_to_one)):
        assert len(cells) == n_cand
        for columns in (5, 8):
            counts, pool, ref = table_of(cells, columns)
            got, _ = check(acc, ("neighbours", n_cand, name, columns), counts, pool, ref, False, params_of(prior))
            assert len(got) == n_cand
            for r in got:
                seen[(int(r["depth"]), int(r["alt"]), int(r["bg_alt"]), int(r["bg_depth"]))].add(int(r["q"]))
    assert seen == {c: {q} for c, q in want.items()}


DENSE_SEED = 41457
DENSE_PRIOR = (3, 2999)


def dense_cells():
    """257 cells at n = 2^18 and 2^20 (the last of each at the depth itself): k at mean + z sigma, z uniform in [0, 8]; backgrounds from 1e-3 to 0.9."""
    rng = np.random.default_rng(DENSE_SEED)
    cells = []
    for x in range(257):
        n = (1 << 18, CAP)[x % 2]
        e = float(rng.choice([1e-3, 1e-2, 0.1, 0.3, 0.5, 0.9])) * float(rng.uniform(0.9, 1.1))
        N_o = int(rng.integers(10_000, 3_000_000))
        B = N_o + DENSE_PRIOR[1]
        A = max(DENSE_PRIOR[0], min(B - 1, int(B * e)))
        mean, sigma = n * A / B, math.sqrt(n * A / B * (1 - A / B))
        k = min(n, int(mean + float(rng.uniform(0, 8)) * sigma) + 1)
        cells.append((n, k, A - DENSE_PRIOR[0], N_o))
    return cells


@pytest.mark.parametrize("columns", [5, 8])
def test_a_dense_deep_table(acc, columns):
    """257 positions, every one a candidate at n = 2^18 or 2^20, scored by hp_phred (once for both shapes).  The usual rule - cells within 1e-6 of an integer are
    dropped from both sides, at most 1 in 1,000 candidates - allows none among 257; the seed was checked on the CPU to hold none."""
    cells = dense_cells()
    counts, pool, ref = table_of(cells, columns)
    got, cands = check(acc, ("dense", columns), counts, pool, ref, False, params_of(DENSE_PRIOR))
    assert len(cands) == 257 and {c["depth"] for c in cands} == {1 << 18, CAP}
    qs = [c["q"] for c in cands]
    assert min(qs) < 5 and max(qs) > 100 and max(qs) < CR.Q_CAP            # from just above the mean to 8 sigma, all below the cap
