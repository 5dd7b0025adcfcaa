"""GPU: the plan on the device and the fold of a count table into loci, reached directly through mipgen_accel_locus_tables.  Synthetic tables and
plans against tests/locus_ref.merge by exact equality of whole arrays and totals; every call is made twice and the bytes compared.  The merged output goes on to
mipgen_accel_call_tables against tests/call_ref.py on the oracle's merge."""
import faulthandler

import numpy as np
import pytest

from mipgen_amd import capi
from tests import call_ref as CALL
from tests import locus_ref as LR
from tests.test_gpu_reads import _accel

pytestmark = pytest.mark.gpu
E_INVALID = -1
LIMIT = (1 << 29) - 1                         # MIPGEN_CALL_MAX_POSITIONS


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test's device work runs under a time limit of its own: a stuck call ends the process with a traceback instead of holding the GPU."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def acc():
    a = _accel()
    yield a
    a.close()


def random_plan(rng, n_loci, strands, excluded=0.2, long_locus=True):
    """A plan whose loci have 0, 1, 2, 3 or 8 sources - and one of them 300, a lane in a long loop beside lanes with one source - scattered over the template
    positions in random order among excluded ones.  strands: "plus", "minus" or "mixed"; bit 1 is drawn on either strand wherever x >= 1."""
    per_locus = rng.choice([0, 1, 2, 3, 8], size=n_loci, p=[0.15, 0.4, 0.2, 0.15, 0.1])
    if long_locus:
        per_locus[rng.integers(0, n_loci)] = 300
    owners = np.repeat(np.arange(n_loci, dtype=np.int64), per_locus)
    n_out = int(len(owners) * excluded) + 1
    entries = np.concatenate([owners, np.full(n_out, -1, dtype=np.int64)])
    rng.shuffle(entries)
    plan = []
    for x, l in enumerate(entries):
        if l < 0:
            plan.append(-1)
            continue
        minus = {"plus": 0, "minus": 1, "mixed": int(rng.integers(0, 2))}[strands]
        plan.append(int(l) * 4 + minus + (2 if x >= 1 and rng.random() < 0.5 else 0))
    return plan


def random_counts(rng, n_pos, columns, top=1 << 20):
    """Counters up to `top`: mostly small, a tenth of the rows near the top."""
    counts = rng.integers(0, 50, (n_pos, columns)).astype(np.int64)
    big = rng.random(n_pos) < 0.1
    counts[big] = rng.integers(top - 3, top + 1, (int(big.sum()), columns))
    counts[rng.random(n_pos) < 0.1] = 0
    return counts.astype(np.int32)


def check(acc, counts, plan, n_loci):
    """locus_tables twice: the same bytes, and the oracle's merged table and totals."""
    want = LR.merge(counts, plan, n_loci)
    merged, totals = acc.locus_tables(counts, plan, n_loci)
    merged2, totals2 = acc.locus_tables(counts, plan, n_loci)
    assert merged.tobytes() == merged2.tobytes() and totals == totals2
    assert merged.dtype == np.int32 and merged.shape == want.shape
    assert np.array_equal(merged, want), np.flatnonzero((merged != want).any(axis=1))[:5]
    assert totals == LR.totals(want)
    return merged


@pytest.mark.parametrize("strands", ["plus", "minus", "mixed"])
@pytest.mark.parametrize("columns", [5, 8])
@pytest.mark.parametrize("n_loci", [1, 63, 64, 65, 257, 4099])
def test_merge_equals_the_oracle(acc, n_loci, columns, strands):
    rng = np.random.default_rng(9000 + 10 * n_loci + columns + {"plus": 0, "minus": 100000, "mixed": 200000}[strands])
    plan = random_plan(rng, n_loci, strands)
    sources = np.bincount([e >> 2 for e in plan if e >= 0], minlength=n_loci)
    assert sources.max() == 300 and (n_loci < 63 or {0, 1, 2, 3, 8} <= set(sources.tolist()))
    check(acc, random_counts(rng, len(plan), columns), plan, n_loci)


@pytest.mark.parametrize("columns", [5, 8])
def test_every_position_excluded_and_none_excluded(acc, columns):
    rng = np.random.default_rng(9101 + columns)
    counts = random_counts(rng, 130, columns)
    merged = check(acc, counts, [-1] * 130, 65)
    assert not merged.any()
    check(acc, counts, [-1] * 130, 1)
    plan = [int(l) * 4 + int(f) for l, f in zip(rng.integers(0, 65, 130), rng.integers(0, 2, 130))]      # none excluded
    merged = check(acc, counts, plan, 65)
    assert int(merged[:, :5].astype(np.int64).sum()) == int(counts[:, :5].astype(np.int64).sum())           # A..T swap among themselves, discordant stays
    check(acc, counts, list(range(0, 4 * 130, 4)), 130)                                                     # the identity: one plus source per locus
    assert np.array_equal(acc.locus_tables(counts, list(range(0, 4 * 130, 4)), 130)[0], counts)


def test_bit_1_on_the_first_position_of_a_probes_successor(acc):
    """Two probes of 70 and 66 positions.  Bit 1 on x = 70, the first position of the second probe, takes the insertion columns of x - 1 = 69, the last row of
    the FIRST probe: the plan is obeyed as given, the device knows no probe."""
    rng = np.random.default_rng(9111)
    counts = random_counts(rng, 136, 8, top=1000)
    plan = [-1] * 136
    plan[70] = 0 * 4 + 1 + 2
    plan[71] = 1 * 4 + 1 + 2
    plan[69] = 1 * 4 + 0
    merged = check(acc, counts, plan, 2)
    assert merged[0].tolist() == [counts[70][3], counts[70][2], counts[70][1], counts[70][0], counts[70][4], counts[70][5], counts[69][6], counts[69][7]]
    assert merged[1][6] == counts[70][6] + counts[69][6] and merged[1][7] == counts[70][7] + counts[69][7]
    # a minus source without bit 1 adds no insertion; a plus source with bit 1 takes row x - 1's instead of its own
    merged = check(acc, counts, [-1] * 70 + [1] + [-1] * 65, 1)
    assert merged[0][6] == 0 == merged[0][7] and merged[0][5] == counts[70][5]
    merged = check(acc, counts, [-1] * 70 + [2] + [-1] * 65, 1)
    assert merged[0].tolist() == counts[70][:6].tolist() + counts[69][6:].tolist()
    # five columns: bit 1 has nothing to move
    five = np.ascontiguousarray(counts[:, :5])
    assert np.array_equal(check(acc, five, plan, 2)[0], [five[70][3], five[70][2], five[70][1], five[70][0], five[70][4]])


@pytest.mark.parametrize("columns", [5, 8])
def test_a_plan_in_reversed_locus_order(acc, columns):
    """Position x belongs to locus n - 1 - x // 2: the sort has to turn the whole order round, and the two sources of a locus stay in ascending x."""
    rng = np.random.default_rng(9121 + columns)
    n_loci = 1000
    counts = random_counts(rng, 2 * n_loci, columns)
    plan = [(n_loci - 1 - x // 2) * 4 + (x & 1) + (2 if x & 1 else 0) for x in range(2 * n_loci)]
    check(acc, counts, plan, n_loci)


@pytest.mark.parametrize("columns", [5, 8])
def test_counters_of_2_to_the_20_in_300_sources(acc, columns):
    counts = np.full((600, columns), 1 << 20, dtype=np.int32)
    plan = [(x % 2) * 4 + (x // 2) % 2 for x in range(600)]                                                  # 300 sources for each of two loci
    merged = check(acc, counts, plan, 2)
    assert int(merged[0][0]) == 300 << 20 == int(merged[1][4])
    if columns == 8:
        assert merged[0][5] == 300 << 20 and merged[0][6] == 150 << 20                                      # the minus sources carry no bit 1: their insertions are 0


def planted_tables(rng, n_pos, columns, plan, n_rows=3):
    """Tables of n_rows samples at depths a call can be made at: about 30 molecules per position on the ref base, alts in some cells, deletions with 8 columns."""
    ref_of_locus = rng.integers(0, 4, max(e >> 2 for e in plan if e >= 0) + 1)
    tables = []
    for r in range(n_rows):
        t = np.zeros((n_pos, columns), dtype=np.int32)
        for x, e in enumerate(plan):
            if e < 0:
                t[x] = rng.integers(0, 40, columns)                                                           # what an excluded position holds must not matter
                continue
            b = int(ref_of_locus[e >> 2])
            col = 3 - b if e & 1 else b                                                                       # a minus source shows the complement
            t[x][col] = rng.integers(20, 40)
            if rng.random() < 0.25:
                t[x][rng.integers(0, 4)] += rng.integers(1, 9)
            if columns == 8 and rng.random() < 0.1:
                t[x][5] = rng.integers(1, 9)
            t[x][4] = rng.integers(0, 3)
        tables.append(t)
    return tables, bytes(b"ACGT"[b] for b in ref_of_locus)


@pytest.mark.parametrize("columns,seed", [(5, 9201), (8, 9202)])
def test_the_merged_table_goes_on_to_call_tables(acc, columns, seed):
    rng = np.random.default_rng(seed)
    n_loci = 257
    plan = random_plan(rng, n_loci, "mixed", long_locus=False)
    tables, ref = planted_tables(rng, len(plan), columns, plan)
    ref = ref.ljust(n_loci, b"N")
    want = [LR.merge(t, plan, n_loci) for t in tables]
    got = [acc.locus_tables(t, plan, n_loci)[0] for t in tables]
    p = CALL.params(min_depth=20, min_alt=3, min_q=20, a0=3, n0=1007)
    pool = CALL.pool(want, p["bg_max_ppm"])
    n_calls = 0
    for row in range(3):
        assert np.array_equal(got[row], want[row])
        totals, cands = CALL.call_cells(want[row], pool, ref, True, p)
        assert totals["excluded"] * 1000 <= max(totals["candidates"], 1), totals
        records, got_totals = acc.call_tables(got[row], pool, ref, True, capi.CallParams(**p))
        assert {k: got_totals[k] for k in ("tested", "too_deep", "candidates")} == {k: totals[k] for k in ("tested", "too_deep", "candidates")}
        assert CALL.drop_excluded(records, cands) == CALL.kept_calls(cands, p)
        n_calls += len(records)
    assert n_calls >= 10


def test_timing_index_14_and_no_other(acc):
    counts = np.ones((64, 5), dtype=np.int32)
    plan = list(range(0, 256, 4))
    before = [acc.last_kernel_ms(k) for k in (11, 12, 13)]
    acc.set_timing(True)
    try:
        acc.locus_tables(counts, plan, 64)
        assert acc.last_kernel_ms(14) > 0
    finally:
        acc.set_timing(False)
    acc.locus_tables(counts, plan, 64)
    assert acc.last_kernel_ms(14) < 0 and [acc.last_kernel_ms(k) for k in (11, 12, 13)] == before


def test_every_invalid_refusal(acc):
    lib, h, C = acc.lib, acc.h, capi.C
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    counts = np.ones((4, 8), dtype=np.int32)
    merged = np.full((3, 8), -7, dtype=np.int32)
    tot = capi.LocusTotals()

    def call(plan=(0, 5, -1, 8), columns=8, n_pos=4, n_loci=3, counts_=counts, null_plan=False):
        arr = np.array(plan, dtype=np.int64)
        return lib.mipgen_accel_locus_tables(h, counts_.ctypes.data_as(i32p) if counts_ is not None else None, columns, None if null_plan else arr.ctypes.data_as(i64p), n_pos,
                                             n_loci, merged.ctypes.data_as(i32p), C.byref(tot))

    for kw, needle in ((dict(null_plan=True), b"no locus plan"), (dict(counts_=None), b"no counts"), (dict(n_loci=0), b"0 loci"), (dict(n_loci=LIMIT + 1), b"loci"),
                       (dict(n_pos=0), b"0 positions"), (dict(n_pos=LIMIT + 1), b"positions"), (dict(plan=(0, 5, -2, 8)), b"entry -2"), (dict(plan=(0, 12, -1, 8)), b"locus 3"),
                       (dict(plan=(0, 5, -1, 8), n_loci=2), b"locus 2"), (dict(plan=(2, 5, -1, 8)), b"bit 1"), (dict(plan=(3, 5, -1, 8)), b"bit 1"), (dict(columns=6), b"6 columns"),
                       (dict(columns=0), b"0 columns")):
        assert call(**kw) == E_INVALID, kw
        assert needle in lib.mipgen_accel_last_error(), (kw, lib.mipgen_accel_last_error())
        assert (merged == -7).all()
    assert call() == 0 and merged.tolist() == [[1] * 8, [1, 1, 1, 1, 1, 1, 0, 0], [1] * 8] and tot.covered == 3
    assert call(plan=(1, 7, -1, 8)) == 0 and merged[1].tolist() == [1] * 8                                  # bit 1 at x = 1 is in order
    assert lib.mipgen_accel_locus_tables(h, counts.ctypes.data_as(i32p), 8, np.array([0, 5, -1, 8], dtype=np.int64).ctypes.data_as(i64p), 4, 3, None, None) == 0
