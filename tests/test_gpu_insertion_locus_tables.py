"""GPU: insertion alleles folded to genome loci from host arrays (mipgen_accel_locus_insertion_tables, mipgen_accel_locus_insertions_fetch).  Synthetic
allele records, anchor tables and plans; every comparison is exact equality of the locus records, the locus anchor table and the totals with
tests/insertion_locus_ref.py, every call is made twice and returns the same bytes, and the five invariants of 4.19 are asserted on every call, `merged` being what
mipgen_accel_locus_tables gives for an 8-column table with the same insertion columns under the same plan."""
import faulthandler

import numpy as np
import pytest

from mipgen_amd import capi
from tests import call_ref as CR
from tests import insertion_call_ref as IC
from tests import insertion_locus_ref as IL
from tests import insertion_ref as I

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE = -1, -6
NONE = np.zeros(0, dtype=capi.INSERTION_RECORD_DTYPE)


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


def records_of(items):
    """INSERTION_RECORD_DTYPE in ascending key order from ((pos, length, bases), count, ambiguous) items."""
    items = sorted(items, key=lambda it: I.key(it[0][0], it[0][1], it[2], it[0][2]))
    out = np.zeros(len(items), dtype=capi.INSERTION_RECORD_DTYPE)
    for i, (a, k, amb) in enumerate(items):
        out[i] = (a[0], a[1], k, 0 if amb else a[2], int(amb))
    return out


def anchors_of(records, n_pos, rng=None):
    """An anchor table the records are consistent with: ins and ambiguous are their sums per position, span at least ins, ins_discordant anything."""
    a = np.zeros((n_pos, 4), dtype=np.int32)
    for r in records:
        a[int(r["pos"])][1] += int(r["count"])
        a[int(r["pos"])][3] += int(r["count"]) if r["ambiguous"] else 0
    extra = rng.integers(0, 50, n_pos) if rng is not None else np.arange(n_pos) % 7
    a[:, 0] = a[:, 1] + extra
    a[:, 2] = (np.arange(n_pos) * 5) % 3
    return a


def check(acc, records, anchors, plan, n_loci):
    """One tables call, twice, against the oracle, with the invariants; (locus records, locus_anchors, totals)."""
    plan = np.asarray(plan, dtype=np.int64)
    got, la, totals = acc.locus_insertion_tables(records, anchors, plan, n_loci)
    again, la2, totals2 = acc.locus_insertion_tables(records, anchors, plan, n_loci)
    assert got.tobytes() == again.tobytes() and la.tobytes() == la2.tobytes() and totals == totals2 and got.dtype == capi.INSERTION_RECORD_DTYPE
    assert acc.locus_insertions_fetch(len(got)).tobytes() == got.tobytes()
    want, w_la, w_totals = IL.fold(records, anchors, plan, n_loci)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert np.array_equal(la, w_la) and totals == w_totals, (totals, w_totals)
    table = np.zeros((len(plan), 8), dtype=np.int32)
    table[:, 6], table[:, 7] = anchors[:, 1], anchors[:, 2]
    merged, _t = acc.locus_tables(table, plan, n_loci)
    IL.check_invariants(got, la, merged, records, plan)
    keys = [I.key(int(r["pos"]), int(r["length"]), bool(r["ambiguous"]), int(r["bases"])) for r in got]
    assert keys == sorted(set(keys))
    return got, la, totals


def random_records(rng, n_records, n_pos, ambiguous_every=0):
    seen, items = set(), []
    while len(items) < n_records:
        l = int(rng.choice([1, 1, 2, 3, 6, 15]))
        amb = bool(ambiguous_every) and len(items) % ambiguous_every == 0
        a = (int(rng.integers(0, n_pos)), l, 0 if amb else int(rng.integers(0, 4 ** l)))
        k = I.key(a[0], a[1], amb, a[2])
        if k not in seen:
            seen.add(k)
            items.append((a, int(rng.choice([1, 2, 3, 9])), amb))
    return records_of(items)


def pair_plan(m):
    """A plus probe over positions [0, m) and a minus probe over [m, 2 m) on the same m loci, as locus_plan builds them: the minus probe's position m + t is locus
    m - 1 - t with bit 0 and, from t = 1 on, bit 1."""
    return [l * 4 for l in range(m)] + [(m - 1 - t) * 4 + 1 + (2 if t >= 1 else 0) for t in range(m)]


@pytest.mark.parametrize("n_records", [0, 1, 63, 64, 65, 300])
def test_numbers_of_records(acc, n_records):
    """The wavefront edges of the slot reservation, under a plus / minus pair of probes and under a plan with excluded positions."""
    rng = np.random.default_rng(907 + n_records)
    m = 90
    records = random_records(rng, n_records, 2 * m, ambiguous_every=7)
    anchors = anchors_of(records, 2 * m, rng)
    _got, _la, totals = check(acc, records, anchors, pair_plan(m), m)
    assert totals["folded"] + totals["dropped"] == n_records                            # (an anchor row of such a pair has one source at most)
    plan = np.array(pair_plan(m), dtype=np.int64)
    plan[rng.random(2 * m) < 0.3] = -1
    check(acc, records, anchors, plan, m)


def test_64_records_all_pulled_twice(acc):
    """Position 2 i is a flags-0 source and position 2 i + 1 a plus source with bit 1: anchor row 2 i is pulled by both, into two loci - 128 pairs of 64 records."""
    plan = []
    for i in range(64):
        plan += [(2 * i) * 4, (2 * i + 1) * 4 + 2]
    records = records_of([((2 * i, 1 + i % 3, i % 4), 1 + i % 5, False) for i in range(64)])
    got, la, totals = check(acc, records, anchors_of(records, 128), plan, 128)
    assert totals["folded"] == 128 and totals["dropped"] == 0 and len(got) == 128 and sum(int(r["count"]) for r in got) == 2 * int(records["count"].sum())
    # the same with both sources in ONE locus: the two pairs of a record meet in one key
    both = [v + (2 if x % 2 else 0) for x, v in enumerate(sum(([l * 4, l * 4] for l in range(64)), []))]
    got, la, totals = check(acc, records, anchors_of(records, 128), both, 64)
    assert totals["folded"] == 128 and len(got) == 64 and [int(r["count"]) for r in got] == [2 * int(r["count"]) for r in records]


def test_nothing_is_pulled(acc):
    records = random_records(np.random.default_rng(911), 70, 40)
    anchors = anchors_of(records, 40)
    for plan in ([-1] * 40, [l * 4 + 1 for l in range(40)]):                            # no source at all; minus sources without bit 1
        got, la, totals = check(acc, records, anchors, plan, 40)
        assert len(got) == 0 and not la.any() and totals == dict.fromkeys(IL.TOTAL_KEYS, 0) | {"dropped": 70}


def test_the_ends_a_probe_boundary_minus_one_entries_and_the_sources_of_a_locus(acc):
    """Two plus probes of 5 positions and a minus probe of 5.  Anchor 0 and anchor n_pos - 1 (a flags-0 source at the last position); bit 1 on the first position
    of the second probe pulls the last row of the first; -1 entries; locus 2 has three sources, locus 6 none."""
    #        probe A (plus)            probe B (plus, bit 1 at its first position)   probe C (minus)
    plan = [0 * 4, 1 * 4, 2 * 4, -1, 3 * 4,   4 * 4 + 2, 2 * 4, -1, 5 * 4, 7 * 4,   8 * 4 + 1, 2 * 4 + 3, 1 * 4 + 3, -1, 9 * 4]
    items = [((0, 1, 2), 3, False), ((4, 2, 7), 2, False), ((4, 1, 0), 1, True), ((6, 3, 11), 4, False), ((2, 3, 11), 5, False), ((10, 3, I.pack(b"GAT")), 6, False),
             ((11, 2, 1), 7, False), ((14, 15, 4 ** 15 - 1), 8, False), ((3, 1, 1), 9, False), ((12, 1, 0), 2, False)]
    records = records_of(items)
    got, la, totals = check(acc, records, anchors_of(records, 15), plan, 10)
    by = {(int(r["pos"]), int(r["length"]), int(r["bases"]), int(r["ambiguous"])): int(r["count"]) for r in got}
    assert by[(0, 1, 2, 0)] == 3 and by[(9, 15, 4 ** 15 - 1, 0)] == 8                    # anchors 0 and n_pos - 1
    assert by[(3, 2, 7, 0)] == 2 and by[(4, 2, 7, 0)] == 2 and by[(3, 1, 0, 1)] == 1 and by[(4, 1, 0, 1)] == 1      # row 4 is A's own and, across the boundary, B's
    assert by[(2, 3, 11, 0)] == 9                                                        # rows 2 and 6 of locus 2 meet in one key
    assert by[(2, 3, I.pack(b"ATC"), 0)] == 6                                            # row 10 under position 11's bit 1, turned
    assert by[(1, 2, I.pack(b"GT"), 0)] == 7                                             # row 11 (AC) under position 12's bit 1, turned
    assert not la[6].any() and totals["dropped"] == 2 and totals["folded"] == 10         # rows 3 and 12 have no source (12: position 13 is -1)


def test_plus_and_minus_alleles_meet_in_one_key_and_differ_in_the_last_base(acc):
    m = 20
    plan = pair_plan(m)
    minus_row = lambda l: m + (m - 1 - l) - 1                                            # the anchor row the minus probe's source of locus l pulls (bit 1: x - 1)
    rc = lambda s: I.pack(bytes({65: 84, 67: 71, 71: 67, 84: 65}[b] for b in reversed(s)))
    items = [((5, 3, I.pack(b"GAT")), 4, False), ((minus_row(5), 3, rc(b"GAT")), 3, False),                         # +GAT on both strands: one record, 7
             ((7, 2, I.pack(b"AT")), 2, False), ((minus_row(7), 2, I.pack(b"AT")), 5, False),                       # a palindrome
             ((9, 3, I.pack(b"CAA")), 1, False), ((9, 3, I.pack(b"CAC")), 2, False),                                 # equal up to the last base on the plus strand
             ((minus_row(9), 3, rc(b"CAC")), 3, False), ((minus_row(9), 3, rc(b"CAG")), 4, False),                   # ... on the minus strand: they differ in the FIRST base there
             ((minus_row(11), 15, rc(b"ACGTACGTACGTACG")), 6, False), ((11, 15, I.pack(b"ACGTACGTACGTACG")), 1, False),
             ((minus_row(13), 4, 0), 2, True), ((minus_row(13), 18, 0), 3, True), ((13, 18, 0), 4, True)]           # ambiguous and a long run from the minus source
    records = records_of(items)
    got, la, totals = check(acc, records, anchors_of(records, 2 * m), plan, m)
    by = {(int(r["pos"]), int(r["length"]), int(r["bases"]), int(r["ambiguous"])): int(r["count"]) for r in got}
    assert by == {(5, 3, I.pack(b"GAT"), 0): 7, (7, 2, I.pack(b"AT"), 0): 7, (9, 3, I.pack(b"CAA"), 0): 1, (9, 3, I.pack(b"CAC"), 0): 5, (9, 3, I.pack(b"CAG"), 0): 4,
                  (11, 15, I.pack(b"ACGTACGTACGTACG"), 0): 7, (13, 4, 0, 1): 2, (13, 18, 0, 1): 7}
    assert totals["folded"] == len(items) and totals["dropped"] == 0


def test_locus_records_through_the_insertion_call(acc):
    """The 2 + 2 of 40 + 40 cell: no call under either probe at min_alt 3, one call of 4 of 80 at the locus; the folded arrays go through the existing
    mipgen_accel_insertion_call_tables and equal the oracle's calls on the oracle's fold."""
    m = 12
    plan = pair_plan(m)
    rc_gat = I.pack(b"ATC")
    records = records_of([((4, 3, I.pack(b"GAT")), 2, False), ((m + (m - 1 - 4) - 1, 3, rc_gat), 2, False)])
    anchors = np.zeros((2 * m, 4), dtype=np.int32)
    anchors[:, 0] = 40
    anchors[4][1] = anchors[m + (m - 1 - 4) - 1][1] = 2
    p = CR.params(min_depth=20, min_alt=3, min_ppm=0, min_q=0, a0=1, n0=1024, bg_max_ppm=200000)
    empty = np.zeros(0, dtype=capi.INSERTION_POOL_RECORD_DTYPE)
    probe_calls, _t = acc.insertion_call_tables(records, anchors[:, 0], empty, np.full(2 * m, 400, dtype=np.int32), False, capi.CallParams(**p))
    assert len(probe_calls) == 0
    got, la, totals = check(acc, records, anchors, plan, m)
    assert len(got) == 1 and (int(got[0]["pos"]), int(got[0]["count"]), int(got[0]["bases"])) == (4, 4, I.pack(b"GAT")) and int(la[4][0]) == 80
    S = np.full(m, 800, dtype=np.int32)
    calls, ct = acc.insertion_call_tables(got, la[:, 0], empty, S, False, capi.CallParams(**p))
    want, w_la, _w = IL.fold(records, anchors, plan, m)
    w_totals, cands = IC.call_cells(IC.Row(w_la, want), IC.pool_lookup(empty, S), False, p)
    assert w_totals["excluded"] == 0 and IC.kept_calls(cands, p) == [tuple(int(v) for v in r) for r in calls] and len(calls) == 1
    assert (int(calls[0]["pos"]), int(calls[0]["depth"]), int(calls[0]["alt"])) == (4, 80, 4)


def test_refusals_and_state():
    a = capi.Accel(capi.make_params(130, 140))
    try:
        lib, h = a.lib, a.h
        i32p, i64p = capi.C.POINTER(capi.C.c_int32), capi.C.POINTER(capi.C.c_int64)
        out = np.zeros(8, dtype=capi.INSERTION_RECORD_DTYPE)
        assert lib.mipgen_accel_locus_insertions_fetch(h, out.ctypes.data, 0) == E_STATE and b"holds no locus insertion alleles" in lib.mipgen_accel_last_error()
        assert lib.mipgen_accel_locus_insertion_call_fetch(h, None, 0) == E_STATE
        assert lib.mipgen_accel_locus_insertion_pool_fetch(h, None, 0, None) == E_STATE                          # no consensus reads
        assert lib.mipgen_accel_reads_consensus_locus_insertion_call(h, 0, capi.C.byref(capi.CallParams()), None, None, None, None, None, None) == E_STATE
        assert lib.mipgen_accel_reads_consensus_locus_insertion_pool(h, b"ACGT", np.array([4], dtype=np.int32).ctypes.data_as(i32p), 1, 1, 0, 4, 200000, None) == E_STATE
        assert lib.mipgen_accel_reads_consensus_locus_insertions(h, b"ACGT", np.array([4], dtype=np.int32).ctypes.data_as(i32p), 1, 0, 1, 0, 4, None, None, None, None,
                                                                 None) == E_STATE
        good = records_of([((1, 1, 0), 10, False), ((2, 2, 3), 5, False)])
        anchors = anchors_of(good, 4)
        good_plan = np.array([0, 4, 8 + 2, -1], dtype=np.int64)
        tot = capi.LocusInsertionTotals()

        def call(records=good, n_records=None, anchors_=anchors, plan=good_plan, n_pos=4, n_loci=3):
            return lib.mipgen_accel_locus_insertion_tables(h, records.ctypes.data if records is not None else None, len(records) if n_records is None else n_records,
                                                           anchors_.ctypes.data_as(i32p) if anchors_ is not None else None,
                                                           plan.ctypes.data_as(i64p) if plan is not None else None, n_pos, n_loci, None, capi.C.byref(tot))

        def edited(arr, i, **kw):
            o = arr.copy()
            for k, v in kw.items():
                o[k][i] = v
            return o

        bad = [{"plan": None}, {"n_loci": 0}, {"n_loci": 1 << 29}, {"n_pos": 0}, {"n_pos": 1 << 29}, {"plan": np.array([0, 4, -2, -1], dtype=np.int64)},
               {"plan": np.array([0, 4, 12, -1], dtype=np.int64)}, {"plan": np.array([2, 4, 8, -1], dtype=np.int64)},      # below -1; locus 3 of 3; bit 1 at x = 0
               {"anchors_": None}, {"records": None, "n_records": 2}, {"n_records": -1}, {"n_records": 1 << 29},
               {"records": edited(good, 1, pos=4)}, {"records": edited(good, 0, pos=-1)}, {"records": good[::-1].copy()}, {"records": np.concatenate([good[:1], good[:1]])},
               {"records": edited(good, 0, length=0)}, {"records": edited(good, 1, length=16)}]
        for kw in bad:
            assert call(**kw) == E_INVALID, kw
        assert lib.mipgen_accel_locus_insertions_fetch(h, out.ctypes.data, 0) == E_STATE                          # nothing was run by any of them
        assert call() == 0 and (tot.alleles, tot.folded, tot.dropped) == (2, 2, 1)                                # row 1 under positions 1 and 2 (bit 1); row 2 by none
        for n in (0, 1, 3, -1):
            assert lib.mipgen_accel_locus_insertions_fetch(h, out.ctypes.data, n) == E_INVALID, n
        assert lib.mipgen_accel_locus_insertions_fetch(h, None, 2) == E_INVALID
        assert lib.mipgen_accel_locus_insertions_fetch(h, out.ctypes.data, 2) == 0 and out["pos"][:2].tolist() == [1, 2] and out["count"][:2].tolist() == [10, 10]
        assert call(n_pos=0) == E_INVALID and lib.mipgen_accel_locus_insertions_fetch(h, out.ctypes.data, 2) == 0   # a refused call leaves the records of the last one
        # the other lists of the handle: none was made, and this call left none
        assert lib.mipgen_accel_call_fetch(h, None, 0) == E_STATE and lib.mipgen_accel_insertion_call_fetch(h, None, 0) == E_STATE
        # timing index 17 and no other
        a.set_timing(True)
        assert a.last_kernel_ms(17) < 0
        assert call() == 0 and a.last_kernel_ms(17) > 0 and all(a.last_kernel_ms(k) < 0 for k in range(11, 17))
        assert call(records=good[:0], n_records=0) == 0 and tot.alleles == 0 and lib.mipgen_accel_locus_insertions_fetch(h, None, 0) == 0
        a.set_timing(False)
    finally:
        a.close()
