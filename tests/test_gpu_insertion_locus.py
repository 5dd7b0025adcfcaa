"""GPU: insertion alleles per genome locus end to end from reads (mipgen_accel_reads_consensus_locus_insertions, _locus_insertion_pool, _locus_insertion_call and their
fetches, `mipgen_count -insertion_loci / -call_insertion_loci`).  Six probes on a golden genome, molecules of 65 and 40 bases, W = 4: a plus / minus pair
on the same bases, two overlapping plus probes, and a plus / minus pair around a run of one base; two samples and undetermined, a few dozen molecules per cell.
Planted: +GGC split 2 + 2 of 40 + 40 over the strand pair of sample_a - no probe calls it, the locus does -, +GCC as 5 + 3 in sample_b, an insertion in the overlap
of the same-strand pair, and the repeated base once more inside its run, seen from both strands.  Every comparison is exact equality against
tests/insertion_locus_ref.py on the groups the device itself fetched, after the one exclusion of the call model (a candidate whose exact score lies within 1e-6 of
an integer is dropped from both sides, at most 1 in 1,000: asserted as `budget`)."""
import faulthandler
import re

import numpy as np
import pytest

from mipgen_amd import capi
from tests import call_ref as CR
from tests import consensus_ref as CONS
from tests import gapped_ref as G
from tests import helpers as H
from tests import insertion_call_ref as IC
from tests import insertion_locus_ref as IL
from tests import insertion_ref as I
from tests import locus_ref as LR
from tests import reads_ref as R
from tests.test_gpu_gapped import variant
from tests.test_gpu_insertions import with_insert
from tests.test_gpu_pileup import COUNT_BIN, TAGS, Lane, _run, write_fastq_q
from tests.test_gpu_reads import _accel, random_tag
from tests.test_gpu_samples import draw_barcodes
from tests.test_pileup_cpu import clean_window, synthetic_row
from tests.test_reads_cpu import HEADER

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE = -1, -6
W, ARM = 4, 16
LABELS = ["sample_a", "sample_b"]
P1 = CR.params(min_depth=20, min_alt=3, min_ppm=0, min_q=0, a0=1, n0=1024, bg_max_ppm=200000)     # (n0 no power of 10: k = n under the prior alone is no integer score)


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test's device work runs under a time limit of its own: a stuck call ends the process with a traceback instead of holding the GPU."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def quiet_positions(g, lo, hi):
    """The 1-based genome positions P in [lo, hi) with g at P and P + 1 both A or T: a run of G and C planted between them can neither slide nor be split."""
    return [P for P in range(lo, hi) if g[P - 1] in b"AT" and g[P] in b"AT"]


def plant(M, row, P, X):
    """The molecule of table row `row` with the plus-strand bases X inserted between genome positions P and P + 1."""
    if row[17] == b"+":
        return with_insert(M, P - int(row[3]) + 1, X)
    return with_insert(M, int(row[4]) - P, R.revcomp(X))


def build_design():
    """(genome, table rows, sites): rows 0 / 1 a plus / minus pair of 65 bases, rows 2 / 3 two plus probes of 40 bases four apart, rows 4 / 5 a plus / minus pair of
    65 bases around the first run of exactly six equal A or T bases behind them.  sites: the positions of the planted insertions in genome terms."""
    g = H.golden_genome()
    a0 = clean_window(g, 5000, 65)
    b0 = clean_window(g, a0 + 300, 44)
    c0 = None
    for m in re.finditer(rb"(?<![AT])(A{6}|T{6})(?![AT])", g):
        at = m.start() + 1 - 29                                              # 1-based: the run is at + 29 .. at + 34, inside the target at + 16 .. at + 48
        if at >= 1 and at + 64 < a0 and set(g[at - 1:at + 64]) <= set(b"ACGT"):
            c0 = at
            break
    assert c0 is not None
    rows = [synthetic_row(g, a0, a0 + 64, b"+", arm=ARM), synthetic_row(g, a0, a0 + 64, b"-", arm=ARM),
            synthetic_row(g, b0, b0 + 39, b"+", arm=ARM), synthetic_row(g, b0 + 4, b0 + 43, b"+", arm=ARM),
            synthetic_row(g, c0, c0 + 64, b"+", arm=ARM), synthetic_row(g, c0, c0 + 64, b"-", arm=ARM)]
    quiet = quiet_positions(g, a0 + ARM + 2, a0 + 64 - ARM - 2)
    assert len(quiet) >= 2 and quiet[-1] - quiet[0] >= 3
    sites = dict(split=quiet[0], both=quiet[-1], overlap=b0 + 21, run=(c0 + 29, g[c0 + 28:c0 + 29]))
    return g, rows, sites


def build_lane(rng, rows, sites, barcodes):
    mols = [r[6] + r[13] + r[10] for r in rows]
    L = Lane(rng)
    index = lambda s: barcodes[s] if s < 2 else random_tag(rng, 8)
    both = lambda p, Mv, s, times: [variant(L, mols[p], Mv, Mv, len(Mv), len(Mv), qual=ord("I"), index=index(s)) for _ in range(times)]
    for s in range(3):
        for p, M in enumerate(mols):
            for _ in range(38 if s == 0 and p < 2 else 12 if s < 2 else 5):
                L.molecule(M, len(M), len(M), qual=ord("I"), index=index(s))
    for p in (0, 1):
        both(p, plant(mols[p], rows[p], sites["split"], b"GGC"), 0, 2)                                      # 2 + 2 of 40 + 40
    both(0, plant(mols[0], rows[0], sites["both"], b"GCC"), 1, 5); both(1, plant(mols[1], rows[1], sites["both"], b"GCC"), 1, 3)
    both(0, plant(mols[0], rows[0], sites["both"], b"GCC"), 2, 1)                                           # undetermined shows it once
    both(2, plant(mols[2], rows[2], sites["overlap"], b"CC"), 1, 2); both(3, plant(mols[3], rows[3], sites["overlap"], b"CC"), 1, 4)
    both(3, plant(mols[3], rows[3], sites["overlap"], b"CG"), 0, 3)
    P, base = sites["run"]
    both(4, plant(mols[4], rows[4], P, base), 1, 3); both(5, plant(mols[5], rows[5], P, base), 1, 2)       # the run's base once more, somewhere in the run
    return mols, L


@pytest.fixture(scope="module")
def lane():
    """The design, the reads and everything the oracles make of them, computed once."""
    g, rows, sites = build_design()
    rng = np.random.default_rng(4519)
    barcodes = draw_barcodes(rng, 2, 8)
    mols, L = build_lane(rng, rows, sites, barcodes)
    cols = L.shuffled()
    arms = [(r[6], r[10]) for r in rows]
    ext, lig, eq, lq, idx = cols
    groups = CONS.consensus_reads(arms, ext, lig, eq, lq, idx, barcodes, 0, TAGS)[4]
    lens = [len(m) for m in mols]
    plans = {parts: LR.build_plan(rows, parts) for parts in ("target", "all")}
    folded = {parts: IL.session_rows(groups, mols, 3, plans[parts][0], len(plans[parts][1]), 1, 0, W) for parts in plans}
    return dict(g=g, rows=rows, sites=sites, barcodes=barcodes, mols=mols, lens=lens, arms=arms, cols=cols, groups=groups, plans=plans, folded=folded)


def open_session(acc, lane):
    ext, lig, eq, lq, idx = lane["cols"]
    assert acc.consensus_reads(lane["arms"], ext, lig, eq, lq, idx, lane["barcodes"], 0, TAGS)[4] == lane["groups"]


def locus_of(lane, parts, P):
    return lane["plans"][parts][1].index((b"1", P))


def spelt(rec):
    return I.unpack(int(rec["bases"]), int(rec["length"])).decode()


def same(a, b):
    return all(x.tobytes() == y.tobytes() if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def test_the_planted_cells_are_where_the_design_says(lane):
    """(Oracle only.)  The hand-worked cells in the oracle's rows: one record of k1 + k2 over n1 + n2 for the strand pair, the same-strand pair added up, the two
    lines at the two ends of the run."""
    sites = lane["sites"]
    at = np.cumsum([0] + lane["lens"])
    for parts in ("target", "all"):
        folded, (plan, loci, ref, sources) = lane["folded"][parts], lane["plans"][parts]
        anchors, records, lrec, la, totals = folded[0]
        l = locus_of(lane, parts, sites["split"])
        assert [(spelt(r), int(r["count"])) for r in lrec if int(r["pos"]) == l] == [("GGC", 4)] and int(la[l][0]) == 80 and sources[l] == 2
        probe = sorted((int(r["pos"]), spelt(r), int(r["count"])) for r in records if int(r["length"]) == 3 and int(r["count"]) == 2)
        assert [(s, k) for _x, s, k in probe] == [("GGC", 2), ("GCC", 2)] and probe[0][0] < at[1] <= probe[1][0]     # the minus probe's record is the reverse complement
        anchors, records, lrec, la, totals = folded[1]
        l = locus_of(lane, parts, sites["both"])
        assert [(spelt(r), int(r["count"])) for r in lrec if int(r["pos"]) == l] == [("GCC", 8)] and int(la[l][0]) == 12 + 5 + 12 + 3
        cc = [(int(r["pos"]), int(r["count"])) for r in lrec if spelt(r) == "CC"]
        assert len(cc) == 1 and cc[0][1] == 6 and sources[cc[0][0]] == 2                                    # 2 + 4 of the two overlapping plus probes
        # the run: the plus probe anchors the extra base in front of the run, the minus probe behind it - two locus alleles, as columns 6 and 7 of LOCI have them
        P, base = sites["run"]
        run = [(loci[int(r["pos"])][1], spelt(r), int(r["count"])) for r in lrec if loci[int(r["pos"])][1] in range(P - 1, P + 7)]
        assert run == [(P - 1, base.decode(), 3), (P + 5, base.decode(), 2)], run
        assert folded[2][2]["count"].tolist() == [1]                                                          # undetermined
    assert lane["folded"]["all"][0][4]["dropped"] <= lane["folded"]["target"][0][4]["dropped"]


def compare_fold(acc, lane, parts, row, res):
    counts, anchors, it, lrec, la, lt = res
    w_anchors, w_records, w_lrec, w_la, w_totals = lane["folded"][parts][row]
    assert np.array_equal(anchors, w_anchors) and acc.insertions_fetch(it["alleles"]).tobytes() == w_records.tobytes()
    assert lrec.tobytes() == w_lrec.tobytes(), (row, lrec, w_lrec)
    assert np.array_equal(la, w_la) and lt == w_totals, (row, lt, w_totals)
    assert acc.locus_insertions_fetch(lt["alleles"]).tobytes() == lrec.tobytes()


@pytest.mark.parametrize("parts", ["target", "all"])
def test_fold_pool_and_calls_equal_the_oracle(lane, parts):
    mols, lens = lane["mols"], lane["lens"]
    plan, loci, ref, sources = lane["plans"][parts]
    folded = lane["folded"][parts]
    a = _accel()
    try:
        open_session(a, lane)
        plain = [a.consensus_insertions(mols, lens, r, 1, 0, W) for r in range(3)]
        a.consensus_locus_plan(plan, ref)
        for row in (1, 0, 2, 0):
            res = a.consensus_locus_insertions(mols, lens, row, 1, 0, W)
            assert same(res, a.consensus_locus_insertions(mols, lens, row, 1, 0, W))
            compare_fold(a, lane, parts, row, res)
            assert res[0].tobytes() == plain[row][0].tobytes() and res[1].tobytes() == plain[row][1].tobytes() and res[2] == plain[row][3]
            merged = a.consensus_locus_pileup(mols, lens, row, 1, 0, W)[1]
            IL.check_invariants(res[3], res[4], merged, plain[row][2], plan)
        # per probe, with the existing calls: the split insertion is not called
        a.consensus_insertion_pool(mols, lens, 1, 0, W, P1["bg_max_ppm"])
        probe_calls = a.consensus_insertion_call(0, capi.CallParams(**P1))[3]
        assert not any(spelt(r) in ("GGC", "GCC") for r in probe_calls)
        # per locus
        rows = [IC.Row(la, lrec) for _a, _r, lrec, la, _t in folded]
        budget = [0, 0]
        for p in (P1, dict(P1, min_alt=2, bg_max_ppm=500000)):
            totals = a.consensus_locus_insertion_pool(mols, lens, 1, 0, W, p["bg_max_ppm"])
            w_pool, w_S = IC.sparse_pool(rows[:2], p["bg_max_ppm"])
            assert totals == {"rows": 2, "entries": sum(len(r.count) for r in rows[:2]), "alleles": len(w_pool)}, totals
            pool, S = a.locus_insertion_pool_fetch(totals["alleles"])
            assert pool.tobytes() == w_pool.tobytes() and np.array_equal(S, w_S) and len(S) == len(loci)
            with pytest.raises(RuntimeError):
                a.locus_insertions_fetch(0)                                                                   # (the pool's last row is no locus insertions call)
            oracle = IL.call_rows(folded, True, p)
            for row in (2, 0, 1, 0):
                res = a.consensus_locus_insertion_call(row, capi.CallParams(**p))
                assert same(res, a.consensus_locus_insertion_call(row, capi.CallParams(**p)))
                compare_fold(a, lane, parts, row, res[:6])
                recs, ct = res[6], res[7]
                w_totals, cands = oracle[row]
                assert {k: ct[k] for k in ("tested", "too_deep", "candidates")} == {k: w_totals[k] for k in ("tested", "too_deep", "candidates")}, (row, ct, w_totals)
                assert IC.drop_excluded(recs, cands) == IC.kept_calls(cands, p), (row, recs, cands)
                assert w_totals["calls"] <= ct["calls"] <= w_totals["calls"] + w_totals["excluded"] and not recs["reserved"].any()
                assert a.locus_insertion_call_fetch(len(recs)).tobytes() == recs.tobytes()
                budget[0] += w_totals["candidates"]; budget[1] += w_totals["excluded"]
                if row == 0 and p is P1:                                                                      # the 2 + 2 cell is called at the locus: 4 of 80
                    l = locus_of(lane, parts, lane["sites"]["split"])
                    assert [(int(r["depth"]), int(r["alt"]), spelt(r)) for r in recs if int(r["pos"]) == l] == [(80, 4, "GGC")]
            with pytest.raises(RuntimeError, match="bg_max_ppm"):
                a.consensus_locus_insertion_call(0, capi.CallParams(**dict(p, bg_max_ppm=p["bg_max_ppm"] + 1)))
        assert budget[0] >= 8 and budget[1] * 1000 <= budget[0]
        # the calls per probe are still the last insertion call's
        assert a.insertion_call_fetch(len(probe_calls)).tobytes() == probe_calls.tobytes()
    finally:
        a.close()


def test_the_other_calls_the_timing_and_a_second_plan(lane):
    """The plain insertions call, an insertion call, a locus pileup and a locus call made before the new calls return the same bytes after them; index 17 is set by
    every new call and no other index by any; a second plan drops the locus insertion pool."""
    mols, lens = lane["mols"], lane["lens"]
    plan, loci, ref, sources = lane["plans"]["target"]
    a = _accel()
    try:
        open_session(a, lane)
        params = capi.CallParams(**P1)

        def others():
            a.consensus_locus_plan(plan, ref)
            a.consensus_insertion_pool(mols, lens, 1, 0, W, P1["bg_max_ppm"])
            a.consensus_locus_call_pool(mols, lens, 1, 0, W, P1["bg_max_ppm"])
            out = [a.consensus_insertions(mols, lens, 1, 1, 0, W), a.consensus_insertion_call(1, params), a.consensus_locus_pileup(mols, lens, 1, 1, 0, W),
                   a.consensus_locus_call(1, params)]
            return [[x.tobytes() if isinstance(x, np.ndarray) else x for x in o] for o in out]

        before = others()
        n_ins_calls, n_locus_calls = len(a.consensus_insertion_call(1, params)[3]), len(a.consensus_locus_call(1, params)[2])
        a.set_timing(True)
        assert a.last_kernel_ms(17) < 0
        seen = [a.last_kernel_ms(k) for k in range(4, 17)]
        a.consensus_locus_insertions(mols, lens, 1, 1, 0, W)
        assert a.last_kernel_ms(17) > 0 and [a.last_kernel_ms(k) for k in range(4, 17)] == seen
        a.consensus_locus_insertion_pool(mols, lens, 1, 0, W, P1["bg_max_ppm"])
        assert a.last_kernel_ms(17) > 0 and [a.last_kernel_ms(k) for k in range(4, 17)] == seen
        for row in (1, 0, 2):
            a.consensus_locus_insertion_call(row, params)
            assert a.last_kernel_ms(17) > 0 and [a.last_kernel_ms(k) for k in range(4, 17)] == seen
        a.set_timing(False)
        assert len(a.insertion_call_fetch(n_ins_calls)) == n_ins_calls and len(a.call_fetch(n_locus_calls)) == n_locus_calls
        # a second plan drops the locus insertion pool and the anchor map; the fold under it is the oracle's
        plan_all, loci_all, ref_all, _s = lane["plans"]["all"]
        a.consensus_locus_plan(plan_all, ref_all)
        with pytest.raises(capi.AccelError, match=f"error {E_STATE}: .*no locus insertion pool"):
            a.consensus_locus_insertion_call(0, params)
        compare_fold(a, lane, "all", 1, a.consensus_locus_insertions(mols, lens, 1, 1, 0, W))
        assert others() == before
    finally:
        a.close()


def test_state_refusals_and_zero_groups(lane):
    mols, lens = lane["mols"], np.array(lane["lens"], dtype=np.int32)
    plan, loci, ref, sources = lane["plans"]["target"]
    a = _accel()
    try:
        lib, h, C = a.lib, a.h, capi.C
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        arr, seq, n = np.array(plan, dtype=np.int64), b"".join(mols), len(mols)
        prm = capi.CallParams(**P1)
        lt, pt, ct = capi.LocusInsertionTotals(), capi.InsertionPoolTotals(), capi.CallTotals()
        install = lambda: lib.mipgen_accel_reads_consensus_locus_plan(h, arr.ctypes.data_as(i64p), len(arr), ref, len(ref))
        fold = lambda seq_=seq, lens_=lens, n_=n, row=0, W_=W: lib.mipgen_accel_reads_consensus_locus_insertions(h, seq_, lens_.ctypes.data_as(i32p), n_, row, 1, 0, W_, None, None,
                                                                                                             None, None, C.byref(lt))
        pool = lambda seq_=seq, W_=W, bg=200000: lib.mipgen_accel_reads_consensus_locus_insertion_pool(h, seq_, lens.ctypes.data_as(i32p), n, 1, 0, W_, bg, C.byref(pt))
        call = lambda row=0, prm_=prm: lib.mipgen_accel_reads_consensus_locus_insertion_call(h, row, C.byref(prm_) if prm_ is not None else None, None, None, None, None, None,
                                                                                            C.byref(ct))
        pfetch = lambda k: lib.mipgen_accel_locus_insertion_pool_fetch(h, np.zeros(max(k, 1), dtype=capi.INSERTION_POOL_RECORD_DTYPE).ctypes.data, k, None)
        for f in (fold, pool, call, lambda: pfetch(0)):
            assert f() == E_STATE and b"holds no consensus reads" in lib.mipgen_accel_last_error()
        assert lib.mipgen_accel_locus_insertions_fetch(h, None, 0) == E_STATE and lib.mipgen_accel_locus_insertion_call_fetch(h, None, 0) == E_STATE   # before any call
        # a session without groups: no plan is STATE; with one, zeros
        arms = capi.probe_array(lane["arms"])
        assert lib.mipgen_accel_reads_open_consensus(h, arms, n, 8, 0, 0, None, 0, 0, 0) == 0
        assert lib.mipgen_accel_reads_finish_consensus(h, None, None, None, None, None, None) == 0
        for f in (fold, pool, call):
            assert f() == E_STATE and b"no locus plan" in lib.mipgen_accel_last_error()
        assert install() == 0
        la = np.full((len(loci), 4), -1, dtype=np.int32)
        assert lib.mipgen_accel_reads_consensus_locus_insertions(h, seq, lens.ctypes.data_as(i32p), n, 0, 1, 0, W, None, None, la.ctypes.data_as(i32p), None, C.byref(lt)) == 0
        assert not la.any() and (lt.loci, lt.alleles, lt.folded, lt.dropped) == (0, 0, 0, 0) and lib.mipgen_accel_locus_insertions_fetch(h, None, 0) == 0
        assert call() == E_STATE and b"no locus insertion pool" in lib.mipgen_accel_last_error() and pfetch(0) == E_STATE
        assert pool() == 0 and (pt.rows, pt.entries, pt.alleles) == (1, 0, 0) and pfetch(0) == 0 and pfetch(1) == E_INVALID
        assert call() == 0 and (ct.tested, ct.candidates, ct.calls) == (0, 0, 0) and lib.mipgen_accel_locus_insertion_call_fetch(h, None, 0) == 0
        # reads: the plan and the pool went with the old ones
        ext, lig, eq, lq, idx = lane["cols"]
        a.consensus_reads(lane["arms"], ext, lig, eq, lq, idx, lane["barcodes"], 0, TAGS)
        assert fold() == E_STATE and call() == E_STATE and install() == 0 and call() == E_STATE
        # every refusal of the insertions call, and a table that is not the plan's
        short = lens.copy(); short[-1] -= 1
        for kw in (dict(seq_=None), dict(n_=n - 1), dict(row=3), dict(row=-1), dict(W_=0), dict(W_=16), dict(lens_=np.zeros(n, dtype=np.int32))):
            assert fold(**kw) == E_INVALID, kw
        assert fold(lens_=short) == E_INVALID and b"the locus plan was installed for" in lib.mipgen_accel_last_error()
        for kw in (dict(seq_=None), dict(W_=0), dict(bg=-1), dict(bg=1000001)):
            assert pool(**kw) == E_INVALID, kw
        assert call() == E_STATE                                                                                # a refused pool leaves none
        assert fold() == 0 and lt.alleles > 0
        out = np.zeros(int(lt.alleles) + 1, dtype=capi.INSERTION_RECORD_DTYPE)
        assert lib.mipgen_accel_locus_insertions_fetch(h, out.ctypes.data, lt.alleles + 1) == E_INVALID and lib.mipgen_accel_locus_insertions_fetch(h, out.ctypes.data, lt.alleles) == 0
        assert pool() == 0 and call() == 0 and ct.calls > 0
        assert lib.mipgen_accel_locus_insertion_call_fetch(h, None, ct.calls + 1) == E_INVALID
        assert call(row=3) == E_INVALID and call(prm_=None) == E_INVALID and call(prm_=capi.CallParams(min_alt=0)) == E_INVALID
        assert call(prm_=capi.CallParams(bg_max_ppm=1)) == E_STATE and b"locus insertion pool was built with" in lib.mipgen_accel_last_error()
        assert install() == 0 and call() == E_STATE and pfetch(0) == E_STATE                                  # a plan replaced: the pool is gone
        assert lib.mipgen_accel_reads_open(h, arms, n, 8, 0, 0) == 0 and call() == E_STATE and fold() == E_STATE
        assert lib.mipgen_accel_reads_finish(h, None, None, None) == 0
    finally:
        a.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_barcodes", [False, True])
def test_cli_equals_the_oracle(tmp_path, lane, with_barcodes):
    """The design of this file through `mipgen_count`, -barcodes on both strands: ILOCI, ILCALLS and the new last stderr lines are the oracle's; FILE, INS, ICALLS,
    LOCI, CALLS, stdout and every other stderr line are those of the run without the new options."""
    rows, mols = lane["rows"], lane["mols"]
    ext, lig, eq, lq, idx = lane["cols"]
    with open(tmp_path / "table.txt", "wb") as fh:
        fh.write(HEADER.encode() + b"".join(b"\t".join(r) + b"\n" for r in rows))
    write_fastq_q(tmp_path / "ext.fq", ext, eq); write_fastq_q(tmp_path / "lig.fq", lig, lq)
    write_fastq_q(tmp_path / "i1.fq", idx, [b"I" * 8] * len(idx))
    with open(tmp_path / "samples.tsv", "wb") as fh:
        fh.write(b"\n".join(l.encode() + b"\t" + b for l, b in zip(LABELS, lane["barcodes"])) + b"\n")
    common = [COUNT_BIN, "-tag_sizes", "8,0", "-reads", "ext.fq", "lig.fq", "table.txt", "-o", "counts.tsv"] + (
        ["-barcodes", "samples.tsv", "-index_reads", "i1.fq"] if with_barcodes else [])
    groups = lane["groups"] if with_barcodes else CONS.consensus_reads(lane["arms"], ext, lig, eq, lq, None, None, 0, TAGS)[4]
    lab = LABELS if with_barcodes else None
    opts = ["-call_min_depth", "20", "-call_min_alt", "3", "-call_min_q", "0", "-call_prior", "1,1024"]
    old = ["-pileup_indels", str(W), "-pileup_insertions", "{}ins.tsv", "-call_insertions", "{}icalls.tsv", "-pileup_loci", "{}loci.tsv", "-call_loci", "{}lcalls.tsv"]
    files = lambda tag: [a.format(tag) for a in old]
    text, line, calls, cline, excluded = IL.files(groups, rows, lab, P1, "target", 1, 0, W)
    assert excluded == 0 and text.count(b"\n") > 4 and calls.count(b"\n") >= 2
    base = _run(common + ["-pileup", "0pile.tsv"] + files("0") + opts, str(tmp_path))
    assert base.returncode == 0, base.stderr.decode()
    one = _run(common + ["-pileup", "1pile.tsv"] + files("1") + opts + ["-insertion_loci", "iloci1.tsv"], str(tmp_path))
    assert one.returncode == 0, one.stderr.decode()
    assert open(tmp_path / "iloci1.tsv", "rb").read() == text
    assert one.stderr.decode() == base.stderr.decode() + line and one.stdout == base.stdout
    two = _run(common + ["-pileup", "2pile.tsv"] + files("2") + opts + ["-insertion_loci", "iloci2.tsv", "-call_insertion_loci", "ilcalls2.tsv"], str(tmp_path))
    assert two.returncode == 0, two.stderr.decode()
    assert open(tmp_path / "iloci2.tsv", "rb").read() == text and open(tmp_path / "ilcalls2.tsv", "rb").read() == calls
    assert two.stderr.decode() == base.stderr.decode() + line + cline and two.stdout == base.stdout
    for name in ("pile.tsv", "ins.tsv", "icalls.tsv", "loci.tsv", "lcalls.tsv"):
        want = open(tmp_path / ("0" + name), "rb").read()                     # (no substitution is planted: the variant call files may hold their header alone)
        assert want.count(b"\n") >= 1 and open(tmp_path / ("1" + name), "rb").read() == want and open(tmp_path / ("2" + name), "rb").read() == want, name
    assert open(tmp_path / "counts.tsv", "rb").read() != b""
    # without the per-probe calls beside it: the same two files
    lean = _run(common + ["-pileup", "3pile.tsv", "-pileup_indels", str(W), "-pileup_insertions", "3ins.tsv", "-pileup_loci", "3loci.tsv", "-insertion_loci", "iloci3.tsv",
                          "-call_insertion_loci", "ilcalls3.tsv"] + opts, str(tmp_path))
    assert lean.returncode == 0, lean.stderr.decode()
    assert open(tmp_path / "iloci3.tsv", "rb").read() == text and open(tmp_path / "ilcalls3.tsv", "rb").read() == calls
    assert open(tmp_path / "3pile.tsv", "rb").read() == open(tmp_path / "0pile.tsv", "rb").read() and open(tmp_path / "3ins.tsv", "rb").read() == open(tmp_path / "0ins.tsv", "rb").read()
    if with_barcodes:                                                         # the split insertion: a line of ILCALLS, no line of ICALLS
        split = b"%d" % lane["sites"]["split"]
        assert any(l.startswith(b"sample_a\t1\t" + split + b"\t3\tGGC\t80\t4\t") for l in calls.split(b"\n"))
        assert not any(b"\tGGC\t" in l or b"\tGCC\t" in l for l in open(tmp_path / "0icalls.tsv", "rb").read().split(b"\n") if l.startswith(b"sample_a\t"))
