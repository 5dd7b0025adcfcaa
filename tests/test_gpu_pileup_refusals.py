"""GPU: the refusals of every entry point of accel_pileup.hip, pinned: code, whole text and order.  One session of two probes (molecules of 33 and
40 bases), two barcodes plus undetermined and a dozen read pairs.  For every adjacent pair of refusals in a function's source order one call violates both and must
get the first; the expected texts are literals.  Then what a refusal leaves behind: no pool after a refused pool call, no locus pool after a second plan, no pileup
totals before a call has succeeded or after a pool was rebuilt.  MIPGEN_E_NOMEM is not provoked (no test can exhaust a device others share), the refusal of more than
2^31 - 1 rounds of 64 cannot be reached with two probes, and nothing here tries to make the device fault: every refused call returns before it allocates or launches."""
import faulthandler

import numpy as np
import pytest

from mipgen_amd import capi, synth
from tests.test_gpu_pileup import TAGS, Lane, cut_probes
from tests.test_gpu_reads import _accel, random_tag
from tests.test_gpu_samples import draw_barcodes

pytestmark = pytest.mark.gpu
C = capi.C
OK, E_INVALID, E_STATE = 0, -1, -6
I32P, I64P = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
LENS, N_POS, ROWS = (33, 40), 73, 3
NO_HANDLE = "null handle"
NO_READS = "the handle holds no consensus reads: mipgen_accel_reads_finish_consensus leaves them, the next mipgen_accel_reads_open* drops them"
NO_LENS = "bad arguments: no molecule lengths"
NO_SEQ = "bad arguments: no template bases"
NO_PLAN = "the consensus reads have no locus plan: mipgen_accel_reads_consensus_locus_plan installs it"
NO_POOL = "the consensus reads have no pool: mipgen_accel_reads_consensus_call_pool builds it"
NO_LOCUS_POOL = "the consensus reads have no locus pool: mipgen_accel_reads_consensus_locus_call_pool builds it"
NO_ROW = "no row was called: mipgen_accel_reads_consensus_call counts one"
NO_LOCUS_ROW = "no row was called per locus: mipgen_accel_reads_consensus_locus_call counts one"
NO_CALLS = "the handle holds no calls: mipgen_accel_call_tables or mipgen_accel_reads_consensus_call leaves them"


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test's device work runs under a time limit of its own: a stuck call ends the process with a traceback instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lane():
    """Two molecules per (sample, probe), one of them read twice, and two undetermined ones: 14 read pairs."""
    rng = np.random.default_rng(4160)
    mols, arms = cut_probes(synth.random_genome(40000, 17), list(LENS))
    barcodes = draw_barcodes(rng, 2, 8)
    L = Lane(rng)
    for s in range(3):
        for p, M in enumerate(mols):
            for k in range(2 if s < 2 else 1):
                L.molecule(M, len(M), len(M), family=2 - k if s < 2 else 1, qual=ord("I"), index=barcodes[s] if s < 2 else random_tag(rng, 8))
    assert len(L.ext) == 14
    return dict(mols=mols, arms=arms, barcodes=barcodes, cols=L.shuffled(), seq=b"".join(mols))


class Handle:
    """The entry points with the arguments of a call that succeeds as defaults; every method returns the code, `refused` compares code and text."""

    def __init__(self, lane, with_reads=True):
        self.a = _accel()
        self.lib, self.h, self.seq = self.a.lib, self.a.h, lane["seq"]
        self.lens = np.array(LENS, dtype=np.int32)
        self.plan_arr = np.arange(N_POS, dtype=np.int64) * 4                      # every template position a locus of its own, plus strand
        self.ref = lane["seq"]
        self.prm = capi.CallParams()
        if with_reads:
            self.open(lane)

    def open(self, lane):
        ext, lig, eq, lq, idx = lane["cols"]
        groups = self.a.consensus_reads(lane["arms"], ext, lig, eq, lq, idx, lane["barcodes"], 0, TAGS)[4]
        assert len(groups) == 10                                                  # 2 per (sample, probe), 1 per probe undetermined

    def close(self):
        self.a.close()

    def refused(self, rc, code, text):
        got = self.lib.mipgen_accel_last_error().decode()
        assert (rc, got) == (code, text)

    @staticmethod
    def _lens(lens):
        return None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)

    def pileup(self, h=True, lens=LENS, n=2, row=0, mf=1, mq=0):
        l = self._lens(lens)
        return self.lib.mipgen_accel_reads_consensus_pileup(self.h if h else None, None if l is None else l.ctypes.data_as(I32P), n, row, mf, mq, None, None)

    def gapped(self, h=True, seq=True, lens=LENS, n=2, row=0, mf=1, mq=0, W=4):
        l = self._lens(lens)
        return self.lib.mipgen_accel_reads_consensus_pileup_gapped(self.h if h else None, self.seq if seq else None, None if l is None else l.ctypes.data_as(I32P), n, row,
                                                                   mf, mq, W, None, None)

    def pool(self, h=True, seq=True, lens=LENS, n=2, mf=1, mq=0, W=0, bg=200000):
        l = self._lens(lens)
        return self.lib.mipgen_accel_reads_consensus_call_pool(self.h if h else None, self.seq if seq else None, None if l is None else l.ctypes.data_as(I32P), n, mf, mq,
                                                               W, bg)

    def call(self, h=True, row=0, prm=True):
        return self.lib.mipgen_accel_reads_consensus_call(self.h if h else None, row, C.byref(self.prm) if prm else None, None, None)

    def totals(self, h=True):
        return self.lib.mipgen_accel_reads_consensus_call_pileup_totals(self.h if h else None, None)

    def plan(self, h=True, plan=True, n_pos=N_POS, ref=True, n_loci=N_POS):
        arr = self.plan_arr if plan is True else plan
        return self.lib.mipgen_accel_reads_consensus_locus_plan(self.h if h else None, None if arr is None else arr.ctypes.data_as(I64P), n_pos, self.ref if ref else None,
                                                                n_loci)

    def locus_pileup(self, h=True, seq=True, lens=LENS, n=2, row=0, mf=1, mq=0, W=0):
        l = self._lens(lens)
        return self.lib.mipgen_accel_reads_consensus_locus_pileup(self.h if h else None, self.seq if seq else None, None if l is None else l.ctypes.data_as(I32P), n, row,
                                                                  mf, mq, W, None, None, None, None)

    def locus_pool(self, h=True, seq=True, lens=LENS, n=2, mf=1, mq=0, W=0, bg=200000):
        l = self._lens(lens)
        return self.lib.mipgen_accel_reads_consensus_locus_call_pool(self.h if h else None, self.seq if seq else None, None if l is None else l.ctypes.data_as(I32P), n,
                                                                     mf, mq, W, bg)

    def locus_call(self, h=True, row=0, prm=True):
        return self.lib.mipgen_accel_reads_consensus_locus_call(self.h if h else None, row, C.byref(self.prm) if prm else None, None, None, None)

    def locus_totals(self, h=True):
        return self.lib.mipgen_accel_reads_consensus_locus_call_pileup_totals(self.h if h else None, None)


@pytest.fixture()
def H(lane):
    x = Handle(lane)
    yield x
    x.close()


def walk_row_ladder(H, f, gapped, rows=True, lens_name="pileup"):
    """The refusals of plan_row behind entry point f, from the molecule lengths on.  gapped: f takes template bases and places them (max_indel 1..15)."""
    seq = dict(seq=False) if gapped else {}
    H.refused(f(lens=None, n=3, **seq), E_INVALID, NO_LENS)
    if gapped:
        H.refused(f(seq=False, n=3), E_INVALID, NO_SEQ)
    H.refused(f(n=3, lens=(0, 40, 40)), E_INVALID, "3 molecule lengths: the session that left the consensus reads had 2 probes")
    H.refused(f(lens=(0, -1), mf=0), E_INVALID, "molecule length 0 of probe 0: a length is 1 or more")
    if gapped:
        H.refused(f(lens=(2049, 0)), E_INVALID, "molecule length 2049 of probe 0: the gapped pileup places molecules of at most 2048 bases")
        H.refused(f(lens=(33, 0), W=16), E_INVALID, "molecule length 0 of probe 1: a length is 1 or more")
    if rows:
        H.refused(f(lens=(33, -2), row=3), E_INVALID, "molecule length -2 of probe 1: a length is 1 or more")
        H.refused(f(row=3, mf=0), E_INVALID, "row 3: the session had 3 rows")
        H.refused(f(row=-1, mf=0), E_INVALID, "row -1: the session had 3 rows")
    H.refused(f(mf=0, mq=41), E_INVALID, "min_family 0: 1 or more")
    H.refused(f(mq=41, **(dict(W=16) if gapped else {})), E_INVALID, "min_quality 41: 0 to 40 (the consensus writes 2 to 40)")
    H.refused(f(mq=-1), E_INVALID, "min_quality -1: 0 to 40 (the consensus writes 2 to 40)")


def walk_call_params(H, f):
    """The refusals of the call parameters behind f(prm=...), which reads H.prm."""
    H.refused(f(prm=False), E_INVALID, "bad arguments: no call parameters")
    steps = [(dict(min_depth=0, min_alt=0), "min_depth 0: 1 or more"),
             (dict(min_alt=0, min_ppm=-1), "min_alt 0: 1 or more"),
             (dict(min_ppm=1000001, min_q=10000), "min_ppm 1000001: 0 to 1000000"),
             (dict(min_ppm=-1, min_q=10000), "min_ppm -1: 0 to 1000000"),
             (dict(min_q=10000, a0=0), "min_q 10000: 0 to 9999"),
             (dict(min_q=-1, a0=0), "min_q -1: 0 to 9999"),
             (dict(a0=0, bg_max_ppm=-1), "prior 0 / 1000: 0 < a0 < n0 <= 2^30"),
             (dict(a0=5, n0=5, bg_max_ppm=-1), "prior 5 / 5: 0 < a0 < n0 <= 2^30"),
             (dict(n0=(1 << 30) + 1, bg_max_ppm=-1), "prior 1 / 1073741825: 0 < a0 < n0 <= 2^30"),
             (dict(bg_max_ppm=-1), "bg_max_ppm -1: 0 to 1000000"),
             (dict(bg_max_ppm=1000001), "bg_max_ppm 1000001: 0 to 1000000")]
    for kw, text in steps:
        H.prm = capi.CallParams(**kw)
        H.refused(f(), E_INVALID, text)
    H.prm = capi.CallParams()


def walk_locus_plan(H, f):
    """The refusals of a plan behind f(plan=, n_pos=, n_loci=); no refused call reads the plan beyond the entry it names."""
    arr = lambda *v: np.array(v, dtype=np.int64)
    H.refused(f(plan=None, n_loci=0), E_INVALID, "bad arguments: no locus plan")
    H.refused(f(n_loci=0, n_pos=0), E_INVALID, "0 loci: 1 to 2^29 - 1")
    H.refused(f(n_loci=1 << 29, n_pos=0), E_INVALID, "536870912 loci: 1 to 2^29 - 1")
    H.refused(f(plan=arr(-2), n_pos=0), E_INVALID, "0 positions: 1 to 2^29 - 1")
    H.refused(f(plan=arr(-2), n_pos=1 << 29), E_INVALID, "536870912 positions: 1 to 2^29 - 1")
    H.refused(f(plan=arr(-2, 4 * N_POS), n_pos=2), E_INVALID, "locus plan entry -2 of position 0: -1 or locus * 4 + flags")
    H.refused(f(plan=arr(4 * N_POS + 2, -2), n_pos=2), E_INVALID, f"locus {N_POS} of position 0: the plan has {N_POS} loci")
    H.refused(f(plan=arr(6, -2), n_pos=2), E_INVALID, "locus plan entry 6 of position 0: bit 1 takes the insertion columns of row x - 1")
    H.refused(f(plan=arr(0, -1, 4 * N_POS + 2), n_pos=3), E_INVALID, f"locus {N_POS} of position 2: the plan has {N_POS} loci")


def test_without_consensus_reads(lane):
    """A null handle, then a handle that holds no reads: STATE comes before every refusal of an argument."""
    H = Handle(lane, with_reads=False)
    try:
        for f in (H.pileup, H.gapped, H.pool, H.call, H.totals, H.plan, H.locus_pileup, H.locus_pool, H.locus_call, H.locus_totals):
            H.refused(f(h=False), E_INVALID, NO_HANDLE)
        for f in (H.pileup, H.gapped, H.pool, H.locus_pileup, H.locus_pool):
            H.refused(f(lens=None, n=3), E_STATE, NO_READS)
        H.refused(H.call(row=-1, prm=False), E_STATE, NO_READS)
        H.refused(H.locus_call(row=-1, prm=False), E_STATE, NO_READS)
        H.refused(H.plan(ref=False, plan=None), E_STATE, NO_READS)
        H.refused(H.totals(), E_STATE, NO_ROW)
        H.refused(H.locus_totals(), E_STATE, NO_LOCUS_ROW)
    finally:
        H.close()


def test_pileup_and_gapped_pileup(H):
    walk_row_ladder(H, H.pileup, False)
    walk_row_ladder(H, H.gapped, True)
    H.refused(H.gapped(W=0), E_INVALID, "max_indel 0: 1 to 15")
    H.refused(H.gapped(W=16), E_INVALID, "max_indel 16: 1 to 15")
    assert H.pileup() == OK and H.gapped() == OK


def test_call_pool_and_call(H):
    # the pool: template bases are asked for at max_indel 0 too (they are the ref bytes), molecules are bounded only where they are placed
    H.refused(H.pool(seq=False, n=3), E_INVALID, NO_SEQ)
    walk_row_ladder(H, lambda **kw: H.pool(**{"W": 4, **kw}), True, rows=False)
    walk_row_ladder(H, H.pool, False, rows=False)
    H.refused(H.pool(mq=41, W=16), E_INVALID, "min_quality 41: 0 to 40 (the consensus writes 2 to 40)")
    H.refused(H.pool(W=16, bg=-1), E_INVALID, "max_indel 16: 1 to 15")
    H.refused(H.pool(W=-1, bg=-1), E_INVALID, "max_indel -1: 1 to 15")
    H.refused(H.pool(bg=-1, lens=(1 << 29, 40)), E_INVALID, "bg_max_ppm -1: 0 to 1000000")
    H.refused(H.pool(bg=1000001), E_INVALID, "bg_max_ppm 1000001: 0 to 1000000")
    H.refused(H.pool(lens=(1 << 29, 40)), E_INVALID, "536870952 template positions: a call takes 2^29 - 1 at most")
    # a pool call refused for an argument leaves no pool
    H.refused(H.call(row=9, prm=False), E_STATE, NO_POOL)
    H.refused(H.totals(), E_STATE, NO_ROW)
    # the call
    assert H.pool() == OK
    H.refused(H.totals(), E_STATE, NO_ROW)
    H.refused(H.call(row=3, prm=False), E_INVALID, "row 3: the session had 3 rows")
    H.refused(H.call(row=-1, prm=False), E_INVALID, "row -1: the session had 3 rows")
    walk_call_params(H, H.call)
    H.prm = capi.CallParams(bg_max_ppm=10)
    H.refused(H.call(), E_STATE, "bg_max_ppm 10: the pool was built with 200000")
    H.prm = capi.CallParams()
    H.refused(H.totals(), E_STATE, NO_ROW)                                        # no refused call counted a row
    assert H.call(row=2) == OK and H.totals() == OK
    H.refused(H.call(row=3), E_INVALID, "row 3: the session had 3 rows")
    assert H.totals() == OK                                                       # a call refused for an argument leaves the totals of the last one
    # a pool call refused for an argument leaves the pool that is held; a rebuilt pool has no row called
    H.refused(H.pool(bg=-1), E_INVALID, "bg_max_ppm -1: 0 to 1000000")
    assert H.call() == OK and H.totals() == OK
    assert H.pool(W=4) == OK
    H.refused(H.totals(), E_STATE, NO_ROW)
    assert H.call() == OK and H.totals() == OK


def test_call_tables_and_fetch(lane):
    H = Handle(lane, with_reads=False)
    try:
        lib, h = H.lib, H.h
        counts = np.array([[0, 30, 0, 0, 0]], dtype=np.int32)
        pool = np.zeros((1, 10), dtype=np.int32)
        tot = capi.CallTotals()

        def tables(h_=h, counts_=counts, columns=5, n_pos=1, prm=True):
            return lib.mipgen_accel_call_tables(h_, None if counts_ is None else counts_.ctypes.data_as(I32P), columns, pool.ctypes.data_as(I32P), b"A", n_pos, 1,
                                                C.byref(H.prm) if prm else None, C.byref(tot))

        fetch = lambda n, records=None, h_=h: lib.mipgen_accel_call_fetch(h_, None if records is None else records.ctypes.data, n)
        H.refused(fetch(5, h_=None), E_INVALID, NO_HANDLE)
        H.refused(fetch(5), E_STATE, NO_CALLS)
        H.refused(tables(h_=None), E_INVALID, NO_HANDLE)
        H.refused(tables(counts_=None, columns=6), E_INVALID, "bad arguments: no counts, no pool or no ref bytes")
        H.refused(tables(columns=6, n_pos=0), E_INVALID, "6 columns: 5 (the pileup's table) or 8 (the gapped one)")
        H.refused(tables(n_pos=0, prm=False), E_INVALID, "0 positions: 1 to 2^29 - 1")
        H.refused(tables(n_pos=1 << 29, prm=False), E_INVALID, "536870912 positions: 1 to 2^29 - 1")
        walk_call_params(H, tables)
        H.refused(fetch(5), E_STATE, NO_CALLS)                                    # no refused call left any
        H.prm = capi.CallParams(min_depth=1, min_alt=1, min_q=0)
        assert tables() == OK and tot.calls == 1                                  # 30 of 30 molecules show C where the ref is A
        H.refused(fetch(2), E_INVALID, "2 records asked: the last call left 1")
        H.refused(fetch(0), E_INVALID, "0 records asked: the last call left 1")
        H.refused(fetch(1), E_INVALID, "bad arguments: no records array")
        records = np.zeros(1, dtype=capi.CALL_RECORD_DTYPE)
        assert fetch(1, records) == OK and (int(records[0]["pos"]), int(records[0]["allele"])) == (0, 1)
    finally:
        H.close()


def test_locus_tables(lane):
    H = Handle(lane, with_reads=False)
    try:
        lib, h = H.lib, H.h
        counts = np.zeros((N_POS, 5), dtype=np.int32)
        merged = np.zeros((N_POS, 5), dtype=np.int32)

        def tables(h_=h, counts_=counts, columns=5, plan=True, n_pos=N_POS, n_loci=N_POS):
            arr = H.plan_arr if plan is True else plan
            return lib.mipgen_accel_locus_tables(h_, None if counts_ is None else counts_.ctypes.data_as(I32P), columns, None if arr is None else arr.ctypes.data_as(I64P),
                                                 n_pos, n_loci, merged.ctypes.data_as(I32P), None)

        H.refused(tables(h_=None), E_INVALID, NO_HANDLE)
        H.refused(tables(counts_=None, columns=6), E_INVALID, "bad arguments: no counts")
        H.refused(tables(columns=6, plan=None), E_INVALID, "6 columns: 5 (the pileup's table) or 8 (the gapped one)")
        walk_locus_plan(H, tables)
        assert tables() == OK
    finally:
        H.close()


def test_locus_plan_pileup_pool_and_call(H):
    # no plan yet: STATE after the refusals of the row, before the table is compared with the plan
    walk_row_ladder(H, H.locus_pileup, False)
    walk_row_ladder(H, lambda **kw: H.locus_pileup(**{"W": 4, **kw}), True)
    H.refused(H.locus_pileup(mq=41, W=-1), E_INVALID, "min_quality 41: 0 to 40 (the consensus writes 2 to 40)")
    H.refused(H.locus_pileup(W=16), E_INVALID, "max_indel 16: 1 to 15")
    H.refused(H.locus_pileup(W=-1), E_INVALID, "max_indel -1: 1 to 15")
    H.refused(H.locus_pileup(lens=(33, 41)), E_STATE, NO_PLAN)
    H.refused(H.locus_pool(W=16, bg=-1), E_INVALID, "max_indel 16: 1 to 15")
    H.refused(H.locus_pool(bg=-1), E_INVALID, "bg_max_ppm -1: 0 to 1000000")
    H.refused(H.locus_pool(lens=(33, 41)), E_STATE, NO_PLAN)
    H.refused(H.locus_call(row=9, prm=False), E_STATE, NO_PLAN)
    # the plan
    H.refused(H.plan(ref=False, plan=None), E_INVALID, "bad arguments: no ref bytes of the loci")
    walk_locus_plan(H, H.plan)
    H.refused(H.locus_pileup(), E_STATE, NO_PLAN)                                 # no refused plan was installed
    assert H.plan() == OK
    # the pileup and the pool under a plan
    H.refused(H.locus_pileup(W=16, lens=(33, 41)), E_INVALID, "max_indel 16: 1 to 15")
    H.refused(H.locus_pileup(lens=(33, 41)), E_INVALID, "74 template positions: the locus plan was installed for 73")
    H.refused(H.locus_pileup(seq=False, W=4), E_INVALID, NO_SEQ)
    assert H.locus_pileup(seq=False) == OK and H.locus_pileup(W=4) == OK        # without indels no template bases are needed
    walk_row_ladder(H, H.locus_pool, False, rows=False)
    walk_row_ladder(H, lambda **kw: H.locus_pool(**{"W": 4, **kw}), True, rows=False)
    H.refused(H.locus_pool(W=16, bg=-1), E_INVALID, "max_indel 16: 1 to 15")
    H.refused(H.locus_pool(bg=1000001, lens=(33, 41)), E_INVALID, "bg_max_ppm 1000001: 0 to 1000000")
    H.refused(H.locus_pool(lens=(33, 41)), E_INVALID, "74 template positions: the locus plan was installed for 73")
    # a pool call refused for an argument leaves no pool
    H.refused(H.locus_call(row=9, prm=False), E_STATE, NO_LOCUS_POOL)
    H.refused(H.locus_totals(), E_STATE, NO_LOCUS_ROW)
    # the call
    assert H.locus_pool(seq=False) == OK
    H.refused(H.locus_totals(), E_STATE, NO_LOCUS_ROW)
    H.refused(H.locus_call(row=3, prm=False), E_INVALID, "row 3: the session had 3 rows")
    walk_call_params(H, H.locus_call)
    H.prm = capi.CallParams(bg_max_ppm=10)
    H.refused(H.locus_call(), E_STATE, "bg_max_ppm 10: the locus pool was built with 200000")
    H.prm = capi.CallParams()
    H.refused(H.locus_totals(), E_STATE, NO_LOCUS_ROW)
    assert H.locus_call(row=2) == OK and H.locus_totals() == OK
    H.refused(H.totals(), E_STATE, NO_ROW)                                        # the per-probe calls have their own
    # a rebuilt pool has no row called; a second plan drops the pool
    assert H.locus_pool(W=4) == OK
    H.refused(H.locus_totals(), E_STATE, NO_LOCUS_ROW)
    assert H.locus_call() == OK and H.locus_totals() == OK
    H.refused(H.plan(n_loci=0), E_INVALID, "0 loci: 1 to 2^29 - 1")
    assert H.locus_call() == OK                                                   # a refused plan leaves plan and pool
    assert H.plan() == OK
    H.refused(H.locus_call(row=9, prm=False), E_STATE, NO_LOCUS_POOL)
    H.refused(H.locus_totals(), E_STATE, NO_LOCUS_ROW)
    assert H.locus_pool() == OK and H.locus_call() == OK and H.locus_totals() == OK
