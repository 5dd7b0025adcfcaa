"""GPU: the insertion alleles (mipgen_accel_reads_consensus_insertions, mipgen_accel_insertions_fetch, `mipgen_count -pileup_insertions`).  Every
comparison is exact equality of counts, anchors, records and totals against tests/insertion_ref.py - plain loops over the oracle's own path - on the groups the
device itself fetched; `counts` is also the gapped pileup's table of the same arguments, and every call is made twice and returns the same bytes."""
import faulthandler
import json

import numpy as np
import pytest

from mipgen_amd import capi, synth
from tests import consensus_ref as CR
from tests import gapped_ref as G
from tests import helpers as H
from tests import insertion_ref as I
from tests import reads_ref as R
from tests.test_gapped_cpu import plant
from tests.test_gpu_gapped import PAD, variant
from tests.test_gpu_pileup import ARM, COUNT_BIN, TAGS, WG, Lane, _run, cut_probes, session, tag_of, write_fastq_q
from tests.test_gpu_reads import TABLES, _accel, random_tag
from tests.test_gpu_samples import GOLDEN_PLAIN, clean_reads_uneven_depth_inputs, draw_barcodes, plain_session_digest
from tests.test_insertions_cpu import HAND_CELLS, long_run_cell
from tests.test_pileup_cpu import clean_window, synthetic_row
from tests.test_reads_cpu import HEADER

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE = -1, -6


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


@pytest.fixture(scope="module")
def genome():
    return synth.random_genome(40000, 17)


def invariants(counts, anchors, records):
    assert np.array_equal(anchors[:, 1], counts[:, 6]) and np.array_equal(anchors[:, 2], counts[:, 7])
    per_pos, amb_pos = np.zeros(len(anchors), dtype=np.int64), np.zeros(len(anchors), dtype=np.int64)
    amb = records["ambiguous"] == 1
    np.add.at(per_pos, records["pos"], records["count"])
    np.add.at(amb_pos, records["pos"][amb], records["count"][amb])
    assert np.array_equal(per_pos, anchors[:, 1]) and np.array_equal(amb_pos, anchors[:, 3])


def check(acc, groups, mols, row=0, mf=1, mq=0, W=4):
    """One insertions call, twice, against the oracle on `groups` and against the gapped pileup of the same arguments; (counts, anchors, records, totals)."""
    n, lens = len(mols), [len(m) for m in mols]
    counts, anchors, records, totals = acc.consensus_insertions(mols, lens, row, mf, mq, W)
    again = acc.consensus_insertions(mols, lens, row, mf, mq, W)
    assert counts.tobytes() == again[0].tobytes() and anchors.tobytes() == again[1].tobytes() and records.tobytes() == again[2].tobytes() and totals == again[3]
    assert anchors.dtype == np.int32 and anchors.shape == (sum(lens), 4) and records.dtype == capi.INSERTION_RECORD_DTYPE
    w_anchors, w_records, w_totals = I.insertions(groups, mols, n, row, mf, mq, W)
    assert np.array_equal(anchors, w_anchors), (row, mf, mq, W, np.flatnonzero((anchors != w_anchors).any(axis=1))[:5])
    assert records.tobytes() == w_records.tobytes(), (row, mf, mq, W, records[:5], w_records[:5])
    assert totals == w_totals and tuple(totals) == I.TOTAL_KEYS, (row, mf, mq, W, totals, w_totals)
    g_counts, g_totals = acc.consensus_pileup_gapped(mols, lens, row, mf, mq, W)
    assert counts.tobytes() == g_counts.tobytes() and np.array_equal(counts, G.pileup(groups, mols, n, row, mf, mq, W)[0])
    assert all(totals[k] == g_totals[k] for k in ("groups", "used", "insertions", "ins_discordant", "gapped_sides"))
    invariants(counts, anchors, records)
    return counts, anchors, records, totals


def with_insert(M, at, X):
    return M[:at] + X + M[at:]


def quiet_sites(M, lo, hi):
    """The t in [lo, hi) with M[t - 1] and M[t] both A or T: a run of G and C planted in front of M[t] can neither slide nor be split."""
    return [t for t in range(lo, hi) if M[t - 1] in b"AT" and M[t] in b"AT"]


# ---- template lengths, band widths, planted insertions ---------------------------------------------------------------------------------------------------------
def test_lengths_bands_and_planted_insertions(acc, genome):
    """Molecules of 40, 63, 64, 65, 129 and 200 bases under W = 1, 4 and 15.  On each: insertions of 1, 2, 3, 15 and 16 bases in both reads (16 exceeds every W and
    is not placed), one in one read only, one the ligation read is too short to see, one next to N, one beside a deletion, families of 1 and 2; on the molecules
    that have them, insertions at anchors 62, 63 and 64 - the last lanes of the first round of 64 positions and the first of the second."""
    rng = np.random.default_rng(601)
    lengths = [40, 63, 64, 65, 129, 200]
    mols, arms = cut_probes(genome, lengths)
    mols = [M[:60] + b"ATTATAAT" + M[68:] if len(M) > 100 else M for M in mols]                               # (quiet sites around the end of the first round)
    L = Lane(rng)
    for p, M in enumerate(mols):
        n, mid = len(M), len(M) // 2
        for k, size in enumerate((1, 2, 3, 15, 16)):
            Mv = plant(M, "ins", mid, size, rng)
            variant(L, M, Mv, Mv, len(Mv), len(Mv), family=1 + k % 2)
        Mv = plant(M, "ins", ARM + 2, 2, rng)
        variant(L, M, Mv, M, n, n)                                                                             # in the extension read only: discordant where both cover
        variant(L, M, Mv, Mv, len(Mv), ARM + 1)                                                                # the ligation read is too short to see it
        Mv = plant(M, "ins", ARM + 4, 3, rng)
        variant(L, M, Mv[:ARM + 5] + b"N" + Mv[ARM + 6:], Mv, len(Mv), len(Mv), qual=ord("I"))                 # N inside the run of the extension read
        Mv = plant(plant(M, "ins", n - ARM - 2, 2, rng), "del", ARM + 1, 2, rng)
        variant(L, M, Mv, Mv, len(Mv), len(Mv))                                                                # a deletion in front of it
        for a in (62, 63, 64):
            if n > 100:
                Mv = with_insert(M, a + 1, (b"G", b"GC", b"CGG")[a % 3])
                variant(L, M, Mv, Mv, len(Mv), len(Mv), qual=ord("5"))
    got, want = session(acc, arms, L.shuffled())
    assert got == want
    at = np.cumsum([0] + lengths)
    for W in (1, 4, 15):
        for mf, mq in ((1, 0), (2, 21)):
            counts, anchors, records, totals = check(acc, got, mols, 0, mf, mq, W)
        counts, anchors, records, totals = check(acc, got, mols, 0, 1, 0, W)
        assert totals["insertions"] > 0 and totals["span"] > totals["insertions"] and totals["alleles"] > 0
        assert not (records["length"] == 16).any() and ((records["length"] == 15).any() == (W == 15))
        if W >= 3:
            for p in (4, 5):
                assert all(anchors[at[p] + a][1] > 0 for a in (62, 63, 64)), (W, p)
    assert totals["ins_discordant"] > 0 and totals["ambiguous"] > 0


def test_alleles_of_one_anchor(acc, genome):
    """Two alleles of one anchor and length that differ only in the last base; two alleles of one anchor with lengths 1 and 2; their counts."""
    rng = np.random.default_rng(607)
    mols, arms = cut_probes(genome, [80, 70])
    L = Lane(rng)
    M = mols[0]
    a = quiet_sites(M, 30, 50)[0]
    for X, times in ((b"GGC", 3), (b"GGG", 2)):
        for _ in range(times):
            variant(L, M, with_insert(M, a, X), with_insert(M, a, X), len(M) + 3, len(M) + 3, qual=ord("I"))
    M = mols[1]
    b = quiet_sites(M, 30, 50)[0]
    for X, times in ((b"G", 4), (b"GC", 1)):
        for _ in range(times):
            variant(L, M, with_insert(M, b, X), with_insert(M, b, X), len(M) + 2, len(M) + 2, qual=ord("I"))
    got, want = session(acc, arms, L.shuffled())
    counts, anchors, records, totals = check(acc, got, mols, 0, 1, 0, 4)
    assert [tuple(int(v) for v in r) for r in records] == [(a - 1, 3, 3, I.pack(b"GGC"), 0), (a - 1, 3, 2, I.pack(b"GGG"), 0), (80 + b - 1, 1, 4, I.pack(b"G"), 0),
                                                           (80 + b - 1, 2, 1, I.pack(b"GC"), 0)]
    assert tuple(anchors[a - 1]) == (5, 5, 0, 0) and tuple(anchors[80 + b - 1]) == (5, 5, 0, 0) and totals["alleles"] == 4


# ---- the hand-worked cells of the CPU test, planted in reads --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", HAND_CELLS + [long_run_cell()[0]], ids=[c.name for c in HAND_CELLS] + ["a run above 15 bases"])
def test_the_hand_worked_cells_planted_in_reads(acc, cell):
    """One molecule of one probe whose arms are those of the sequence the reads were made from; the template of the call is the cell's."""
    S = cell.S
    arms = [(S[:ARM], S[-ARM:])]
    tag = tag_of(5)
    got = acc.consensus_reads(arms, [tag + cell.ext], [cell.lig], [b"I" * len(tag) + cell.ext_qual], [cell.lig_qual], None, None, 0, TAGS)[4]
    assert len(got) == 1 and got[0][3] == cell.ext and got[0][5] == cell.lig
    counts, anchors, records, totals = check(acc, got, [cell.template], 0, 1, cell.min_quality, cell.W)
    assert tuple(int(v) for v in anchors[cell.anchor]) == cell.row
    assert [tuple(int(v) for v in r) for r in records] == [(t, l, n, 0 if s is None else I.pack(s), int(s is None)) for t, l, n, s in cell.records]


# ---- molecules per cell: both frame kernels emit -----------------------------------------------------------------------------------------------------------------
def test_molecules_per_cell(acc, genome):
    """Cells of 1, 4, 255, 256 and 257 molecules and an empty probe between them; every third molecule carries an insertion, so the one-wavefront kernel and the
    workgroup kernel both count and emit."""
    rng = np.random.default_rng(613)
    sizes = [1, 4, 0, WG - 1, WG, WG + 1]
    mols, arms = cut_probes(genome, [40, 65, 40, 40, 40, 40])
    L = Lane(rng)
    for M, s in zip(mols, sizes):
        for k in range(s):
            if k % 3 == 0:
                Mv = plant(M, "ins", ARM + 1 + k % 5, 1 + k % 3, rng)
                variant(L, M, Mv, Mv if k % 9 else M, len(Mv) - k % 3, len(Mv) - k % 2, family=2 if k % 11 == 0 else 1, qual=ord("#") + (k % 3) * 19)
            else:
                L.molecule(M, len(M) - 3 * (k % 4), len(M) - 2 * (k % 3), qual=ord("#") + (k % 3) * 19)
    got, want = session(acc, arms, L.shuffled(), chunks=3)
    assert got == want and [sum(1 for g in got if g[0] == p) for p in range(len(sizes))] == sizes
    at = np.cumsum([0] + [len(m) for m in mols])
    for mf, mq in ((1, 0), (2, 3)):
        counts, anchors, records, totals = check(acc, got, mols, 0, mf, mq, 4)
    counts, anchors, records, totals = check(acc, got, mols, 0, 1, 0, 4)
    assert not anchors[at[2]:at[3]].any() and totals["groups"] == sum(sizes)
    for p in (1, 3, 4, 5):                                                                                     # (the one molecule of cell 0 shows its insertion on one side only)
        assert anchors[at[p]:at[p + 1], 1].sum() > 0, p


def test_exact_numbers_of_events_in_a_row(acc, genome):
    """Five samples and undetermined with exactly 0, 1, 63, 64, 65 and 300 events: nothing to sort, one key, and a wavefront's worth of slots on either side."""
    rng = np.random.default_rng(617)
    mols, arms = cut_probes(genome, [48, 52])
    barcodes = draw_barcodes(rng, 5, 8)
    events = [0, 1, 63, 64, 65, 300]
    L = Lane(rng)
    sites = [quiet_sites(M, ARM + 1, len(M) - ARM) for M in mols]
    assert all(len(s) >= 2 for s in sites)
    for r, n_events in enumerate(events):
        index = barcodes[r] if r < 5 else b"N" * 8                                                             # (no barcode: undetermined)
        for k in range(n_events):
            M = mols[k % 2]
            Mv = with_insert(M, sites[k % 2][k % len(sites[k % 2])], (b"G", b"GC", b"CG", b"C")[k % 4])
            variant(L, M, Mv, Mv, len(Mv), len(Mv), qual=ord("I"), index=index)
        for k in range(3):
            L.molecule(mols[k % 2], 48, 48, index=index)
    got, want = session(acc, arms, L.shuffled(), barcodes)
    assert got == want
    for r in (5, 0, 3, 1, 2, 4):
        counts, anchors, records, totals = check(acc, got, mols, r, 1, 0, 4)
        assert totals["insertions"] == events[r] and totals["ins_discordant"] == 0 and (totals["alleles"] == 0) == (events[r] == 0)
        assert totals["used"] == events[r] + 3


# ---- rows, and the other calls before and after --------------------------------------------------------------------------------------------------------------------
def test_rows_and_the_other_calls_untouched(genome):
    """Two samples plus undetermined, rows 2, 0, 1, 0.  The gapped pileup, a call and a locus pileup made before the insertions calls return the same bytes after
    them; timing index 15 is set by an insertions call and no other index is."""
    rng = np.random.default_rng(619)
    mols, arms = cut_probes(genome, [90, 129, 64, 75])
    barcodes = draw_barcodes(rng, 2, 8)
    L = Lane(rng)
    for p, M in enumerate(mols):
        for k in range(5 + 2 * p):
            index = barcodes[k % 2] if k % 5 != 4 else random_tag(rng, 8)
            Mv = plant(M, "ins" if k % 2 else "del", ARM + 3 + 2 * k, 1 + k % 3, rng) if k % 4 else M
            variant(L, M, Mv, Mv, 70, 66, family=1 + k % 2, index=index)
    lens = [len(m) for m in mols]
    n_pos = sum(lens)
    a = _accel()
    try:
        got, want = session(a, arms, L.shuffled(), barcodes)
        assert got == want and {g[0] // len(arms) for g in got} == {0, 1, 2}
        params = capi.CallParams(min_depth=1, min_alt=1, min_q=0)
        plan = np.arange(n_pos, dtype=np.int64) * 4
        ref = b"".join(mols)

        def others():
            a.consensus_call_pool(mols, lens, 1, 0, 4)
            a.consensus_locus_plan(plan, ref)
            out = [a.consensus_pileup_gapped(mols, lens, r, 1, 0, 4) for r in range(3)] + [a.consensus_call(0, params), a.consensus_locus_pileup(mols, lens, 1, 1, 0, 4)]
            return [[x.tobytes() if isinstance(x, np.ndarray) else x for x in o] for o in out]

        before = others()
        results = {}
        for r in (2, 0, 1, 0):
            res = check(a, got, mols, r, 1, 0, 4)
            if r in results:
                assert all(x.tobytes() == y.tobytes() for x, y in zip(res[:3], results[r][:3])) and res[3] == results[r][3]
            results[r] = res
        assert sum(results[r][3]["groups"] for r in range(3)) == len(got) and sum(results[r][3]["insertions"] for r in range(3)) > 0
        assert others() == before
        # timing
        a.set_timing(True)
        assert a.last_kernel_ms(15) < 0
        a.consensus_pileup_gapped(mols, lens, 0, 1, 0, 4)
        assert a.last_kernel_ms(12) > 0 and a.last_kernel_ms(15) < 0
        seen = [a.last_kernel_ms(k) for k in range(4, 15)]
        a.consensus_insertions(mols, lens, 0, 1, 0, 4)
        assert a.last_kernel_ms(15) > 0 and [a.last_kernel_ms(k) for k in range(4, 15)] == seen
        a.set_timing(False)
    finally:
        a.close()


# ---- state, refusals, the untouched handle -----------------------------------------------------------------------------------------------------------------------
def test_state_refusals_and_a_plain_session_afterwards(genome):
    rng = np.random.default_rng(631)
    mols, arms = cut_probes(genome, [90, 64])
    L = Lane(rng)
    for M in mols:
        for k in range(3):
            Mv = plant(M, "ins", 30 + k, 1 + k, rng)
            variant(L, M, Mv, Mv, 70 + k, 66 + k)
    ext, lig, eq, lq, idx = L.shuffled()
    n, lens = len(arms), np.array([len(m) for m in mols], dtype=np.int32)
    seq = b"".join(mols)
    a = _accel()
    try:
        lib, h = a.lib, a.h
        i32p = capi.C.POINTER(capi.C.c_int32)
        counts = np.full((int(lens.sum()), 8), -7, dtype=np.int32)
        anchors = np.full((int(lens.sum()), 4), -7, dtype=np.int32)
        tot = capi.InsertionTotals()

        def call(seq_=seq, lens_=lens, n_=n, row=0, mf=1, mq=0, W=4, out=counts, anc=anchors, tot_=tot):
            return lib.mipgen_accel_reads_consensus_insertions(h, seq_, lens_.ctypes.data_as(i32p) if lens_ is not None else None, n_, row, mf, mq, W,
                                                               out.ctypes.data_as(i32p) if out is not None else None,
                                                               anc.ctypes.data_as(i32p) if anc is not None else None, capi.C.byref(tot_) if tot_ is not None else None)

        def fetch(k):
            rec = np.zeros(max(k, 1), dtype=capi.INSERTION_RECORD_DTYPE)
            return lib.mipgen_accel_insertions_fetch(h, rec.ctypes.data, k), rec[:max(k, 0)]

        assert call() == E_STATE and b"holds no consensus reads" in lib.mipgen_accel_last_error()
        assert fetch(0)[0] == E_STATE
        arr = capi.probe_array(arms)
        assert lib.mipgen_accel_reads_open_consensus(h, arr, n, 8, 0, 0, None, 0, 0, 0) == 0
        assert call() == E_STATE and fetch(0)[0] == E_STATE                                                     # before the finish
        assert lib.mipgen_accel_reads_finish_consensus(h, None, None, None, None, None, None) == 0
        assert fetch(0)[0] == E_STATE and b"no insertion alleles" in lib.mipgen_accel_last_error()               # reads, but no call yet
        assert call() == 0 and not counts.any() and not anchors.any() and all(getattr(tot, k) == 0 for k in I.TOTAL_KEYS)      # zero groups give zeros
        assert fetch(0)[0] == 0 and fetch(1)[0] == E_INVALID
        got = a.consensus_reads(arms, ext, lig, eq, lq, tag_sizes=TAGS)[4]
        assert fetch(0)[0] == E_STATE                                                                           # new reads: the records went with the old ones
        counts[:] = -7; anchors[:] = -7
        bad, long_ = lens.copy(), lens.copy()
        bad[1] = 0; long_[0] = 2049
        for kw in ({"seq_": None}, {"lens_": None}, {"n_": n - 1}, {"n_": n + 1}, {"lens_": bad}, {"lens_": long_}, {"row": -1}, {"row": 1}, {"mf": 0}, {"mq": -1},
                   {"mq": 41}, {"W": 0}, {"W": 16}, {"W": -1}):
            assert call(**kw) == E_INVALID, kw
        assert call(W=16) == E_INVALID and b"max_indel 16" in lib.mipgen_accel_last_error()
        assert (counts == -7).all() and (anchors == -7).all() and fetch(0)[0] == E_STATE
        w_anchors, w_records, w_totals = I.insertions(got, mols, n, 0, W=4)
        n_rec = w_totals["alleles"]
        assert n_rec >= 6
        assert call() == 0 and np.array_equal(anchors, w_anchors) and np.array_equal(counts, G.pileup(got, mols, n, 0, W=4)[0])
        assert {k: getattr(tot, k) for k in I.TOTAL_KEYS} == w_totals
        for k in (0, n_rec - 1, n_rec + 1, -1):
            assert fetch(k)[0] == E_INVALID, k
        assert b"left %d" % n_rec in lib.mipgen_accel_last_error()
        assert lib.mipgen_accel_insertions_fetch(h, None, n_rec) == E_INVALID
        rc, rec = fetch(n_rec)
        assert rc == 0 and rec.tobytes() == w_records.tobytes()
        assert call(out=None, anc=None) == 0 and tot.alleles == n_rec and call(tot_=None) == 0 and np.array_equal(anchors, w_anchors)
        assert call(row=1) == E_INVALID and fetch(n_rec)[0] == 0                                                    # a refused call leaves the records of the last one
        # the next open drops the reads
        assert lib.mipgen_accel_reads_open(h, arr, n, 8, 0, 0) == 0
        assert call() == E_STATE and fetch(n_rec)[0] == E_STATE
        assert lib.mipgen_accel_reads_finish(h, None, None, None) == 0
        assert call() == E_STATE
        # a plain session afterwards is the recorded one
        name, key = TABLES[0]
        t_rows, t_ext, t_lig = clean_reads_uneven_depth_inputs(name, key)
        plain = a.count_reads([(r[6], r[10]) for r in t_rows], t_ext, t_lig, want_assignment=True)
        assert plain_session_digest(*plain) == json.load(open(GOLDEN_PLAIN))[f"{name}/{key}"]["sha256"]
    finally:
        a.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_barcodes", [False, True])
def test_cli_equals_the_oracle(tmp_path, with_barcodes):
    """A small table on both strands and FASTQ with planted insertions: the -pileup_insertions file byte for byte and the new last stderr line; the -pileup file,
    the -call file and every other stderr line are those of the run without the option."""
    g = H.golden_genome()
    rng = np.random.default_rng(641 + with_barcodes)
    t_rows, at = [], 5000
    for k in range(6):
        first = clean_window(g, at, 140)
        length = (130, 121, 140, 64)[k % 4]
        t_rows.append(synthetic_row(g, first, first + length - 1, b"+" if k % 3 else b"-", arm=20 + k % 3))
        at = first + 400
    with open(tmp_path / "table.txt", "wb") as fh:
        fh.write(HEADER.encode() + b"".join(b"\t".join(r) + b"\n" for r in t_rows))
    mols = [r[6] + r[13] + r[10] for r in t_rows]
    arms = [(r[6], r[10]) for r in t_rows]
    barcodes = draw_barcodes(rng, 3, 8)
    labels = ["sample_a", "sample_b", "sample_c"]
    ext, lig, eq, lq, idx = [], [], [], [], []
    for p, M in enumerate(mols):
        for k in range(4 + 3 * (p % 3)):
            tag = random_tag(rng, 8)
            Mv = M
            if k % 3 == 1:
                Mv = plant(M, "del", int(rng.integers(26, len(M) - 30)), 1 + k % 4, rng)
            elif k % 3 == 2 or k == 0:
                Mv = with_insert(M, 30 + p, (b"GAT", b"GAC", b"T")[k % 3])                                       # the same anchor, three alleles
            Mv = bytearray(Mv)
            if k % 2:
                t = int(rng.integers(24, len(Mv) - 24))
                Mv[t] = b"ACGT"[(b"ACGT".index(Mv[t]) + 1 + k % 3) & 3]
            index = barcodes[int(rng.integers(0, 2))] if rng.random() < 0.85 else random_tag(rng, 8)
            for m in range(1 + (k + p) % 3):
                e = tag[:5] + (bytes(Mv) + PAD)[:95]
                l = tag[5:] + (R.revcomp(bytes(Mv)) + PAD)[:97]
                ext.append(e); lig.append(l); idx.append(index)
                eq.append(rng.integers(35, 75, len(e)).astype(np.uint8).tobytes()); lq.append(rng.integers(35, 75, len(l)).astype(np.uint8).tobytes())
    write_fastq_q(tmp_path / "ext.fq", ext, eq); write_fastq_q(tmp_path / "lig.fq", lig, lq)
    write_fastq_q(tmp_path / "i1.fq", idx, [b"I" * 8] * len(idx))
    with open(tmp_path / "samples.tsv", "wb") as fh:
        fh.write(b"\n".join(l.encode() + b"\t" + b for l, b in zip(labels, barcodes)) + b"\n")
    common = [COUNT_BIN, "-tag_sizes", "5,3", "-reads", "ext.fq", "lig.fq", "table.txt", "-o", "counts.tsv"] + (
        ["-barcodes", "samples.tsv", "-index_reads", "i1.fq"] if with_barcodes else [])
    want = CR.consensus_reads(arms, ext, lig, eq, lq, idx if with_barcodes else None, barcodes if with_barcodes else None, 0, (5, 3))
    assert want[2]["assigned"] == len(ext)
    lab = labels if with_barcodes else None
    for extra, W, mf, mq in (([], 4, 1, 0), (["-pileup_min_family", "2", "-pileup_min_quality", "30"], 2, 2, 30)):
        gapped = ["-pileup_indels", str(W)] + extra
        base = _run(common + ["-pileup", "pile0.tsv"] + gapped, str(tmp_path))
        assert base.returncode == 0, base.stderr.decode()
        text, line = I.insertions_file(want[4], t_rows, lab, mf, mq, W)
        assert text.count(b"\n") > 3 and b"\t-\t" in text and b"\t+\t" in text
        p = _run(common + ["-pileup", "pile.tsv"] + gapped + ["-pileup_insertions", "ins.tsv"], str(tmp_path))
        assert p.returncode == 0, p.stderr.decode()
        assert open(tmp_path / "ins.tsv", "rb").read() == text
        assert p.stderr.decode() == base.stderr.decode() + line
        assert open(tmp_path / "pile.tsv", "rb").read() == open(tmp_path / "pile0.tsv", "rb").read() == G.pileup_file(want[4], t_rows, lab, mf, mq, W)[0]
        # with -call beside it: the call route runs unchanged and the insertions call feeds INS only
        base = _run(common + ["-pileup", "pile0.tsv", "-call", "calls0.tsv"] + gapped, str(tmp_path))
        assert base.returncode == 0, base.stderr.decode()
        p = _run(common + ["-pileup", "pile.tsv", "-call", "calls.tsv"] + gapped + ["-pileup_insertions", "ins2.tsv"], str(tmp_path))
        assert p.returncode == 0, p.stderr.decode()
        assert open(tmp_path / "ins2.tsv", "rb").read() == text and p.stderr.decode() == base.stderr.decode() + line
        assert open(tmp_path / "pile.tsv", "rb").read() == open(tmp_path / "pile0.tsv", "rb").read()
        assert open(tmp_path / "calls.tsv", "rb").read() == open(tmp_path / "calls0.tsv", "rb").read()
