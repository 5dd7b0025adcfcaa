"""GPU: the deletion alleles (mipgen_accel_reads_consensus_deletions, mipgen_accel_deletions_fetch, `mipgen_count -pileup_deletions`).  Every comparison
is exact equality of counts, sites, records and totals against tests/deletion_ref.py - plain loops over the voted classes of every molecule - on the groups the
device itself fetched; `counts` is also the gapped pileup's table of the same arguments, every call is made twice and returns the same bytes, and the six invariants
hold on every call."""
import faulthandler
import json

import numpy as np
import pytest

from mipgen_amd import capi, synth
from tests import consensus_ref as CR
from tests import deletion_ref as D
from tests import gapped_cases as GC
from tests import gapped_ref as G
from tests import helpers as H
from tests import insertion_ref as I
from tests import reads_ref as R
from tests.test_deletions_cpu import END_EXTRA, HAND_CELLS, cut
from tests.test_gapped_cpu import plant
from tests.test_gpu_gapped import PAD, variant
from tests.test_gpu_gapped_shapes import add_pairs
from tests.test_gpu_pileup import ARM, COUNT_BIN, TAGS, WG, Lane, _run, cut_probes, session, tag_of, write_fastq_q
from tests.test_gpu_reads import TABLES, _accel, random_tag
from tests.test_gpu_samples import GOLDEN_PLAIN, clean_reads_uneven_depth_inputs, draw_barcodes, plain_session_digest
from tests.test_insertions_cpu import M as HAND_M
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


def raw_deletions(acc, mols, row, mf, mq, W):
    """The call with the template bytes as they are (capi.Accel.consensus_deletions upper-cases them): (counts, sites, records, totals)."""
    lens = np.array([len(m) for m in mols], dtype=np.int32)
    counts = np.full((int(lens.sum()), 8), -7, dtype=np.int32)
    sites = np.full((int(lens.sum()), 4), -7, dtype=np.int32)
    tot = capi.DeletionTotals()
    i32p = capi.C.POINTER(capi.C.c_int32)
    rc = acc.lib.mipgen_accel_reads_consensus_deletions(acc.h, b"".join(mols), lens.ctypes.data_as(i32p), len(mols), row, mf, mq, W, counts.ctypes.data_as(i32p),
                                                        sites.ctypes.data_as(i32p), capi.C.byref(tot))
    assert rc == 0, acc.lib.mipgen_accel_last_error()
    return counts, sites, acc.deletions_fetch(int(tot.alleles)), {k: int(getattr(tot, k)) for k in D.TOTAL_KEYS}


def check(acc, groups, mols, row=0, mf=1, mq=0, W=4, per_molecule=None):
    """One deletions call, twice, against the oracle on `groups` and against the gapped pileup of the same arguments; (counts, sites, records, totals)."""
    n, lens = len(mols), [len(m) for m in mols]
    counts, sites, records, totals = raw_deletions(acc, mols, row, mf, mq, W)
    again = raw_deletions(acc, mols, row, mf, mq, W)
    assert counts.tobytes() == again[0].tobytes() and sites.tobytes() == again[1].tobytes() and records.tobytes() == again[2].tobytes() and totals == again[3]
    assert sites.dtype == np.int32 and sites.shape == (sum(lens), 4) and records.dtype == capi.DELETION_RECORD_DTYPE
    w_sites, w_records, w_totals = D.deletions(groups, mols, n, row, mf, mq, W, per_molecule)
    assert np.array_equal(sites, w_sites), (row, mf, mq, W, np.flatnonzero((sites != w_sites).any(axis=1))[:5])
    assert records.tobytes() == w_records.tobytes(), (row, mf, mq, W, records[:5], w_records[:5])
    assert totals == w_totals and tuple(totals) == D.TOTAL_KEYS, (row, mf, mq, W, totals, w_totals)
    g_counts, g_totals = acc.consensus_pileup_gapped(mols, lens, row, mf, mq, W) if all(m == m.upper() for m in mols) else (counts, None)
    w_counts, wg_totals = G.pileup(groups, mols, n, row, mf, mq, W)
    assert counts.tobytes() == g_counts.tobytes() and np.array_equal(counts, w_counts)
    assert g_totals is None or g_totals == wg_totals
    D.check_invariants(counts, sites, records, totals, wg_totals)
    return counts, sites, records, totals


def alleles(records):
    return [(int(r["pos"]), int(r["length"]), int(r["ragged"]), int(r["count"])) for r in records]


def free_of(S, a, l):
    """l bases for a template to hold in front of S[a] that the reads made from S lack, so that their deletion has one placement: no base of them equals S[a - 1]
    (the run can neither slide to the left nor be split there) or S[a]."""
    pool = [b for b in b"ACGT" if b not in (S[a - 1] if a else 0, S[a] if a < len(S) else 0)]
    return bytes(pool[j % 2] for j in range(l))


# ---- template lengths, band widths, planted deletions -----------------------------------------------------------------------------------------------------------
def test_lengths_bands_and_planted_deletions(acc, genome):
    """Molecules of 40, 63, 64, 65, 129 and 200 bases under W = 1, 4 and 15.  On each: deletions of 1, 2, 3, 15 and 16 bases in both reads (16 exceeds every W), one
    in one read only (discordant, no event), one the ligation read is too short to see, one with N beside it, one beside an insertion, one read that lacks 3 bases
    against one that lacks 2 of them (ragged), families of 1 and 2."""
    rng = np.random.default_rng(701)
    lengths = [40, 63, 64, 65, 129, 200]
    mols, arms = cut_probes(genome, lengths)
    L = Lane(rng)
    for p, M in enumerate(mols):
        n, mid = len(M), len(M) // 2
        for k, size in enumerate((1, 2, 3, 15, 16)):
            if n - 2 * ARM > size + 2:
                Mv = plant(M, "del", min(mid, n - ARM - size - 1), size, rng)
                variant(L, M, Mv, Mv, len(Mv), len(Mv), family=1 + k % 2)
        Mv = plant(M, "del", ARM + 2, 2, rng)
        variant(L, M, Mv, M, n, n)                                                                             # in the extension read only
        variant(L, M, Mv, Mv, len(Mv), ARM + 1)                                                                # the ligation read is too short to see it
        variant(L, M, Mv[:ARM + 2] + b"N" + Mv[ARM + 3:], Mv, len(Mv), len(Mv), qual=ord("I"))                 # N behind the run in the extension read
        variant(L, M, plant(M, "del", ARM + 1, 3, rng), plant(M, "del", ARM + 1, 2, rng), n, n)                # ragged on the right, or whatever the repeat makes of it
        variant(L, M, plant(M, "del", ARM + 1, 3, rng), plant(M, "del", ARM + 2, 2, rng), n, n, qual=ord("5"))  # ragged on the left
        Mv = plant(plant(M, "ins", n - ARM - 2, 2, rng), "del", ARM + 1, 2, rng)
        variant(L, M, Mv, Mv, len(Mv), len(Mv))                                                                # an insertion behind it
    got, want = session(acc, arms, L.shuffled())
    assert got == want
    for W in (1, 4, 15):
        for mf, mq in ((1, 0), (2, 21)):
            check(acc, got, mols, 0, mf, mq, W)
        counts, sites, records, totals = check(acc, got, mols, 0, 1, 0, W)
        assert totals["events"] > 0 and totals["depth"] > totals["deleted_bases"] >= totals["events"] and totals["alleles"] > 0
        assert W < 4 or records["length"].max() >= 3                                                               # (under a linear gap score a long deletion breaks up at chance matches)
    assert totals["ragged"] > 0 and (counts[:, 4] > 0).any()


# ---- runs around the boundary of a round, at both ends of the template, across two rounds: free templates ---------------------------------------------------------------
def test_runs_where_the_rounds_meet(acc, genome):
    """The call takes its templates from the caller: exact reads of both sides, and a template that holds l more bases in front of position a, show one clean run
    [a, a + l) per molecule.  a = 62, 63, 64, 65 with l = 1, 2, 3, 15: the last lanes of the first round, lane 0 of the second with its extra observation of t = 63,
    and the continuation past lane 63.  A run across t = 128 of a 200-base template; runs at t = 0 and runs that end at L - 1 for L = 63, 64, 65 and 70, the tail
    being the last lane before the clamped ones."""
    rng = np.random.default_rng(709)
    sources, arms = cut_probes(genome, [185, 185, 185, 185, 60, 60])
    L = Lane(rng)
    for S in sources:
        add_pairs(L, S, G.revcomp(S), family=2, qual=ord("I"))
        add_pairs(L, S, G.revcomp(S)[:ARM + 3])                                                                # one side only
        add_pairs(L, S[:ARM + 3], G.revcomp(S))
    got, want = session(acc, arms, L.shuffled())
    assert got == want
    at = lambda mols: np.cumsum([0] + [len(m) for m in mols])
    for l in (1, 2, 3, 15):
        mols = [S[:a] + free_of(S, a, l) + S[a:] for S, a in zip(sources, (62, 63, 64, 65))] + list(sources[4:])
        for W in (15, 4):
            counts, sites, records, totals = check(acc, got, mols, 0, 1, 0, W)
            if l <= W:
                assert alleles(records) == [(at(mols)[p] + a, l, 0, 3) for p, a in enumerate((62, 63, 64, 65))], (l, W)
    # across t = 128: a run of 15 from 120, and one of 9 that ends at 127, the last lane of the second round
    mols = [sources[0][:120] + free_of(sources[0], 120, 15) + sources[0][120:], sources[1][:119] + free_of(sources[1], 119, 9) + sources[1][119:]] + list(sources[2:])
    counts, sites, records, totals = check(acc, got, mols, 0, 1, 0, 15)
    assert alleles(records) == [(120, 15, 0, 3), (200 + 119, 9, 0, 3)]
    # both ends, the tail being the last lane before the clamped ones: templates of 63, 64, 65 and 70 bases that hold l = 3, 4, 5, 10 more bases in front of the
    # first base of the 60-base reads (the extension reads, anchored at t = 0, delete them; the ligation reads end before them) or behind their last
    for total in (63, 64, 65, 70):
        l = total - 60
        S4, S5 = sources[4], sources[5]
        mols = list(sources[:4]) + [free_of(S4, 0, l) + S4, S5 + free_of(S5, 60, l)]
        counts, sites, records, totals = check(acc, got, mols, 0, 1, 0, 15)
        found = {(x, n, r): c for x, n, r, c in alleles(records)}
        assert found.get((at(mols)[4], l, 0), 0) >= 2 and found.get((at(mols)[5] + 60, l, 0), 0) >= 2, (total, found)


# ---- the hand-worked cells of the CPU test, planted in reads ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", HAND_CELLS, ids=[c.name for c in HAND_CELLS])
def test_the_hand_worked_cells_planted_in_reads(acc, cell):
    """One molecule of one probe whose arms are those of the sequence the reads were made from: the ragged cells on either flank, the deletion in one read only, the
    low-quality base inside the other side's run, two runs one base apart, the homopolymer."""
    S = cell.S
    arms = [(S[:ARM], S[-ARM:])]
    tag = tag_of(5)
    got = acc.consensus_reads(arms, [tag + cell.ext], [cell.lig], [b"I" * len(tag) + cell.ext_qual], [cell.lig_qual], None, None, 0, TAGS)[4]
    assert len(got) == 1 and got[0][3] == cell.ext and got[0][5] == cell.lig
    counts, sites, records, totals = check(acc, got, [cell.template], 0, 1, cell.min_quality, cell.W)
    assert alleles(records) == [(a, l, int(rag), 1) for a, l, rag in cell.events]
    assert tuple(np.flatnonzero(counts[:, 4])) == cell.discordant


@pytest.mark.parametrize("extra", [1, 2, 3])
def test_runs_at_both_ends_of_the_hand_template(acc, extra):
    tag = tag_of(6)
    lig = G.revcomp(HAND_M)
    got = acc.consensus_reads([(HAND_M[:ARM], HAND_M[-ARM:])], [tag + HAND_M], [lig], [b"I" * (len(tag) + len(HAND_M))], [b"I" * len(lig)], None, None, 0, TAGS)[4]
    for template, want in ((END_EXTRA[0][:extra] + HAND_M, (0, extra, 0, 1)), (HAND_M + END_EXTRA[1][:extra], (len(HAND_M), extra, 0, 1))):
        counts, sites, records, totals = check(acc, got, [template], 0, 1, 0, 4)
        assert alleles(records) == [want]


def ragged_pair(M, a, left):
    """(extension sequence, ligation sequence) of a molecule whose extension read lacks M[a : a + 3] and whose ligation read lacks two of the three: the first two
    (ragged on the right, the flank at a + 2) or the last two (ragged on the left, the flank at a)."""
    return cut(a, 3, M), cut(a + 1, 2, M) if left else cut(a, 2, M)


def test_ragged_flanks_on_lane_63_and_on_lane_0(acc, genome):
    """Templates of 130 bases with a hand-made stretch around t = 64 in which every deletion below has one placement.  Right flanks at 63 and at 64 (runs 61..62 and
    62..63: the flank of the latter is the first position of the next round, read from the direct observation); left flanks at 63 and at 64 (runs that start at 64 - lane
    0, its neighbour observed by the lane itself - and at 65)."""
    rng = np.random.default_rng(719)
    mols, arms = cut_probes(genome, [130] * 4)
    mols = [M[:56] + b"ACGTACGTACGTACGTA" + M[73:] for M in mols]                                              # (any four bases in a row differ: a run of up to 3 cannot slide)
    arms = [(M[:ARM], M[-ARM:]) for M in mols]
    L = Lane(rng)
    plan = ((61, False), (62, False), (63, True), (64, True))                                                  # (a, left): flank 63, 64, 63, 64
    for M, (a, left) in zip(mols, plan):
        e, l = ragged_pair(M, a, left)
        for _ in range(2):
            variant(L, M, e, l, len(M), len(M), qual=ord("I"))
        variant(L, M, l, e, len(M), len(M), qual=ord("I"))                                                     # the sides swapped
        variant(L, M, e, e, len(M), len(M), qual=ord("I"))                                                     # the clean run of 3 at the same start
    got, want = session(acc, arms, L.shuffled())
    assert got == want
    for W in (4, 15):
        counts, sites, records, totals = check(acc, got, mols, 0, 1, 0, W)
        want_alleles = []
        for p, (a, left) in enumerate(plan):
            x = 130 * p + a
            want_alleles += [(x, 3, 0, 1), (x + 1, 2, 1, 3)] if left else [(x, 2, 1, 3), (x, 3, 0, 1)]
        assert alleles(records) == want_alleles, (alleles(records), want_alleles)
        assert totals["ragged"] == 12 and totals["events"] == 16


# ---- the generator's sessions -------------------------------------------------------------------------------------------------------------------------------------
SESSION_SEEDS = (1049,)                                             # picked on the CPU: the oracle shows the four kinds of event below
SESSION_LENGTHS = (65, 96, 97, 130, 130, 200, 200, 200) * 12


@pytest.mark.parametrize("seed", SESSION_SEEDS)
def test_random_edits_on_low_complexity_templates(acc, seed):
    """96 probes of 65 to 200 bases, 8 to 12 molecules each, reads with up to four indels of 1 to 16 bases, substitutions and N, under W = 1, 4, 15.  From the oracle
    alone, over the three band widths at (min_family, min_quality) = (1, 0): the session holds at least 10 events each that are longer than W, that cross a multiple of 64, that are ragged, and that share their
    molecule with another event."""
    probes = GC.probes(seed, SESSION_LENGTHS)
    L = Lane(np.random.default_rng(727))
    for p in probes:
        for e, l, family in p.molecules:
            add_pairs(L, e, l, family)
    mols = [p.M for p in probes]
    got, want = session(acc, [p.arms for p in probes], L.shuffled())
    assert got == want
    longer = crossing = ragged = shared = 0
    for W in (1, 4, 15):
        per_molecule = []
        check(acc, got, mols, 0, 1, 0, W, per_molecule)
        for _p, _L, ev in per_molecule:
            longer += sum(l > W for _a, l, _r in ev); crossing += sum(a // 64 != (a + l - 1) // 64 for a, l, _r in ev)
            ragged += sum(r for _a, _l, r in ev); shared += len(ev) if len(ev) >= 2 else 0
    check(acc, got, mols, 0, 2, 20, 4)
    assert min(longer, crossing, ragged, shared) >= 10, (longer, crossing, ragged, shared)


# ---- molecules per cell: both frame kernels emit ---------------------------------------------------------------------------------------------------------------------
def test_molecules_per_cell(acc, genome):
    """Cells of 1, 4, 255, 256 and 257 molecules and an empty probe between them; every third molecule carries a deletion, so the one-wavefront kernel and the
    workgroup kernel both count and emit.  The cell of 257 has a template of 100 bases and deletions that start at 62, 63 and 64 and cross into the second round."""
    rng = np.random.default_rng(733)
    sizes = [1, 4, 0, WG - 1, WG, WG + 1]
    mols, arms = cut_probes(genome, [40, 65, 40, 40, 40, 100])
    L = Lane(rng)
    for p, (M, s) in enumerate(zip(mols, sizes)):
        for k in range(s):
            if k % 3 == 0:
                at = 62 + k % 3 + (k // 3) % 3 if p == 5 else ARM + 1 + k % 5
                Mv = plant(M, "del", at, 1 + (k // 9) % 3, rng)
                variant(L, M, Mv, Mv if k % 9 else M, len(Mv) - k % 3, len(Mv) - k % 2, family=2 if k % 11 == 0 else 1, qual=ord("#") + (k % 3) * 19)
            else:
                L.molecule(M, len(M) - 3 * (k % 4), len(M) - 2 * (k % 3), qual=ord("#") + (k % 3) * 19)
    got, want = session(acc, arms, L.shuffled(), chunks=3)
    assert got == want and [sum(1 for g in got if g[0] == p) for p in range(len(sizes))] == sizes
    at = np.cumsum([0] + [len(m) for m in mols])
    for mf, mq in ((1, 0), (2, 3)):
        check(acc, got, mols, 0, mf, mq, 4)
    counts, sites, records, totals = check(acc, got, mols, 0, 1, 0, 4)
    assert not sites[at[2]:at[3]].any() and totals["groups"] == sum(sizes)
    for p in (1, 3, 4, 5):
        assert sites[at[p]:at[p + 1], 1].sum() > 0, p
    in_big = records[records["pos"] >= at[5]]
    assert ((in_big["pos"] - at[5] < 64) & (in_big["pos"] - at[5] + in_big["length"] > 64)).any() and (in_big["pos"] - at[5] == 64).any()


def quiet_starts(M, lo, hi):
    """The a in [lo, hi) at which a deletion of M[a] or of M[a : a + 2] has one placement."""
    return [a for a in range(lo, hi) if M[a - 1] != M[a] and M[a] != M[a + 1] and M[a - 1] != M[a + 1] and M[a] != M[a + 2]]


def test_exact_numbers_of_events_in_a_row(acc, genome):
    """Five samples and undetermined with exactly 0, 1, 63, 64, 65 and 300 events: nothing to sort, one key, and a wavefront's worth of slots on either side."""
    rng = np.random.default_rng(739)
    mols, arms = cut_probes(genome, [48, 52])
    barcodes = draw_barcodes(rng, 5, 8)
    events = [0, 1, 63, 64, 65, 300]
    L = Lane(rng)
    starts = [quiet_starts(M, ARM + 1, len(M) - ARM - 2) for M in mols]
    assert all(len(s) >= 2 for s in starts)
    for r, n_events in enumerate(events):
        index = barcodes[r] if r < 5 else b"N" * 8                                                             # (no barcode: undetermined)
        for k in range(n_events):
            M = mols[k % 2]
            Mv = cut(starts[k % 2][k % len(starts[k % 2])], 1 + k % 2, M)
            variant(L, M, Mv, Mv, len(Mv), len(Mv), qual=ord("I"), index=index)
        for k in range(3):
            L.molecule(mols[k % 2], 48, 48, index=index)
    got, want = session(acc, arms, L.shuffled(), barcodes)
    assert got == want
    for r in (5, 0, 3, 1, 2, 4):
        counts, sites, records, totals = check(acc, got, mols, r, 1, 0, 4)
        assert totals["events"] == events[r] and totals["ragged"] == 0 and (totals["alleles"] == 0) == (events[r] == 0)
        assert totals["used"] == events[r] + 3


# ---- rows, and the other calls before and after --------------------------------------------------------------------------------------------------------------------
def test_rows_and_the_other_calls_untouched(genome):
    """Two samples plus undetermined, rows 2, 0, 1, 0.  The gapped pileup, an insertions call, a call and a locus pileup made before the deletions calls return the
    same bytes after them, and the insertions records are still fetched; timing index 19 is set by a deletions call and no other index is."""
    rng = np.random.default_rng(743)
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
            out = [a.consensus_pileup_gapped(mols, lens, r, 1, 0, 4) for r in range(3)] + [a.consensus_call(0, params), a.consensus_locus_pileup(mols, lens, 1, 1, 0, 4),
                                                                                          a.consensus_insertions(mols, lens, 1, 1, 0, 4)]
            return [[x.tobytes() if isinstance(x, np.ndarray) else x for x in o] for o in out]

        before = others()
        n_ins = len(a.consensus_insertions(mols, lens, 0, 1, 0, 4)[2])
        ins_records = a.insertions_fetch(n_ins).tobytes()
        results = {}
        for r in (2, 0, 1, 0):
            res = check(a, got, mols, r, 1, 0, 4)
            if r in results:
                assert all(x.tobytes() == y.tobytes() for x, y in zip(res[:3], results[r][:3])) and res[3] == results[r][3]
            results[r] = res
            assert a.insertions_fetch(n_ins).tobytes() == ins_records                                            # the insertions records stay where they are
        assert sum(results[r][3]["groups"] for r in range(3)) == len(got) and sum(results[r][3]["events"] for r in range(3)) > 0
        n_del = results[0][3]["alleles"]
        assert others() == before
        assert a.deletions_fetch(n_del).tobytes() == results[0][2].tobytes()                                   # ... and so do the deletion records
        # timing
        a.set_timing(True)
        assert a.last_kernel_ms(19) < 0
        a.consensus_pileup_gapped(mols, lens, 0, 1, 0, 4)
        a.consensus_insertions(mols, lens, 0, 1, 0, 4)
        assert a.last_kernel_ms(12) > 0 and a.last_kernel_ms(15) > 0 and a.last_kernel_ms(19) < 0
        seen = [a.last_kernel_ms(k) for k in range(4, 19)]
        a.consensus_deletions(mols, lens, 0, 1, 0, 4)
        assert a.last_kernel_ms(19) > 0 and [a.last_kernel_ms(k) for k in range(4, 19)] == seen
        a.set_timing(False)
    finally:
        a.close()


# ---- state, refusals, the untouched handle -----------------------------------------------------------------------------------------------------------------------
def test_state_refusals_and_a_plain_session_afterwards(genome):
    rng = np.random.default_rng(751)
    mols, arms = cut_probes(genome, [90, 64])
    L = Lane(rng)
    for M in mols:
        for k in range(3):
            Mv = plant(M, "del", 30 + 3 * k, 1 + k, rng)
            variant(L, M, Mv, Mv, 70 + k, 66 + k)
    ext, lig, eq, lq, idx = L.shuffled()
    n, lens = len(arms), np.array([len(m) for m in mols], dtype=np.int32)
    seq = b"".join(mols)
    a = _accel()
    try:
        lib, h = a.lib, a.h
        i32p = capi.C.POINTER(capi.C.c_int32)
        counts = np.full((int(lens.sum()), 8), -7, dtype=np.int32)
        sites = np.full((int(lens.sum()), 4), -7, dtype=np.int32)
        tot = capi.DeletionTotals()

        def call(seq_=seq, lens_=lens, n_=n, row=0, mf=1, mq=0, W=4, out=counts, sit=sites, tot_=tot):
            return lib.mipgen_accel_reads_consensus_deletions(h, seq_, lens_.ctypes.data_as(i32p) if lens_ is not None else None, n_, row, mf, mq, W,
                                                              out.ctypes.data_as(i32p) if out is not None else None,
                                                              sit.ctypes.data_as(i32p) if sit is not None else None, capi.C.byref(tot_) if tot_ is not None else None)

        def fetch(k):
            rec = np.zeros(max(k, 1), dtype=capi.DELETION_RECORD_DTYPE)
            return lib.mipgen_accel_deletions_fetch(h, rec.ctypes.data, k), rec[:max(k, 0)]

        assert call() == E_STATE and b"holds no consensus reads" in lib.mipgen_accel_last_error()
        assert fetch(0)[0] == E_STATE
        arr = capi.probe_array(arms)
        assert lib.mipgen_accel_reads_open_consensus(h, arr, n, 8, 0, 0, None, 0, 0, 0) == 0
        assert call() == E_STATE and fetch(0)[0] == E_STATE                                                     # before the finish
        assert lib.mipgen_accel_reads_finish_consensus(h, None, None, None, None, None, None) == 0
        assert fetch(0)[0] == E_STATE and b"no deletion alleles" in lib.mipgen_accel_last_error()                # reads, but no call yet
        assert call() == 0 and not counts.any() and not sites.any() and all(getattr(tot, k) == 0 for k in D.TOTAL_KEYS)        # zero groups give zeros
        assert fetch(0)[0] == 0 and fetch(1)[0] == E_INVALID
        got = a.consensus_reads(arms, ext, lig, eq, lq, tag_sizes=TAGS)[4]
        assert fetch(0)[0] == E_STATE                                                                           # new reads: the records went with the old ones
        counts[:] = -7; sites[:] = -7
        bad, long_ = lens.copy(), lens.copy()
        bad[1] = 0; long_[0] = 2049
        for kw in ({"seq_": None}, {"lens_": None}, {"n_": n - 1}, {"n_": n + 1}, {"lens_": bad}, {"lens_": long_}, {"row": -1}, {"row": 1}, {"mf": 0}, {"mq": -1},
                   {"mq": 41}, {"W": 0}, {"W": 16}, {"W": -1}):
            assert call(**kw) == E_INVALID, kw
        assert call(W=16) == E_INVALID and b"max_indel 16" in lib.mipgen_accel_last_error()
        assert (counts == -7).all() and (sites == -7).all() and fetch(0)[0] == E_STATE
        w_sites, w_records, w_totals = D.deletions(got, mols, n, 0, W=4)
        n_rec = w_totals["alleles"]
        assert n_rec >= 4
        assert call() == 0 and np.array_equal(sites, w_sites) and np.array_equal(counts, G.pileup(got, mols, n, 0, W=4)[0])
        assert {k: getattr(tot, k) for k in D.TOTAL_KEYS} == w_totals
        for k in (0, n_rec - 1, n_rec + 1, -1):
            assert fetch(k)[0] == E_INVALID, k
        assert b"left %d" % n_rec in lib.mipgen_accel_last_error()
        assert lib.mipgen_accel_deletions_fetch(h, None, n_rec) == E_INVALID
        rc, rec = fetch(n_rec)
        assert rc == 0 and rec.tobytes() == w_records.tobytes()
        assert call(out=None, sit=None) == 0 and tot.alleles == n_rec and call(tot_=None) == 0 and np.array_equal(sites, w_sites)
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
    """A small table on both strands and FASTQ with planted deletions and insertions: the -pileup_deletions file byte for byte and the new last stderr line; the
    -pileup file, the -pileup_insertions file, the -call file and every other stderr line are those of the run without the option."""
    g = H.golden_genome()
    rng = np.random.default_rng(757 + with_barcodes)
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
        for k in range(5 + 3 * (p % 3)):
            tag = random_tag(rng, 8)
            Me = Ml = M
            if k % 3 == 1:
                Me = Ml = cut(30 + p, 1 + k % 4, M)                                                              # the same start, several lengths
            elif k % 3 == 2:
                Me = Ml = M[:30 + p] + (b"GAT", b"GAC", b"T")[k % 3] + M[30 + p:]
            elif k == 3:
                Me, Ml = cut(40, 3, M), cut(40, 2, M)                                                            # two reads that disagree on the extent
            Me, Ml = bytearray(Me), bytearray(Ml)
            if k % 2:
                t = int(rng.integers(24, 28))
                Me[t] = Ml[t] = b"ACGT"[(b"ACGT".index(Me[t]) + 1 + k % 3) & 3]
            index = barcodes[int(rng.integers(0, 2))] if rng.random() < 0.85 else random_tag(rng, 8)
            for m in range(1 + (k + p) % 3):
                e = tag[:5] + (bytes(Me) + PAD)[:95]
                l = tag[5:] + (R.revcomp(bytes(Ml)) + PAD)[:97]
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
        text, line = D.deletions_file(want[4], t_rows, lab, mf, mq, W)
        assert text.count(b"\n") > 3 and b"\t-\t" in text and b"\t+\t" in text and (W < 4 or any(f.split(b"\t")[7] == b"1" for f in text.splitlines()[1:]))
        p = _run(common + ["-pileup", "pile.tsv"] + gapped + ["-pileup_deletions", "del.tsv"], str(tmp_path))
        assert p.returncode == 0, p.stderr.decode()
        assert open(tmp_path / "del.tsv", "rb").read() == text
        assert p.stderr.decode() == base.stderr.decode() + line
        assert open(tmp_path / "pile.tsv", "rb").read() == open(tmp_path / "pile0.tsv", "rb").read() == G.pileup_file(want[4], t_rows, lab, mf, mq, W)[0]
        # with -pileup_insertions and -call beside it: those routes run unchanged and the deletions call feeds DEL only
        beside = ["-pileup_insertions", "ins0.tsv", "-call", "calls0.tsv"]
        base = _run(common + ["-pileup", "pile0.tsv"] + gapped + beside, str(tmp_path))
        assert base.returncode == 0, base.stderr.decode()
        p = _run(common + ["-pileup", "pile.tsv"] + gapped + ["-pileup_insertions", "ins.tsv", "-call", "calls.tsv", "-pileup_deletions", "del2.tsv"], str(tmp_path))
        assert p.returncode == 0, p.stderr.decode()
        assert open(tmp_path / "del2.tsv", "rb").read() == text and p.stderr.decode() == base.stderr.decode() + line
        assert open(tmp_path / "pile.tsv", "rb").read() == open(tmp_path / "pile0.tsv", "rb").read()
        assert open(tmp_path / "ins.tsv", "rb").read() == open(tmp_path / "ins0.tsv", "rb").read() == I.insertions_file(want[4], t_rows, lab, mf, mq, W)[0]
        assert open(tmp_path / "calls.tsv", "rb").read() == open(tmp_path / "calls0.tsv", "rb").read()
